"""Native differentiable-coordinates path (`pytest -m gpu`).

Covers the HIP backward of the fused SH+basis kernel (`sh_basis_bwd`), the
ubuild dB kernel (`ubuild_bwd_db`) and the kNN-kernel graph build under
`differentiable_coors=True`, each against the eager autograd path it
replaces (forced with SE3_EAGER_KNN / SE3_EAGER_BASIS / SE3_EAGER_UBUILD).

Error metric everywhere: max-abs difference / max-abs of the oracle.
Bounds are relative to the error the eager path itself makes against the
same higher-precision oracle, so they track the number format rather than
the implementation under test. Measured values: profiles/diffcoors_parity.md.
"""
import copy

import pytest
import torch

from se3_transformer_amd import SE3Transformer
from se3_transformer_amd.ops import fused
from se3_transformer_amd.ops.basis import get_basis_packed

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')]

EAGER_VARS = ('SE3_EAGER_KNN', 'SE3_EAGER_BASIS', 'SE3_EAGER_UBUILD')


def rel_err(a, ref):
    return ((a.double() - ref.double()).abs().max()
            / ref.double().abs().max()).item()


def set_eager(monkeypatch, names):
    for v in EAGER_VARS:
        if v in names:
            monkeypatch.setenv(v, '1')
        else:
            monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- sh_basis

def basis_grad(rel, cot, max_degree, dtype):
    """d/d rel of sum_k (basis[k] * G[k]).sum() in `dtype`."""
    r = rel.to(dtype).clone().requires_grad_()
    basis = get_basis_packed(r, max_degree, differentiable=True)
    loss = sum((basis[k] * cot[k].to(dtype)).sum() for k in basis)
    loss.backward()
    return r.grad, basis


def well_conditioned_rel(E):
    """rel ~ N(0,1) with rho >= 0.3 r (SH-frame rho^2 = z^2 + x^2): keeps the
    1/rho conditioning near the SH poles from dominating the comparison."""
    g = torch.Generator().manual_seed(1234)
    rel = torch.randn(E, 3, generator=g)
    while True:
        rho = (rel[:, 2] ** 2 + rel[:, 0] ** 2).sqrt()
        bad = rho < 0.3 * rel.norm(dim=-1)
        if not bad.any():
            return rel.cuda()
        rel[bad] = torch.randn(int(bad.sum()), 3, generator=g)


@pytest.mark.parametrize('max_degree', [1, 2, 3])
def test_sh_basis_bwd_matches_autograd(max_degree, monkeypatch):
    """bound: err_kernel <= max(8 * err_eager_fp32, 2e-6) against the f64
    eager oracle — both are fp32 evaluations of the same recurrences in a
    different order (factor 8); floor = fp32 eps x ~30-op recurrence depth."""
    rel = well_conditioned_rel(300)          # two 256-thread blocks, ragged tail
    set_eager(monkeypatch, ())
    with torch.no_grad():
        plain = get_basis_packed(rel, max_degree, differentiable=False)
    g = torch.Generator().manual_seed(99)
    cot = {k: torch.randn(v.shape, generator=g).cuda() for k, v in plain.items()}

    g_kernel, basis = basis_grad(rel, cot, max_degree, torch.float32)
    for k in plain:
        assert basis[k].grad_fn is not None
        assert torch.equal(basis[k], plain[k]), f'forward differs for pair {k}'
        assert not plain[k].requires_grad

    set_eager(monkeypatch, ('SE3_EAGER_BASIS',))
    g_ref, _ = basis_grad(rel, cot, max_degree, torch.float64)
    g_eager, _ = basis_grad(rel, cot, max_degree, torch.float32)

    err_eager = rel_err(g_eager, g_ref)
    err_kernel = rel_err(g_kernel, g_ref)
    print(f'sh_basis_bwd max_degree={max_degree}: err_kernel={err_kernel:.3e} '
          f'err_eager_fp32={err_eager:.3e}')
    assert torch.isfinite(g_kernel).all()
    assert err_kernel <= max(8 * err_eager, 2e-6)


def test_sh_basis_bwd_degenerate_rows(monkeypatch):
    """rel = 0 (invalid kNN slots), rel on the +-y axis (the SH pole) and a
    row inside the rho clamp: finite everywhere, exactly zero for the first
    three, and the bound of the test above against eager fp32 autograd."""
    max_degree = 2
    rel = torch.tensor([[0., 0., 0.], [0., 1., 0.], [0., -2., 0.],
                        [1e-13, 0.5, -1e-13], [0.3, -0.2, 0.9],
                        [1., 0., 0.], [0., 0., 1.], [-0.5, 0.4, -0.3]],
                       device='cuda')
    set_eager(monkeypatch, ())
    with torch.no_grad():
        plain = get_basis_packed(rel, max_degree)
    g = torch.Generator().manual_seed(7)
    cot = {k: torch.randn(v.shape, generator=g).cuda() for k, v in plain.items()}
    g_kernel, _ = basis_grad(rel, cot, max_degree, torch.float32)

    set_eager(monkeypatch, ('SE3_EAGER_BASIS',))
    g_eager, _ = basis_grad(rel, cot, max_degree, torch.float32)
    g_ref, _ = basis_grad(rel, cot, max_degree, torch.float64)

    assert torch.isfinite(g_kernel).all()
    assert (g_kernel[:3] == 0).all(), g_kernel[:3]
    err_eager = rel_err(g_eager, g_ref)
    err_kernel = rel_err(g_kernel, g_eager)
    print(f'degenerate rows: err_kernel_vs_eager={err_kernel:.3e} '
          f'err_eager_fp32={err_eager:.3e}')
    assert err_kernel <= max(8 * err_eager, 2e-6)


# ------------------------------------------------------------------ ubuild

def bf16_exact(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().float().cuda()


@pytest.mark.parametrize('x_dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('O,I,F', [(7, 7, 7), (3, 5, 3), (3, 1, 1)])
def test_ubuild_db(O, I, F, x_dtype):
    """x, B-independent cotangent G are bf16-representable, so every product
    of the dB sum is exact in fp32 and only the summation order over the
    C = 32 terms differs from the fp32 einsum: rel_err < 1e-5."""
    E, C = 50, 32                            # 16-edge blocks, ragged last one
    x0 = bf16_exact(E, C, I, seed=1).to(x_dtype)
    B0 = torch.randn(E, O, I, F, generator=torch.Generator().manual_seed(2)).cuda()
    G = bf16_exact(C * F, O, E, seed=3)

    def run(b_grad):
        x = x0.clone().requires_grad_()
        B = B0.clone().requires_grad_(b_grad)
        assert fused.ubuild_ok(B, C, O, I, F)
        out = fused.ubuild(x, B, O, I, F)
        (out.float() * G).sum().backward()
        return out.detach(), x.grad, B.grad

    out_plain, dx_plain, none_db = run(False)
    out_grad, dx_grad, db = run(True)
    assert none_db is None
    assert torch.equal(out_plain, out_grad)

    db_ref = torch.einsum('eci,cfoe->eoif', x0.float(), G.view(C, F, O, E))
    err = rel_err(db, db_ref)
    print(f'ubuild dB ({O},{I},{F}) x={x_dtype}: rel_err={err:.3e}')
    assert db.dtype == torch.float32 and db.shape == (E, O, I, F)
    assert err < 1e-5

    ulp = torch.finfo(x_dtype).eps * dx_plain.float().abs()
    assert ((dx_grad.float() - dx_plain.float()).abs() <= ulp).all()


# ------------------------------------------------------------------- model

def make_model(num_degrees):
    torch.manual_seed(5)
    return SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                          num_degrees=num_degrees, output_degrees=2,
                          num_neighbors=6, valid_radius=1.2,
                          differentiable_coors=True).cuda()


def make_inputs(b=2, n=40, dim=32, masked=5):
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(b, n, dim, generator=g).cuda()
    coors = torch.randn(b, n, 3, generator=g).cuda()
    mask = torch.ones(b, n, dtype=torch.bool)
    if masked:
        mask[:, -masked:] = False
    cot = torch.randn(b, n, dim, 3, generator=g).cuda()   # return_type=1 shape
    return feats, coors, mask.cuda(), cot


def run_model(model, inputs, dtype=torch.float32, autocast=False):
    feats, coors, mask, cot = inputs
    model.zero_grad(set_to_none=True)
    c = coors.to(dtype).clone().requires_grad_()
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        out = model(feats.to(dtype), c, mask, return_type=1)
    (out.to(dtype) * cot.to(dtype)).sum().backward()
    pgrad = torch.cat([p.grad.reshape(-1).double() for p in model.parameters()
                       if p.grad is not None])
    return out.detach(), c.grad, pgrad


def test_model_fp32_matches_f64_oracle(monkeypatch):
    """kNN kernel + sh_basis fwd/bwd in an fp32 model against the same
    weights in float64 eager. bound per quantity (output, coors.grad,
    parameter grads): err_new <= max(8 * err_parent, 2e-5), err_parent the
    error of the all-eager fp32 graph/basis path against the same oracle."""
    model = make_model(num_degrees=3)
    inputs = make_inputs()
    mask = inputs[2]

    set_eager(monkeypatch, ())
    new = run_model(model, inputs)
    set_eager(monkeypatch, ('SE3_EAGER_KNN', 'SE3_EAGER_BASIS'))
    parent = run_model(model, inputs)
    ref = run_model(copy.deepcopy(model).double(), inputs, dtype=torch.float64)

    assert torch.isfinite(new[1]).all()
    assert (new[1][~mask] == 0).all(), 'masked nodes must get zero coors.grad'
    for name, a, p, r in zip(('out', 'coors.grad', 'param grads'), new, parent, ref):
        assert a.shape == r.shape
        err_new, err_parent = rel_err(a, r), rel_err(p, r)
        print(f'model fp32 {name}: err_new={err_new:.3e} err_parent={err_parent:.3e}')
        assert err_new <= max(8 * err_parent, 2e-5), name


def test_model_bf16_autocast_all_fused(monkeypatch):
    """Every fused kernel on under autocast-bf16: the coors.grad error
    against the fp32 eager oracle stays within 4x that of the bf16 path
    with graph build, basis and ubuild forced eager."""
    model = make_model(num_degrees=2)
    inputs = make_inputs()

    set_eager(monkeypatch, ())
    _, g_new, _ = run_model(model, inputs, autocast=True)
    set_eager(monkeypatch, EAGER_VARS)
    _, g_parent, _ = run_model(model, inputs, autocast=True)
    _, g_ref, _ = run_model(model, inputs)

    assert torch.isfinite(g_new).all()
    err_new, err_parent = rel_err(g_new, g_ref), rel_err(g_parent, g_ref)
    print(f'model bf16 coors.grad: err_new={err_new:.3e} err_parent={err_parent:.3e}')
    assert err_new <= 4 * err_parent


def test_native_path_taken(monkeypatch):
    """The kNN kernel, sh_basis_bwd and the ubuild dB kernel all run, and
    the dense graph build is never entered: its (n, n-1) index table and
    self-removal gathers (the only producers of n^2-sized tensors in the
    model without adjacency inputs) are not called, at n=40 and at n=512."""
    from se3_transformer_amd.models import transformer as tr
    ext = fused._load_ext()
    calls = {}

    def spy(obj, name):
        real = getattr(obj, name)

        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return real(*a, **kw)
        monkeypatch.setattr(obj, name, wrapped, raising=True)

    for name in ('knn_graph', 'sh_basis_bwd', 'ubuild_bwd_db'):
        spy(ext, name)
    spy(tr, '_remove_self')
    spy(tr, '_off_diag_indices')

    set_eager(monkeypatch, ())
    model = make_model(num_degrees=2)
    _, g, _ = run_model(model, make_inputs(), autocast=True)
    assert torch.isfinite(g).all()
    for name in ('knn_graph', 'sh_basis_bwd', 'ubuild_bwd_db'):
        assert calls.get(name, 0) >= 1, f'{name} was not called'

    torch.manual_seed(5)
    big = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1, num_degrees=2,
                         output_degrees=2, num_neighbors=8,
                         differentiable_coors=True).cuda()
    _, g, _ = run_model(big, make_inputs(b=1, n=512, masked=0), autocast=True)
    assert torch.isfinite(g).all()
    assert calls.get('_remove_self', 0) == 0
    assert calls.get('_off_diag_indices', 0) == 0
