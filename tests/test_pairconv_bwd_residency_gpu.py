"""GPU tests of the pairconv backward after the du residency change:

* pairconv_bwd_du keeps its sums in registers and writes dU (miF, E, OP)
  in bf16 (rounded once, to nearest even) or in f32;
* the four ubuild backward kernels read dU in either dtype;
* pairconv_bwd_dw also sums db from the f32 dR entries it builds.

The du tests hold every element to a bound built from an f64 reference on
the same bf16 inputs. H, W and bias are drawn on grids coarse enough that
R = H @ W^T + bias is exact in f32 in any summation order (see _du_case),
so "R rounded to bf16 as the kernel rounds it" has one answer and the f64
reference rounds the very same R.
"""
import os
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

K = 128
SENTINEL = 12345.0


def _pad_o(x, OP):
    return torch.nn.functional.pad(x, (0, OP - x.shape[-1]))


def _rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def _grid(gen, step, lim, *shape, scale=1.0):
    """Seeded normal values rounded to multiples of step, |x| <= lim."""
    x = torch.randn(*shape, generator=gen, device='cuda') * scale
    return (torch.round(x / step) * step).clamp(-lim, lim)


_DU_CASES = {}


def _du_case(O, mo, miF, E):
    """Inputs, both kernel outputs and the f64 reference of one du shape,
    computed once and shared by the tests that read them.

    H is on the grid 1/4 in [-2, 2] (5 significant bits), W on 1/64 in
    [-1/2, 1/2] (6 bits), bias on 1/16 in [-2, 2]: all bf16 values. A
    product is a multiple of 2^-8 and at most 1 in size, so a partial sum of
    the 128 products, and that sum plus the bias, is a multiple of 2^-8
    below 2^8: 16 bits, exact in f32 whatever the order. R16 = bf16(R) is
    then the same in the kernel and in f64."""
    key = (O, mo, miF, E)
    if key in _DU_CASES:
        return _DU_CASES[key]
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(7000 + 100 * O + mo + miF + E)
    H = _grid(gen, 1 / 4, 2.0, E, K).to(torch.bfloat16)
    W = _grid(gen, 1 / 64, 0.5, mo * miF, K, scale=K ** -0.5).to(torch.bfloat16)
    bias = _grid(gen, 1 / 16, 2.0, mo * miF)
    g = torch.randn(mo, E, O, generator=gen, device='cuda').to(torch.bfloat16)
    G = _pad_o(g, OP).contiguous()
    P = fused._pack_w_fwd(W, mo, miF)

    R = H.double() @ W.double().t() + bias.double()          # (E, mo*miF)
    assert torch.equal(R.float().double(), R), 'R must be exact in f32'
    R16 = R.to(torch.bfloat16).double().view(E, mo, miF)
    ref = torch.einsum('emc,meo->ceo', R16, g.double())      # (miF, E, O)
    mag = torch.einsum('emc,meo->ceo', R16.abs(), g.double().abs())

    outs = {}
    for dt in (torch.bfloat16, torch.float32):
        # dU is the middle of a larger buffer: rows e >= E do not exist, so
        # a store past the ragged tile would land in a guard
        guard = 64 * OP
        buf = torch.full((miF * E * OP + 2 * guard,), SENTINEL, dtype=dt,
                         device='cuda')
        dU = buf[guard:guard + miF * E * OP].view(miF, E, OP)
        ext.pairconv_bwd_du(H, P, bias, G, dU, mo, O)
        torch.cuda.synchronize()
        outs[dt] = (buf, guard, dU)
    _DU_CASES[key] = (ref, mag, outs)
    return _DU_CASES[key]


DU_SHAPES = [(O, mo, miF, E) for O in (1, 3, 5, 7) for mo in (8, 16)
             for miF in (32, 64) for E in (64, 71)]


def _check_du(O, mo, miF, E, dt, rel):
    ref, mag, outs = _du_case(O, mo, miF, E)
    buf, guard, dU = outs[dt]
    assert dU.shape[2] >= O
    sent = torch.tensor(SENTINEL, dtype=dt, device='cuda')
    assert (buf[:guard] == sent).all() and (buf[-guard:] == sent).all(), \
        'store outside dU'
    assert torch.equal(dU[..., O:], torch.zeros_like(dU[..., O:])), \
        'dU pad lanes must be exactly zero'
    val = dU[..., :O].double()
    # f32 fma chain over mo terms: each of the mo roundings is at most
    # 2^-24 of a partial sum that sum|R||g| bounds, so mo * 2^-24 * mag;
    # 2^-23 leaves a factor 2. The bf16 store adds half an ulp, at most
    # 2^-9 |stored value|; 2^-8 |dU| covers it measured on the reference.
    bound = rel * ref.abs() + mo * 2.0 ** -23 * mag
    err = (val - ref).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print(f'du {dt} O={O} mo={mo} miF={miF} E={E}: worst |err|/bound = '
          f'{worst:.3f}, max |err| = {err.max().item():.3e}')
    # every element is held to the bound: none is excluded, and a valid
    # element left at the sentinel is far outside it
    assert err.numel() == miF * E * O
    assert (err <= bound).all()


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E', DU_SHAPES)
def test_du_bf16_out_vs_f64(O, mo, miF, E):
    """One and two mo-blocks, one and two urow chunks, a full edge tile and
    a ragged second one, every O."""
    _check_du(O, mo, miF, E, torch.bfloat16, 2.0 ** -8)


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E', DU_SHAPES)
def test_du_f32_out_vs_f64_and_rounds_to_the_bf16_out(O, mo, miF, E):
    _check_du(O, mo, miF, E, torch.float32, 0.0)
    _, _, outs = _du_case(O, mo, miF, E)
    # the store's rounding only: the same register sums, rounded by torch
    assert torch.equal(outs[torch.float32][2].to(torch.bfloat16),
                       outs[torch.bfloat16][2])


@needs_gpu
@pytest.mark.parametrize('O,I,F_', [(1, 1, 1), (3, 3, 3), (7, 3, 3), (7, 7, 7)])
def test_ubuild_backward_reads_bf16_du(O, I, F_):
    """Each ubuild backward kernel on bf16 dU is bit-equal to its f32 form
    on dU16.float(). gather_dx has one edge per node, so its atomic sums
    have one term and no order."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    C, E = 32, 33
    N = E + 3
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(100 * O + 10 * I + F_)
    B = torch.randn(E, O, I, F_, generator=gen, device='cuda')
    # the pad lanes carry a cotangent too
    dU16 = torch.randn(C * F_, E, OP, generator=gen, device='cuda') \
        .to(torch.bfloat16)
    dU32 = dU16.float()
    rows = torch.randperm(N, generator=gen, device='cuda')[:E].to(torch.int32)
    Xn = torch.randn(N, C, I, generator=gen, device='cuda')

    def run(dU):
        out = {}
        for xdt in (torch.float32, torch.bfloat16):
            dX = torch.full((E, C, I), 7.0, dtype=xdt, device='cuda')
            ext.ubuild_bwd_dx(B, dU, dX, O, I, F_)
            out['dx', xdt] = dX
            X = Xn[rows.long()].to(xdt).contiguous()
            dB = torch.full((E, O, I, F_), 7.0, device='cuda')
            ext.ubuild_bwd_db(X, dU, dB, O, I, F_)
            out['db', xdt] = dB
            dBg = torch.full((E, O, I, F_), 7.0, device='cuda')
            ext.ubuild_gather_bwd_db(Xn.to(xdt), rows, dU, dBg, O, I, F_)
            out['gather_db', xdt] = dBg
        dXn = torch.zeros(N, C, I, device='cuda')
        ext.ubuild_gather_bwd_dx(B, dU, rows, dXn, O, I, F_)
        out['gather_dx'] = dXn
        return out

    a, b = run(dU16), run(dU32)
    for key in b:
        assert torch.equal(a[key], b[key]), key
    assert a['gather_dx'].abs().max() > 0


@needs_gpu
@pytest.mark.parametrize('O', [1, 3, 5, 7])
@pytest.mark.parametrize('mo,miF,E', [(mo, miF, E) for mo in (4, 8)
                                      for miF in (32, 64) for E in (33, 70)])
def test_db_from_dw(O, mo, miF, E):
    """db[(m, c)] = sum_{e,o} g u summed by the dw kernel in f32, against
    f64 on the bf16 inputs: E*O products, each exact in f32, added with at
    most one rounding each, so E*O * 2^-24 * sum|g||u|; 2^-23 leaves a
    factor 2. dW does not depend on whether db is wanted."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(31 * O + mo + miF + E)

    def r16(*shape):
        return torch.randn(*shape, generator=gen, device='cuda') \
            .to(torch.bfloat16)

    g, u = r16(mo, E, O), r16(miF, E, O)
    G, U = _pad_o(g, OP).contiguous(), _pad_o(u, OP).contiguous()
    Ht = r16(K, E)
    dW0 = torch.full((mo * miF, K), 7.0, device='cuda')
    ext.pairconv_bwd_dw(G, U, Ht, dW0, torch.empty(0, device='cuda'), mo, O)
    dW1 = torch.full((mo * miF, K), -7.0, device='cuda')
    db = torch.full((mo * miF,), SENTINEL, device='cuda')
    ext.pairconv_bwd_dw(G, U, Ht, dW1, db, mo, O)
    assert torch.equal(dW0, dW1), 'dW changed with db'

    ref = torch.einsum('meo,ceo->mc', g.double(), u.double()).reshape(-1)
    mag = torch.einsum('meo,ceo->mc', g.double().abs(),
                       u.double().abs()).reshape(-1)
    bound = E * O * 2.0 ** -23 * mag
    err = (db.double() - ref).abs()
    print(f'db from dw O={O} mo={mo} miF={miF} E={E}: worst |err|/bound = '
          f'{(err / bound.clamp(min=1e-300)).max().item():.3f}')
    assert (err <= bound).all()


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@needs_gpu
@pytest.mark.parametrize('O,I,F_', [(3, 3, 3), (7, 7, 7)])
def test_fused_pairconv_opad_bf16_du_vs_torch_bwd(O, I, F_):
    """ubuild_opad -> fused_pairconv_opad at dim 32, E = 71: dU reaches the
    ubuild backward in bf16, and dx and db match the SE3_TORCH_BWD=1 path
    inside the bands of tests/test_opad_layout_gpu.py (db 2e-2, and the
    ubuild dX band 3e-2; dU 1e-2)."""
    from se3_transformer_amd.ops import fused
    E, C, mo = 71, 32, 32
    miF = C * F_
    gen = torch.Generator('cuda').manual_seed(17 + O)

    def r16(*shape):
        return torch.randn(*shape, generator=gen, device='cuda') \
            .to(torch.bfloat16).float()

    x0, B = r16(E, C, I), torch.randn(E, O, I, F_, generator=gen, device='cuda')
    H0, W0, bias0 = r16(E, K), r16(mo * miF, K) / K ** 0.5, r16(mo * miF)
    gout = r16(E, mo, O)

    def grads(torch_bwd):
        with _env(SE3_TORCH_BWD='1' if torch_bwd else None):
            x = x0.clone().requires_grad_()
            bias = bias0.clone().requires_grad_()
            U = fused.ubuild_opad(x, B, O, I, F_)
            U.retain_grad()
            out = fused.fused_pairconv_opad(H0, W0, bias, U, mo, O)
            out.backward(gout)
        return x.grad, bias.grad, U.grad

    dx, db, dU = grads(False)
    dx_t, db_t, dU_t = grads(True)
    assert dU.dtype == torch.bfloat16 and dU.shape == (miF, E, fused.opad(O))
    assert torch.equal(dU[..., O:], torch.zeros_like(dU[..., O:]))
    errs = {'dx': _rel_err(dx, dx_t), 'db': _rel_err(db, db_t),
            'dU': _rel_err(dU.float(), dU_t.float())}
    print(f'opad vs torch bwd ({O},{I},{F_}): '
          + ' '.join(f'{k}={v:.3e}' for k, v in errs.items()))
    assert errs['dx'] < 3e-2 and errs['db'] < 2e-2 and errs['dU'] < 1e-2
