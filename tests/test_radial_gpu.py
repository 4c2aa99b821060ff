"""Kernel-level GPU tests of csrc/radial.hip against the f64 reference of
tests/radial_ref.py, on the cases of tests/radial_cases.py, plus the
routing of RadialFunc.hidden to the kernel or away from it.

Bands (radial_cases.py): margin x max(e_decl, floor), never above the cap,
where e_decl is what the f32 reference with the kernel's declared bf16
storage points loses against exact f64 math on the same inputs, computed
here on the device. The margins are twice the largest kernel_err / e_decl
measured over all cases; the table is in profiles/radial_parity.md.
test_radial_reference.py proves without a GPU that each case separates a
broken kernel from a right one by at least 10x these bands.
"""
import pytest
import torch

import radial_cases as C
import radial_ref as R
from fused_helpers import no_switches, switches  # noqa: F401

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

SENTINEL = 777.


def _to_dev(inp):
    return {k: (t.cuda() if torch.is_tensor(t) else t) for k, t in inp.items()}


def _params(inp):
    return [inp[n].detach().clone().requires_grad_(True)
            for n in C.PARAM_NAMES]


def run_wrapper(case, inp):
    """One forward + backward of fused.radial_trunk. Returns the tensors by
    the reference's names (dX missing when the case does not ask for it)."""
    from se3_transformer_amd.ops import fused
    x = inp['x'].detach().clone().requires_grad_(case.need_x)
    params = _params(inp)
    H = fused.radial_trunk(x, *params, inp['eps'])
    assert H.dtype == torch.bfloat16 and H.shape == (case.E, 128)
    H.backward(inp['dH'])
    out = {'H': H.detach()}
    if case.need_x:
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
        out['dX'] = x.grad
    else:
        assert x.grad is None
    for n, p in zip(C.PARAM_NAMES, params):
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        out['d' + n] = p.grad
    return out


def kernel_inputs(inp):
    """What _RadialTrunkFn.forward hands the extension."""
    x16 = inp['x'].contiguous().to(torch.bfloat16)
    w0 = inp['W0'].contiguous().to(torch.bfloat16)
    w3 = inp['W3'].contiguous().to(torch.bfloat16)
    p0 = torch.cat([inp['b0'], inp['g0'], inp['be0']]).contiguous()
    p3 = torch.cat([inp['b3'], inp['g3'], inp['be3']]).contiguous()
    return x16, w0, p0, w3, p3


def run_forward_direct(case, inp):
    """One direct radial_trunk_fwd call: what the forward saves."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    x16, w0, p0, w3, p3 = kernel_inputs(inp)
    H = torch.empty(case.E, 128, dtype=torch.bfloat16, device='cuda')
    yh0, yh3 = torch.empty_like(H), torch.empty_like(H)
    rs = torch.empty(2, case.E, dtype=torch.float32, device='cuda')
    ext.radial_trunk_fwd(x16, w0, p0, w3, p3, H, yh0, yh3, rs, inp['eps'])
    return {'H': H, 'yh0': yh0, 'yh3': yh3, 'rs0': rs[0], 'rs3': rs[1]}


def measure(case):
    """Per tensor: (kernel_err, e_decl, rerun_diff), plus the raw results."""
    inp = _to_dev(C.make_inputs(case))
    ref, e_decl = C.declared_errors(inp)
    got = run_wrapper(case, inp)
    again = run_wrapper(case, inp)
    saved = run_forward_direct(case, inp)
    assert torch.equal(saved.pop('H'), got['H'])
    got.update(saved)
    errs = {}
    for name in R.FWD_NAMES + R.GRAD_NAMES:
        if name not in got:
            continue
        a, b = got[name].double(), again.get(name, got[name]).double()
        errs[name] = (max(C.rel_err(a, ref[name]), C.rel_err(b, ref[name])),
                      e_decl[name], C.rel_err(a, b))
    return errs, inp, ref, got


@needs_gpu
@pytest.mark.parametrize('case', C.CASES, ids=lambda c: c.id)
def test_radial_kernel_vs_f64_reference(case):
    errs, inp, ref, got = measure(case)
    bad = []
    for name, (kerr, e_decl, rerun) in errs.items():
        lim = C.band(case, name, e_decl)
        ratio = kerr / max(e_decl, C.floor(case, name))
        print(f'radial-parity {case.id} {name} kernel={kerr:.3e} '
              f'e_decl={e_decl:.3e} ratio={ratio:.2f} rerun={rerun:.3e} '
              f'band={lim:.3e}')
        if not kerr <= lim:
            bad.append(f'{name}: {kerr:.3e} > band {lim:.3e} '
                       f'(e_decl {e_decl:.3e})')
        if not rerun <= lim:
            bad.append(f'{name}: run-to-run {rerun:.3e} > band {lim:.3e}')
    assert not bad, '; '.join(bad)
    assert ('dX' in errs) == case.need_x

    if case.params == 'flatrow':
        rows = list(C.FLAT_ROWS)
        assert (got['yh0'][rows] == 0).all()
        want = torch.full((3,), inp['eps'] ** -0.5, device='cuda')
        assert C.rel_err(got['rs0'][rows], want) < 1e-6
    if case.params == 'gamma0-g0':
        # dy0 = rs0 (dz g0 - ...) with g0 = 0: exact zeros, no NaN
        for name in ('dX', 'dW0', 'db0'):
            assert not got[name].any(), name
    if case.params == 'gamma0-g3':
        for name in ('dX', 'dW0', 'db0', 'dg0', 'dbe0', 'dW3', 'db3'):
            assert not got[name].any(), name
    if case.dh == 'zero_tail':
        assert not got['dX'][case.tail_start:].any()


@needs_gpu
@pytest.mark.parametrize('E', [1, 33, 70])
def test_radial_kernels_write_nothing_past_row_E(E):
    """The extension gets outputs that are leading slices of larger
    sentinel-filled buffers of the test's own; what lies behind row E (and
    behind the 2 E floats of rs01, the E D floats of dX) stays as it was."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    case = C.Case(f'sentinel-e{E}', D=3, E=E, params='trained')
    inp = _to_dev(C.make_inputs(case))
    x16, w0, p0, w3, p3 = kernel_inputs(inp)
    plain = run_forward_direct(case, inp)

    bufs = [torch.full((E + 32, 128), SENTINEL, dtype=torch.bfloat16,
                       device='cuda') for _ in range(3)]
    H, yh0, yh3 = (b[:E] for b in bufs)
    rs_flat = torch.full((2 * E + 64,), SENTINEL, device='cuda')
    rs = rs_flat[:2 * E].view(2, E)
    ext.radial_trunk_fwd(x16, w0, p0, w3, p3, H, yh0, yh3, rs, inp['eps'])
    torch.cuda.synchronize()
    for b, name in zip(bufs, ('H', 'yh0', 'yh3')):
        assert (b[E:] == SENTINEL).all(), name
        assert torch.equal(b[:E], plain[name]), name
    assert (rs_flat[2 * E:] == SENTINEL).all()
    # rs01[1] starts exactly at offset E
    assert torch.equal(rs_flat[:E], plain['rs0'])
    assert torch.equal(rs_flat[E:2 * E], plain['rs3'])
    ref, e_decl = C.declared_errors(inp)
    for name, t in (('rs0', rs_flat[:E]), ('rs3', rs_flat[E:2 * E])):
        assert C.rel_err(t.double(), ref[name]) \
            <= C.band(case, name, e_decl[name]), name

    D = case.D
    dx_flat = torch.full((E * D + 64,), SENTINEL, device='cuda')
    dx_flat[:E * D] = 0.
    dX = dx_flat[:E * D].view(E, D)
    dW0 = torch.zeros(128, D, device='cuda')
    dW3 = torch.zeros(128, 128, device='cuda')
    dp0, dp3 = torch.zeros(384, device='cuda'), torch.zeros(384, device='cuda')
    dH16 = inp['dH'].contiguous().to(torch.bfloat16)
    ext.radial_trunk_bwd(dH16, x16, w0, p0, w3, w3.t().contiguous(), p3,
                         plain['yh0'], plain['yh3'], rs.contiguous(),
                         dW0, dp0, dW3, dp3, dX, inp['eps'])
    torch.cuda.synchronize()
    assert (dx_flat[E * D:] == SENTINEL).all()
    assert C.rel_err(dX.double(), ref['dX']) \
        <= C.band(case, 'dX', e_decl['dX'])


class _Calls:
    """Counts the calls of ops.fused.radial_trunk."""

    def __init__(self, monkeypatch):
        from se3_transformer_amd.ops import fused
        self.n = 0
        real = fused.radial_trunk

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(fused, 'radial_trunk', counted)


@needs_gpu
def test_radial_module_routing(monkeypatch):
    """RadialFunc.hidden takes the kernel at every instantiated width, and
    stays eager at a width that is not, at mid_dim 64, and when the two
    LayerNorms differ in eps."""
    from se3_transformer_amd.models.core import RadialFunc
    from se3_transformer_amd.ops import fused
    calls = _Calls(monkeypatch)
    torch.manual_seed(11)
    for D in fused.RADIAL_TRUNK_DIMS:
        rp = RadialFunc(1, 2, 2, edge_dim=D - 1).cuda()
        h = rp.hidden(torch.randn(2, 5, D, device='cuda'))
        assert h.shape == (2, 5, 128) and h.dtype == torch.bfloat16
    assert calls.n == len(fused.RADIAL_TRUNK_DIMS)

    calls.n = 0
    x = torch.randn(2, 5, 4, device='cuda')
    h = RadialFunc(1, 2, 2, edge_dim=3).cuda().hidden(x)
    assert h.shape == (2, 5, 128) and h.dtype == torch.float32
    h = RadialFunc(1, 2, 2, edge_dim=2, mid_dim=64).cuda().hidden(x[..., :3])
    assert h.shape == (2, 5, 64) and h.dtype == torch.float32
    rp = RadialFunc(1, 2, 2, edge_dim=2).cuda()
    rp.net[4].eps = 1e-3
    h = rp.hidden(x[..., :3])
    assert h.dtype == torch.float32
    assert calls.n == 0
    rp.net[1].eps = 1e-3
    assert rp.hidden(x[..., :3]).dtype == torch.bfloat16 and calls.n == 1
