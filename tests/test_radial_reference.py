"""CPU tests that keep the radial-trunk reference (tests/radial_ref.py)
honest.

1. With declared_rounding off, in f64, forward and every gradient are what
   autograd gives through RadialFunc(...).double()'s eager `hidden`.
2. Every edge the GPU cases of test_radial_gpu.py aim at can actually be
   seen by them: a mutant of the REFERENCE (one step broken the way a kernel
   could break it) differs from the true reference, on the case's exact
   inputs, in at least one checked tensor by at least 10x the band the GPU
   test may use there (the band formula of radial_cases.py with e_decl
   evaluated here and the committed margins). NaN counts as differing. The
   kernel is neither mutated nor run.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import radial_cases as C
import radial_ref as R
from fused_helpers import no_switches, switches  # noqa: F401


# ---- 1. reference vs autograd -------------------------------------------------

AUTOGRAD_CASES = ['d1', 'd25', 'e1-d3', 'e33-d21', 'trained', 'gamma0-g0',
                  'gamma0-g3', 'flatrow', 'wide', 'offset0', 'offset3',
                  'dhzero-tail', 'needx1-bf16-d21']


@pytest.mark.parametrize('case_id', AUTOGRAD_CASES)
def test_reference_is_autograd_through_the_module_f64(case_id):
    from se3_transformer_amd.models.core import RadialFunc
    case = C.BY_ID[case_id]
    inp = C.make_inputs(case)
    rp = RadialFunc(1, 1, 1, edge_dim=case.D - 1).double()
    by_name = {'net.0.weight': 'W0', 'net.0.bias': 'b0',
               'net.1.weight': 'g0', 'net.1.bias': 'be0',
               'net.3.weight': 'W3', 'net.3.bias': 'b3',
               'net.4.weight': 'g3', 'net.4.bias': 'be3'}
    with torch.no_grad():
        for n, p in rp.named_parameters():
            if n in by_name:
                p.copy_(inp[by_name[n]])
    x = inp['x'].double().requires_grad_(True)
    with switches(SE3_EAGER_RADIAL='1'):
        H = rp.hidden(x)
    H.backward(inp['dH'].double())
    fwd, grads = C.reference(inp)
    assert fwd.H.dtype == torch.float64
    assert C.rel_err(fwd.H, H.detach()) < 1e-10
    assert C.rel_err(grads.dX, x.grad) < 1e-10
    for n, p in rp.named_parameters():
        if n in by_name:
            got = getattr(grads, 'd' + by_name[n])
            assert got.shape == p.grad.shape
            assert C.rel_err(got, p.grad) < 1e-10, n
    # the saved tensors, against torch's own LayerNorm
    y0 = F.linear(x.detach(), inp['W0'].double(), inp['b0'].double())
    assert C.rel_err(fwd.yh0, F.layer_norm(y0, (128,), eps=inp['eps'])) < 1e-10
    rs0 = (y0.var(-1, unbiased=False) + inp['eps']).rsqrt()
    assert C.rel_err(fwd.rs0, rs0) < 1e-10


# ---- 2. every case discriminates ----------------------------------------------

class _OnePassF32(R.Trunk):
    """var = sum(y^2)/128 - mean^2 in fp32, in one LayerNorm."""
    layer = None

    def stats(self, y, layer):
        if layer != self.layer:
            return super().stats(y, layer)
        y32 = y.float()
        mean = y32.sum(-1, keepdim=True) * (1. / 128)
        var = (y32 * y32).sum(-1, keepdim=True) * (1. / 128) - mean * mean
        return mean.to(y.dtype), var.to(y.dtype)


class OnePassLN0(_OnePassF32):
    layer = 0


class OnePassLN3(_OnePassF32):
    layer = 3


class HalfStats(R.Trunk):
    """Statistics over 64 of the 128 features."""

    def stats(self, y, layer):
        return super().stats(y[:, :64], layer)


class NoEps(R.Trunk):
    def rstd(self, var, eps):
        return var ** -0.5


class Db3FromDz(R.Trunk):
    def db3(self, dz3, dy3):
        return dz3.sum(0)


class DgDbeSwapped(R.Trunk):
    def ln_param_grads(self, dz, yh):
        dg, dbe = super().ln_param_grads(dz, yh)
        return dbe, dg


class W3NotTransposed(R.Trunk):
    def da1(self, dy3, W3):
        return dy3 @ W3.t()


class Rs3InLN0(R.Trunk):
    def rs_in_ln0_backward(self, rs0, rs3):
        return rs3


class DxHalfK(R.Trunk):
    def dx(self, dy0, W0):
        return dy0[:, :64] @ W0[:64]


class DivideByGamma(R.Trunk):
    """The backward gets z and works back to yhat = (z - beta) / gamma."""

    def yhat_in_backward(self, yh_stored, g, be):
        return ((yh_stored * g + be) - be) / g


def _tail_rows_counted(case, inp):
    """Rows past E of the last block take part in the dW3 / db3 / dg3 sums
    as the x = 0 rows the kernel stages for them (their dH: the rows of dH
    from the top again). Rows do not interact otherwise, so this is the
    reference on the padded problem, for those three tensors."""
    pad = -case.E % 32
    rows = torch.arange(case.E, case.E + pad) % case.E
    big = dict(inp)
    big['x'] = torch.cat((inp['x'], torch.zeros(pad, case.D,
                                                dtype=inp['x'].dtype)))
    big['dH'] = torch.cat((inp['dH'], inp['dH'][rows]))
    ref = C.named(*C.reference(inp))
    padded = C.named(*C.reference(big))
    for name in ('dW3', 'db3', 'dg3'):
        ref[name] = padded[name]
    return ref


def _plain(c):
    return c.params in ('init', 'trained')


# mutant -> (how it is made, the cases it applies to)
MUTANTS = {
    'onepass_ln0': (OnePassLN0, lambda c: c.params == 'offset0'),
    'onepass_ln3': (OnePassLN3, lambda c: c.params == 'offset3'),
    'half_stats': (HalfStats, _plain),
    'no_eps': (NoEps, lambda c: c.params == 'flatrow'),
    'tail_rows_counted': (None, lambda c: _plain(c) and c.E % 32 != 0
                          and c.dh == 'rand'),
    'db3_from_dz': (Db3FromDz, _plain),
    'dg_dbe_swapped': (DgDbeSwapped, _plain),
    'w3_not_transposed': (W3NotTransposed, _plain),
    'rs3_in_ln0': (Rs3InLN0, _plain),
    'dx_half_k': (DxHalfK, lambda c: _plain(c) and c.need_x),
    'divide_by_gamma': (DivideByGamma, lambda c: c.params.startswith('gamma0')),
}
PAIRS = [(m, c.id) for m, (_, applies) in MUTANTS.items()
         for c in C.CASES if applies(c)]


def _checked(case):
    names = R.FWD_NAMES + R.GRAD_NAMES
    return [n for n in names if n != 'dX' or case.need_x]


@pytest.mark.parametrize('mutant,case_id', PAIRS)
def test_case_tells_mutant_from_reference(mutant, case_id):
    case = C.BY_ID[case_id]
    inp = C.make_inputs(case)
    ref, e_decl = C.declared_errors(inp)
    trunk = MUTANTS[mutant][0]
    if trunk is None:
        mut = _tail_rows_counted(case, inp)
    else:
        mut = C.named(*C.reference(inp, trunk=trunk))
    best = ('', 0.)
    for name in _checked(case):
        gap = C.rel_err(mut[name], ref[name])
        factor = math.inf if math.isnan(gap) else \
            gap / C.band(case, name, e_decl[name])
        if factor > best[1]:
            best = (name, factor)
    print(f'radial-mutant {mutant} {case_id}: {best[0]} moves '
          f'{best[1]:.3g} bands')
    assert best[1] >= 10, (f'{mutant} on {case_id}: at most {best[1]:.3g} '
                           f'bands ({best[0]}), needs 10')


def test_one_pass_variance_goes_negative_at_offset_64():
    """The second half of the defect: at offset 64 and scatter 0.01 the
    one-pass fp32 variance is negative in many rows, and its rsqrt NaN."""
    gen = torch.Generator().manual_seed(5)
    y = (64. + 0.01 * torch.randn(4096, 128, generator=gen)).float()
    _, var1 = OnePassLN0().stats(y, 0)
    _, var2 = R.Trunk().stats(y, 0)
    assert (var2 > 0).all()
    assert (var1 + 1e-5 < 0).sum() > 100


# ---- 3. the cases are what their names say -------------------------------------

def test_inputs_are_bf16_representable_and_repeatable():
    ids = [c.id for c in C.CASES]
    assert len(set(ids)) == len(ids)
    for case in C.CASES:
        assert case.E <= 300
        a, b = C.make_inputs(case), C.make_inputs(case)
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), (case.id, k)
        for k in ('x', 'W0', 'W3'):
            t = a[k].float()
            assert torch.equal(t.to(torch.bfloat16).float(), t), (case.id, k)
        assert a['x'].dtype == (torch.bfloat16 if case.x_bf16
                                else torch.float32)
        assert a['x'].shape == (case.E, case.D)


def test_case_coverage():
    from se3_transformer_amd.ops import fused
    plain = [c for c in C.CASES if c.E == 70 and c.params == 'init']
    assert {c.D for c in plain} == set(fused.RADIAL_TRUNK_DIMS)
    for D in (3, 21):
        assert {c.E for c in C.CASES if c.id.startswith('e') and c.D == D} \
            == {1, 31, 32, 33, 64, 257}
    for D in (1, 21):
        assert {(c.need_x, c.x_bf16) for c in C.CASES
                if c.id.startswith('needx') and c.D == D} \
            == {(a, b) for a in (False, True) for b in (False, True)}


def test_special_cases_have_their_property():
    def pre(case_id):
        inp = C.make_inputs(C.BY_ID[case_id])
        d = {k: (v.double() if torch.is_tensor(v) else v)
             for k, v in inp.items()}
        y0 = d['x'] @ d['W0'].t() + d['b0']
        fwd, _ = C.reference(inp)
        a1 = R.gelu(fwd.yh0 * d['g0'] + d['be0'])
        y3 = a1 @ d['W3'].t() + d['b3']
        return inp, d, y0, y3, fwd

    # flatrow: exactly zero variance, rs = eps^-1/2, also in fp32
    inp, d, y0, _, fwd = pre('flatrow')
    rows = list(C.FLAT_ROWS)
    assert (y0[rows] == C.FLAT_B0).all()
    assert torch.allclose(fwd.rs0[rows], torch.full((3,), inp['eps'] ** -0.5,
                                                    dtype=torch.float64),
                          rtol=1e-14, atol=0)
    f32, _ = C.reference(inp, torch.float32, True)
    assert (f32.yh0[rows] == 0).all()
    assert (fwd.rs0 < 100).sum() == 67

    # wide: |z| reaches about 8 in both layers, both GELU tails are hit
    inp, d, _, _, fwd = pre('wide')
    for yh, g, be in ((fwd.yh0, d['g0'], d['be0']), (fwd.yh3, d['g3'], d['be3'])):
        z = yh * g + be
        assert 6.5 < z.abs().max() < 11, z.abs().max()
        dg = R.dgelu(z)
        assert (dg.abs() < 1e-6).any() and ((dg - 1).abs() < 1e-6).any()

    # offsets: a common offset, the scatter small against it
    for case_id, which in (('offset0', 0), ('offset3', 1)):
        inp, d, y0, y3, fwd = pre(case_id)
        y = (y0, y3)[which]
        sd = y.std(-1)
        assert (y.mean(-1) - C.OFFSET).abs().max() < 0.1
        assert 0.005 < sd.min() and sd.max() < 0.06, (sd.min(), sd.max())
        # the f32 declared-rounding reference is finite and within the
        # forward cap on these inputs
        ref, e_decl = C.declared_errors(inp)
        f32 = C.named(*C.reference(inp, torch.float32, True))
        assert all(torch.isfinite(t).all() for t in f32.values())
        for name in R.FWD_NAMES:
            assert e_decl[name] < C.CAP_FWD, (case_id, name, e_decl[name])
        for name in R.GRAD_NAMES:
            assert e_decl[name] < C.CAP_GRAD, (case_id, name, e_decl[name])

    # gamma0: the zero gamma is exactly zero
    assert (C.make_inputs(C.BY_ID['gamma0-g0'])['g0'] == 0).all()
    assert (C.make_inputs(C.BY_ID['gamma0-g3'])['g3'] == 0).all()

    # dhzero-tail: the rows of the last block carry no gradient
    case = C.BY_ID['dhzero-tail']
    inp = C.make_inputs(case)
    assert case.tail_start == 64
    assert (inp['dH'][64:] == 0).all() and (inp['dH'][:64] != 0).any()
    _, grads = C.reference(inp)
    assert (grads.dX[64:] == 0).all() and (grads.dX[:64] != 0).all()


def test_declared_rounding_costs_what_bf16_costs():
    """e_decl of the bf16-stored tensors is of the size of one bf16
    rounding, so the bands are about the kernel's format and not loose."""
    for case_id in ('d3', 'e257-d21', 'trained'):
        _, e_decl = C.declared_errors(C.make_inputs(C.BY_ID[case_id]))
        for name in C.BF16_STORED:
            assert 2.0 ** -11 < e_decl[name] < 2.0 ** -7, (name, e_decl[name])
        assert e_decl['rs0'] < 1e-5
