"""The kernel-level radial-trunk cases, shared by test_radial_gpu.py (which
runs csrc/radial.hip on them) and test_radial_reference.py (which proves, on
the very same inputs and without a GPU, that each case can tell a broken
kernel from a right one). Inputs are drawn on the CPU from a generator
seeded by the case id, so both files see the same numbers. x, W0 and W3 are
bf16-representable: the kernel's input rounding is not part of any error."""
import zlib
from dataclasses import dataclass

import torch

import radial_ref as R

# ---- bands -----------------------------------------------------------------
# band = min(margin * max(e_decl, floor), cap). e_decl is the error of the
# f32 declared-rounding reference (radial_ref.py) against the exact f64 one
# on the same inputs: what a correct kernel with the declared bf16 storage
# points loses. floor = 1e-7, plus one bf16 ulp (2^-8 of the tensor's max)
# where the tensor is stored in bf16. Caps: what the suite asserted for this
# kernel before these tests existed (test_radial_trunk_kernel_vs_eager);
# they are conditions, not measurements. Margins: twice the largest
# kernel_err / max(e_decl, floor) measured over all cases on the MI355X
# (profiles/radial_parity.md): 2.14 forward (rs0 of offset0), 1.05 gradients
# (dg0 of offset3). None would mean not measured: the band is then the cap.
MARGIN_FWD = 4.28
MARGIN_GRAD = 2.11
E_FLOOR = 1e-7
BF16_ULP = 2.0 ** -8
CAP_FWD = 2e-2
CAP_GRAD = 5e-2
BF16_STORED = ('H', 'yh0', 'yh3')


def rel_err(a, b):
    denom = b.abs().max().clamp(min=1e-6)
    return ((a - b).abs().max() / denom).item()


def floor(case, name):
    bf16 = name in BF16_STORED or (name == 'dX' and case.x_bf16)
    return E_FLOOR + (BF16_ULP if bf16 else 0.)


def band(case, name, e_decl):
    fwd = name in R.FWD_NAMES
    margin, cap = (MARGIN_FWD, CAP_FWD) if fwd else (MARGIN_GRAD, CAP_GRAD)
    if margin is None:
        return cap
    return min(margin * max(e_decl, floor(case, name)), cap)


@dataclass(frozen=True)
class Case:
    id: str
    D: int
    E: int = 70
    params: str = 'init'    # init | trained | gamma0-g0 | gamma0-g3 | flatrow
    #                         | wide | offset0 | offset3
    need_x: bool = True
    x_bf16: bool = False
    dh: str = 'rand'        # rand | zero_tail

    @property
    def tail_start(self):
        """First row of the last (possibly partial) 32-edge block."""
        return (self.E - 1) // 32 * 32


def _cases():
    from se3_transformer_amd.ops import fused
    out = [Case(f'd{D}', D=D) for D in fused.RADIAL_TRUNK_DIMS]
    for D in (3, 21):
        for E in (1, 31, 32, 33, 64, 257):
            out.append(Case(f'e{E}-d{D}', D=D, E=E, params='trained'))
    for D in (1, 21):
        for need_x in (False, True):
            for x_bf16 in (False, True):
                out.append(Case(
                    f'needx{int(need_x)}-{"bf16" if x_bf16 else "fp32"}-d{D}',
                    D=D, params='trained', need_x=need_x, x_bf16=x_bf16))
    for kind in ('trained', 'gamma0-g0', 'gamma0-g3', 'flatrow', 'wide',
                 'offset0', 'offset3'):
        out.append(Case(kind, D=3, params=kind))
    out.append(Case('dhzero-tail', D=3, params='trained', dh='zero_tail'))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}

FLAT_ROWS = (0, 33, 69)     # flatrow: one in each block of E = 70
FLAT_B0 = 0.5
# wide: LayerNorm undoes any scale of x, so it is gamma that carries |z| to
# about 8 (test_radial_reference.py checks that both GELU tails are hit)
WIDE_GAMMA = 2.5
WIDE_X = 4.
# offset0 / offset3: b = OFFSET + N(0, OFFSET_JITTER), the weights scaled by
# a power of two (they stay bf16-representable) so that the pre-activations
# scatter by about 0.02 around the offset
OFFSET = 32.
OFFSET_JITTER = 0.01
OFFSET0_W_SCALE = 2.0 ** -5
OFFSET3_W_SCALE = 2.0 ** -5


def _bf16_values(t):
    return t.to(torch.bfloat16).float()


def make_inputs(case):
    """CPU tensors: x (E, D) fp32 or bf16, the eight fp32 parameters under
    RadialFunc's names, dH (E, 128) fp32, eps."""
    from se3_transformer_amd.models.core import RadialFunc
    seed = zlib.crc32(case.id.encode())
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        rp = RadialFunc(1, 1, 1, edge_dim=case.D - 1)
    n0, ln1, n3, ln4 = rp.net[0], rp.net[1], rp.net[3], rp.net[4]
    p = dict(W0=n0.weight, b0=n0.bias, g0=ln1.weight, be0=ln1.bias,
             W3=n3.weight, b3=n3.bias, g3=ln4.weight, be3=ln4.bias)
    p = {k: v.detach().clone() for k, v in p.items()}
    E, D, kind = case.E, case.D, case.params

    def randn(*shape):
        return torch.randn(*shape, generator=gen)

    x = randn(E, D)
    dH = randn(E, 128)
    if kind != 'init':
        for g, be in (('g0', 'be0'), ('g3', 'be3')):
            p[g] = 1. + 0.3 * randn(128)
            p[be] = 0.3 * randn(128)
    if kind == 'gamma0-g0':
        p['g0'] = torch.zeros(128)
    elif kind == 'gamma0-g3':
        p['g3'] = torch.zeros(128)
    elif kind == 'flatrow':
        x[list(FLAT_ROWS)] = 0.
        p['b0'] = torch.full((128,), FLAT_B0)
    elif kind == 'wide':
        x = x * WIDE_X
        p['g0'] = WIDE_GAMMA * (1. + 0.1 * randn(128))
        p['g3'] = WIDE_GAMMA * (1. + 0.1 * randn(128))
    elif kind == 'offset0':
        p['W0'] = p['W0'] * OFFSET0_W_SCALE
        p['b0'] = OFFSET + OFFSET_JITTER * randn(128)
    elif kind == 'offset3':
        p['W3'] = p['W3'] * OFFSET3_W_SCALE
        p['b3'] = OFFSET + OFFSET_JITTER * randn(128)
    if case.dh == 'zero_tail':
        dH[case.tail_start:] = 0.
    p['W0'], p['W3'] = _bf16_values(p['W0']), _bf16_values(p['W3'])
    x = _bf16_values(x)
    if case.x_bf16:
        x = x.to(torch.bfloat16)
    return dict(x=x, dH=dH, eps=ln1.eps, **p)


PARAM_NAMES = ('W0', 'b0', 'g0', 'be0', 'W3', 'b3', 'g3', 'be3')


def reference(inp, dtype=torch.float64, declared_rounding=False,
              trunk=R.Trunk):
    """(Forward, Grads) of radial_ref on a make_inputs() dict."""
    return R.radial_reference(inp['x'], *(inp[n] for n in PARAM_NAMES),
                              dH=inp['dH'], eps=inp['eps'], dtype=dtype,
                              declared_rounding=declared_rounding,
                              trunk=trunk)


def named(fwd, grads):
    out = dict(zip(R.FWD_NAMES, fwd))
    out.update(zip(R.GRAD_NAMES, grads))
    return out


def declared_errors(inp):
    """(exact f64 reference, e_decl) per tensor name, on the device the
    inputs are on."""
    ref = named(*reference(inp))
    decl = named(*reference(inp, torch.float32, True))
    return ref, {k: rel_err(decl[k].double(), ref[k]) for k in ref}
