"""GPU tests of pairconv_bwd_dh called directly, against an f64 reference on
the same bf16 inputs.

    dR[e,(m,c)] = sum_o g[m,e,o] u[c,e,o]       (rounded to bf16 by the kernel)
    dH[e,k]     = sum_n bf16(dR)[e,n] W[n,k]    (f32 MFMA accumulation)

g and u are drawn on grids coarse enough that dR is exact in f32 in any
summation order (see _dh_case), so bf16(dR) has one answer and the f64
reference rounds the very same dR. Every element of dH is then held to the
f32 accumulation bound over n.

The shapes walk the kernel's paths: one, two (nsplit = 2: two blocks add
into dH) and three mo-blocks (three tiles per chunk in one block: the g
staging wraps and the u registers live across tiles); one, two and three
urow chunks (u reload, both parities of the W ring); a full edge tile, a
ragged second tile, and two full tiles plus a 2-edge remainder.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

K = 128
SENTINEL = 12345.0
GUARD = 64 * K          # one edge tile of dH on either side


def _pad_o(x, OP):
    return torch.nn.functional.pad(x, (0, OP - x.shape[-1]))


def _grid(gen, step, lim, *shape):
    """Seeded normal values rounded to multiples of step, |x| <= lim."""
    x = torch.randn(*shape, generator=gen, device='cuda')
    return (torch.round(x / step) * step).clamp(-lim, lim)


def _launch_dh(ext, G, U, P1, E, mo, O):
    """dH in the middle of a sentinel-filled buffer, zeroed as the op
    expects: a store past row E (or before row 0) lands in a guard."""
    buf = torch.full((E * K + 2 * GUARD,), SENTINEL, device='cuda')
    dH = buf[GUARD:GUARD + E * K].view(E, K)
    dH.zero_()
    ext.pairconv_bwd_dh(G, U, P1, dH, mo, O)
    torch.cuda.synchronize()
    return buf, dH


_DH_CASES = {}


def _dh_case(O, mo, miF, E):
    """Inputs, the kernel's dH and the f64 reference of one shape, computed
    once and shared by the tests that read them.

    g is on the grid 1/4 in [-2, 2] and u on 1/8 in [-1, 1]: bf16 values. A
    product is a multiple of 1/32 and at most 2 in size, so any partial sum
    of the at most 7 products is a multiple of 1/32 below 16: 9 bits, exact
    in f32 whatever the order. dR16 = bf16(dR) is then the same in the
    kernel and in f64. W is plain bf16 noise."""
    key = (O, mo, miF, E)
    if key in _DH_CASES:
        return _DH_CASES[key]
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(9000 + 1000 * O + 7 * mo + miF + E)
    g = _grid(gen, 1 / 4, 2.0, mo, E, O).to(torch.bfloat16)
    u = _grid(gen, 1 / 8, 1.0, miF, E, O).to(torch.bfloat16)
    W = (torch.randn(mo * miF, K, generator=gen, device='cuda') / K ** 0.5) \
        .to(torch.bfloat16)
    G = _pad_o(g, OP).contiguous()
    U = _pad_o(u, OP).contiguous()
    P1 = fused._pack_w_dh(W, mo, miF)

    dR = torch.einsum('meo,ceo->emc', g.double(), u.double())     # (E, mo, miF)
    assert torch.equal(dR.float().double(), dR), 'dR must be exact in f32'
    assert torch.equal(dR * 32, torch.round(dR * 32)) and dR.abs().max() <= 14
    dR16 = dR.float().to(torch.bfloat16).double().reshape(E, mo * miF)
    ref = dR16 @ W.double()                                        # (E, K)
    mag = dR16.abs() @ W.double().abs()

    buf, dH = _launch_dh(ext, G, U, P1, E, mo, O)
    case = dict(ext=ext, G=G, U=U, P1=P1, OP=OP, ref=ref, mag=mag, buf=buf, dH=dH)
    _DH_CASES[key] = case
    return case


def _nsplit(mo, E):
    """The launcher's split of the mo-blocks over blocks that add into dH."""
    nmo, eblk = mo // 8, (E + 63) // 64
    ns = 16 if nmo % 16 == 0 else (8 if nmo % 8 == 0 else 1)
    while eblk * ns * 2 <= 1024 and ns * 2 <= nmo and nmo % (ns * 2) == 0:
        ns *= 2
    return ns


def _check(dH, buf, ref, mag, n_terms, what):
    sent = torch.tensor(SENTINEL, device='cuda')
    assert (buf[:GUARD] == sent).all() and (buf[-GUARD:] == sent).all(), \
        'store outside dH'
    # f32 accumulation over the n = mo*miF terms: each rounding is at most
    # 2^-24 of a partial sum that sum |dR16||W| bounds, so n * 2^-24 * mag;
    # 2^-23 leaves a factor 2 (and covers the one extra addition per split
    # block).
    bound = n_terms * 2.0 ** -23 * mag
    err = (dH.double() - ref).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print(f'dh {what}: worst |err|/bound = {worst:.4f}, '
          f'max |err| = {err.max().item():.3e}')
    # every element is held to the bound: none is excluded
    assert err.numel() == ref.numel()
    assert (err <= bound).all()


DH_SHAPES = [(O, mo, miF, E) for O in (1, 3, 5, 7) for mo in (8, 16, 24)
             for miF in (32, 64, 96) for E in (64, 71, 130)]


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E', DH_SHAPES)
def test_dh_vs_f64(O, mo, miF, E):
    c = _dh_case(O, mo, miF, E)
    assert _nsplit(mo, E) == (2 if mo == 16 else 1)
    _check(c['dH'], c['buf'], c['ref'], c['mag'], mo * miF,
           f'O={O} mo={mo} miF={miF} E={E}')


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E', [s for s in DH_SHAPES if s[1] != 16])
def test_dh_two_launches_bit_equal_without_split(O, mo, miF, E):
    """With nsplit = 1 one block owns each (e, k) sum, added once to the
    zeroed dH: nothing depends on the order of blocks."""
    c = _dh_case(O, mo, miF, E)
    assert _nsplit(mo, E) == 1
    _, dH2 = _launch_dh(c['ext'], c['G'], c['U'], c['P1'], E, mo, O)
    assert torch.equal(dH2, c['dH'])


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E', [s for s in DH_SHAPES if s[0] != 1])
def test_dh_accepts_zeroed_pad_lanes(O, mo, miF, E):
    """The layout promises zero pad lanes o in [O, OP). Copies of U and G
    whose pads are filled with zeros again are taken as before and give the
    same dH: the kernel contracts whole vectors and checks no lane."""
    c = _dh_case(O, mo, miF, E)
    U2, G2 = c['U'].clone(), c['G'].clone()
    U2[..., O:] = 0
    G2[..., O:] = 0
    assert torch.equal(U2, c['U']) and torch.equal(G2, c['G'])
    buf, dH2 = _launch_dh(c['ext'], G2, U2, c['P1'], E, mo, O)
    _check(dH2, buf, c['ref'], c['mag'], mo * miF,
           f'zeroed pads O={O} mo={mo} miF={miF} E={E}')
    if _nsplit(mo, E) == 1:
        assert torch.equal(dH2, c['dH'])
