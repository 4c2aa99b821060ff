"""GPU tests of the pairconv and ubuild kernels on channel counts that are no
multiple of the MFMA tile (8 mo x 32 urows; csrc/pairconv_common.h).

The kernels run on tensors zero-padded to mo_p = ceil8(mo), miF_p =
ceil32(miF): packed W, bias, U and G are exactly zero outside the true
(mo, miF), while out, dW, db and dH have the true sizes and the kernels guard
their stores.

Groups:
1. fused_pairconv_opad on ragged tensors equals the same call on explicitly
   zero-padded aligned tensors, bit for bit (dH: 1e-5, split-K atomics), and
   the kernels called directly write nothing outside out, dW, db and dH;
2. the same results against an f64 reference that owes nothing to the
   aligned kernels;
3. pack_w_both and pack_g on ragged dims;
4. ubuild forward and backward for any channel count;
5. the switches on a ragged PairwiseConv;
6. ragged models run the kernels for every degree pair.

Inputs of groups 1 and 2 are on coarse grids (see _case): R = H W^T + bias,
dR = sum_o g u and the bias term sum_c bias u are then exact in f32 in any
summation order, so what the kernels round to bf16 has one value, the f64
reference rounds that very value, and the bias term's library GEMM gives the
same bits whatever its shape.
"""
import pytest
import torch

from fused_helpers import no_switches, switches  # noqa: F401

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

K = 128
SENTINEL = 12345.0

MOS = (1, 7, 9, 17, 24)          # mo_p = 8, 8, 16 (MB2 = 2, dh nsplit 2), 24, 24
MIFS = (1, 31, 33, 48, 65)       # one, two and three urow chunks
OS = (1, 3, 5, 7)
ES = (64, 71, 130)


def _shapes():
    """60 of the 300 combinations: every (mo, miF) pair twice, with O and E
    walking so that every (mo, O), (miF, O), (mo, E) and (miF, E) occurs, and
    the diagonal pairs twice more."""
    out = []
    for a, mo in enumerate(MOS):
        for b, miF in enumerate(MIFS):
            for r in (0, 2) + ((1, 3) if a == b else ()):
                out.append((mo, miF, OS[(a + b + r) % 4], ES[(a + 2 * b + r) % 3]))
    return out


SHAPES = _shapes()
assert len(SHAPES) == 60 and len(set(SHAPES)) == 60
assert {(s[0], s[2]) for s in SHAPES} == {(m, o) for m in MOS for o in OS}
assert {(s[1], s[2]) for s in SHAPES} == {(c, o) for c in MIFS for o in OS}
assert {(s[0], s[3]) for s in SHAPES} == {(m, e) for m in MOS for e in ES}
assert {(s[1], s[3]) for s in SHAPES} == {(c, e) for c in MIFS for e in ES}


def _rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def _grid(gen, step, lim, *shape, scale=1.0):
    """Seeded normal values rounded to multiples of step, |x| <= lim."""
    x = torch.randn(*shape, generator=gen, device='cuda') * scale
    return (torch.round(x / step) * step).clamp(-lim, lim)


def _pad_o(x, OP):
    return torch.nn.functional.pad(x, (0, OP - x.shape[-1]))


def _pad_mc(t, mo, miF, mo_p, miF_p):
    """(mo*miF, ...) -> (mo_p*miF_p, ...), zeros outside the true (mo, miF)."""
    p = t.new_zeros(mo_p, miF_p, *t.shape[1:])
    p[:mo, :miF] = t.view(mo, miF, *t.shape[1:])
    return p.view(mo_p * miF_p, *t.shape[1:])


def _run_fn(H, W, bias, U, gout, mo, O):
    """fused_pairconv_opad forward and backward: out, dH, dW, db, dU."""
    from se3_transformer_amd.ops import fused
    H, W, bias, U = (t.clone().requires_grad_() for t in (H, W, bias, U))
    out = fused.fused_pairconv_opad(H, W, bias, U, mo, O)
    out.backward(gout)
    torch.cuda.synchronize()
    return dict(out=out.detach(), dH=H.grad, dW=W.grad, db=bias.grad, dU=U.grad)


_CASES = {}


def _case(mo, miF, O, E):
    """Inputs and the Function's results on the ragged tensors of one shape,
    computed once and shared by the tests that read them.

    H is on the grid 1/4 in [-2, 2], W on 1/64 in [-1/2, 1/2], bias on 1/16
    in [-2, 2]: a product H W is a multiple of 2^-8 and at most 1, so any
    partial sum of the 128 products plus the bias is a multiple of 2^-8 below
    2^8: 16 bits, exact in f32 (tests/test_pairconv_bwd_residency_gpu.py).
    g is on 1/4 in [-2, 2] and u on 1/8 in [-1, 1]: the at most 7 products of
    dR are multiples of 1/32 and sum to less than 16, exact in f32
    (tests/test_pairconv_dh_gpu.py). bias u is a multiple of 2^-7 and at most
    2, and a sum of at most 65 of them is below 2^8: 15 bits, exact in f32.
    All of them are bf16 values, so the casts in the Function are exact."""
    key = (mo, miF, O, E)
    if key in _CASES:
        return _CASES[key]
    from se3_transformer_amd.ops import fused
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(5000 + 1000 * O + 31 * mo + 7 * miF + E)
    H = _grid(gen, 1 / 4, 2.0, E, K)
    W = _grid(gen, 1 / 64, 0.5, mo * miF, K, scale=K ** -0.5)
    bias = _grid(gen, 1 / 16, 2.0, mo * miF)
    u = _grid(gen, 1 / 8, 1.0, miF, E, O)
    g = _grid(gen, 1 / 4, 2.0, E, mo, O)
    for t in (H, W, bias, u, g):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    U = _pad_o(u, OP).to(torch.bfloat16).contiguous()
    c = dict(H=H, W=W, bias=bias, u=u, g=g, U=U, OP=OP,
             got=_run_fn(H, W, bias, U, g, mo, O))
    _CASES[key] = c
    return c


# --------------------------------------------------------------------------
# 1. ragged == zero-padded aligned
# --------------------------------------------------------------------------

@needs_gpu
@pytest.mark.parametrize('mo,miF,O,E', SHAPES)
def test_ragged_equals_padded_aligned(mo, miF, O, E):
    """The kernels see the same padded tensors either way and add exact
    zeros on the pads: the same sums in the same order. dH is summed by
    atomics where the mo-blocks are split (1e-5, as
    test_lowmem_pack_mode_matches_default)."""
    from se3_transformer_amd.ops import fused
    c = _case(mo, miF, O, E)
    mo_p, miF_p = fused.pad_dims(mo, miF)
    got = c['got']
    assert got['out'].shape == (E, mo, O)
    assert got['dW'].shape == (mo * miF, K) and got['db'].shape == (mo * miF,)
    assert got['dU'].shape == (miF, E, c['OP'])

    Wp = _pad_mc(c['W'], mo, miF, mo_p, miF_p)
    bp = _pad_mc(c['bias'], mo, miF, mo_p, miF_p)
    Up = torch.zeros(miF_p, E, c['OP'], dtype=torch.bfloat16, device='cuda')
    Up[:miF] = c['U']
    gp = torch.zeros(E, mo_p, O, device='cuda')
    gp[:, :mo] = c['g']
    pad = _run_fn(c['H'], Wp, bp, Up, gp, mo_p, O)

    assert torch.equal(got['out'], pad['out'][:, :mo])
    assert torch.equal(got['dW'].view(mo, miF, K),
                       pad['dW'].view(mo_p, miF_p, K)[:mo, :miF])
    assert torch.equal(got['db'].view(mo, miF),
                       pad['db'].view(mo_p, miF_p)[:mo, :miF])
    assert torch.equal(got['dU'], pad['dU'][:miF])
    assert _rel_err(got['dH'], pad['dH']) < 1e-5
    # what the padded run computes on the pads is exactly zero
    for name, t in (('out', pad['out'][:, mo:]),
                    ('dW', pad['dW'].view(mo_p, miF_p, K)[mo:]),
                    ('dW', pad['dW'].view(mo_p, miF_p, K)[:, miF:]),
                    ('db', pad['db'].view(mo_p, miF_p)[mo:]),
                    ('db', pad['db'].view(mo_p, miF_p)[:, miF:]),
                    ('dU', pad['dU'][miF:])):
        assert not t.any(), name


def _framed(shape, guard, fill=None):
    """A tensor in the middle of a sentinel-filled buffer, guard elements on
    either side: a store outside the tensor lands in a guard."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), SENTINEL, device='cuda')
    t = buf[guard:guard + n].view(*shape)
    if fill is not None:
        t.fill_(fill)
    return buf, t, guard


@needs_gpu
@pytest.mark.parametrize('mo,miF,O,E', SHAPES)
def test_ragged_kernels_store_inside_their_outputs(mo, miF, O, E):
    """The kernel sequence of the Function, called directly with out, dW, db
    and dH in sentinel-framed buffers of the TRUE sizes: the guards on both
    sides are untouched, every element inside is written, and dW, db (bit
    for bit) and dH are those of the Function."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    c = _case(mo, miF, O, E)
    OP = c['OP']
    mo_p, miF_p = fused.pad_dims(mo, miF)
    H16 = c['H'].to(torch.bfloat16)
    U16 = fused._pad_u_rows(c['U'], miF)
    Pf = torch.full((mo_p * miF_p * K,), SENTINEL, dtype=torch.bfloat16,
                    device='cuda')
    Pdh = torch.full_like(Pf, SENTINEL)
    ext.pack_w_both(c['W'], Pf, Pdh, mo)
    G = torch.full((mo_p, E, OP), SENTINEL, dtype=torch.bfloat16, device='cuda')
    ext.pack_g(c['g'].contiguous(), G)

    framed = {
        'out': _framed((E, mo, O), 64 * mo_p * O, 0.0),        # the kernel adds
        'dH': _framed((E, K), 64 * K, 0.0),                    # atomics
        'dW': _framed((mo, miF, K), 4 * 32 * K),               # one dw tile
        'db': _framed((mo * miF,), 4 * 32),
    }
    ext.pairconv_fwd_opad(H16, Pf, U16, framed['out'][1], mo_p)
    ext.pairconv_bwd_dh(G, U16, Pdh, framed['dH'][1], mo_p, O)
    ext.pairconv_bwd_dw(G, U16, H16.t().contiguous(), framed['dW'][1],
                        framed['db'][1], mo_p, O)
    torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL, device='cuda')
    for name, (buf, t, guard) in framed.items():
        assert (buf[:guard] == sent).all() and (buf[-guard:] == sent).all(), \
            f'store outside {name}'
        assert not (t == sent).any(), f'{name} has unwritten elements'
    got = c['got']
    assert torch.equal(framed['dW'][1].view(mo * miF, K), got['dW'])
    assert torch.equal(framed['db'][1], got['db'])
    assert _rel_err(framed['dH'][1], got['dH']) < 1e-5
    # out of the Function = its bias term + what the kernel adds
    b16 = c['bias'].to(torch.bfloat16).view(mo, miF)
    bt = (b16 @ c['U'].view(miF, E * OP)).view(mo, E, OP)[:, :, :O] \
        .permute(1, 0, 2).float()
    assert torch.equal(bt + framed['out'][1], got['out'])


# --------------------------------------------------------------------------
# 2. against f64
# --------------------------------------------------------------------------

def _held(name, val, ref, bound, what):
    err = (val.double() - ref).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print(f'{name} {what}: worst |err|/bound = {worst:.4f}, '
          f'max |err| = {err.max().item():.3e}')
    # every element is held to the bound: none is excluded
    assert err.numel() == ref.numel() and val.shape == ref.shape
    assert (err <= bound).all(), name


@needs_gpu
@pytest.mark.parametrize('mo,miF,O,E', SHAPES)
def test_ragged_vs_f64(mo, miF, O, E):
    """An f64 reference on the same inputs, through none of the kernels.

    R and dR are exact in f32 (_case, asserted here), so R16 = bf16(R) (du)
    and dR16 = bf16(dR) (dh, dw) are what the kernels round, and bt16 =
    bf16(bias term) is what the library GEMM returns. Each result is an f32
    sum of n exact or once-rounded products: every addition rounds by at most
    2^-24 of a partial sum that sum |a||b| bounds, so n * 2^-24 * sum|a||b|;
    2^-23 leaves a factor 2, as in the two test files the grids come from.
    n counts the true terms: the pads add exact zeros, which round nothing.
      out : miF products R u (R in f32, not rounded) + the bias term, n = miF + 1
      dH  : mo*miF products dR16 W
      dW  : E products dR16 H
      db  : E*O products g u, summed before any rounding
      dU  : mo products R16 g, stored in bf16: half an ulp, 2^-9 |dU|, on
            top; 2^-8 |ref| covers it measured on the reference."""
    c = _case(mo, miF, O, E)
    got, what = c['got'], f'mo={mo} miF={miF} O={O} E={E}'
    H, W, bias = c['H'].double(), c['W'].double(), c['bias'].double()
    u, g = c['u'].double(), c['g'].double()          # (miF,E,O), (E,mo,O)

    R0 = (H @ W.t()).view(E, mo, miF)                # without bias: fwd
    R = R0 + bias.view(1, mo, miF)
    assert torch.equal(R.float().double(), R), 'R must be exact in f32'
    dR = torch.einsum('emo,ceo->emc', g, u)
    assert torch.equal(dR.float().double(), dR), 'dR must be exact in f32'
    assert torch.equal(dR * 32, torch.round(dR * 32)) and dR.abs().max() <= 14
    bt = torch.einsum('mc,ceo->emo', bias.view(mo, miF), u)
    assert torch.equal(bt.float().double(), bt), 'bias term must be exact in f32'
    bt16 = bt.float().to(torch.bfloat16).double()
    R16 = R.float().to(torch.bfloat16).double()
    dR16 = dR.float().to(torch.bfloat16).double().reshape(E, mo * miF)

    eps = 2.0 ** -23
    _held('out', got['out'], bt16 + torch.einsum('emc,ceo->emo', R0, u),
          (miF + 1) * eps * (bt16.abs() + torch.einsum('emc,ceo->emo', R0.abs(), u.abs())),
          what)
    _held('dH', got['dH'], dR16 @ W, mo * miF * eps * (dR16.abs() @ W.abs()), what)
    _held('dW', got['dW'], dR16.t() @ H, E * eps * (dR16.abs().t() @ H.abs()), what)
    _held('db', got['db'], dR.sum(0).reshape(-1),
          E * O * eps * torch.einsum('emo,ceo->mc', g.abs(), u.abs()).reshape(-1), what)
    ref_du = torch.einsum('emc,emo->ceo', R16, g)
    assert got['dU'].dtype == torch.bfloat16
    assert not got['dU'][..., O:].any(), 'dU pad lanes must be exactly zero'
    _held('dU', got['dU'][..., :O], ref_du,
          2.0 ** -8 * ref_du.abs()
          + mo * eps * torch.einsum('emc,emo->ceo', R16.abs(), g.abs()), what)


# --------------------------------------------------------------------------
# 3. the packs
# --------------------------------------------------------------------------

@needs_gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('mo,miF', [(mo, miF) for mo in MOS for miF in MIFS])
def test_pack_w_both_on_ragged_dims(mo, miF, dtype):
    """P_fwd and P_dh of a ragged W are the packs of the zero-padded W, the
    pad rows written over whatever the buffers held."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    mo_p, miF_p = fused.pad_dims(mo, miF)
    gen = torch.Generator('cuda').manual_seed(100 * mo + miF)
    W = torch.randn(mo * miF, K, generator=gen, device='cuda').to(dtype)
    n = mo_p * miF_p * K
    guard = 32 * K
    bufs = [torch.full((n + 2 * guard,), SENTINEL, dtype=torch.bfloat16,
                       device='cuda') for _ in range(2)]
    Pf, Pdh = (b[guard:guard + n] for b in bufs)
    ext.pack_w_both(W, Pf, Pdh, mo)
    torch.cuda.synchronize()
    Wp = _pad_mc(W.to(torch.bfloat16), mo, miF, mo_p, miF_p)
    assert torch.equal(Pf, fused._pack_w_fwd(Wp, mo_p, miF_p).reshape(-1))
    assert torch.equal(Pdh, fused._pack_w_dh(Wp, mo_p, miF_p).reshape(-1))
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16, device='cuda')
    for b in bufs:
        assert (b[:guard] == sent).all() and (b[-guard:] == sent).all()


@needs_gpu
@pytest.mark.parametrize('O', OS)
@pytest.mark.parametrize('mo,E', [(1, 64), (7, 71), (9, 130), (17, 33),
                                  (24, 71), (33, 37), (39, 64)])
def test_pack_g_on_ragged_dims(mo, E, O):
    """G with ceil8(mo) rows: the true rows are pack_g's as ever, the pad
    rows exactly zero inside a sentinel-filled buffer. mo = 33, 39 reach a
    second 32-row tile."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    mo_p = fused.pad_dims(mo, 1)[0]
    gen = torch.Generator('cuda').manual_seed(10 * mo + O)
    grad = torch.randn(E, mo, O, generator=gen, device='cuda')
    guard = 64 * OP
    buf = torch.full((mo_p * E * OP + 2 * guard,), SENTINEL,
                     dtype=torch.bfloat16, device='cuda')
    G = buf[guard:guard + mo_p * E * OP].view(mo_p, E, OP)
    ext.pack_g(grad, G)
    torch.cuda.synchronize()
    ref = torch.zeros(mo_p, E, OP, dtype=torch.bfloat16, device='cuda')
    ref[:mo, :, :O] = grad.to(torch.bfloat16).permute(1, 0, 2)
    assert torch.equal(G, ref)
    assert not G[mo:].any()
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16, device='cuda')
    assert (buf[:guard] == sent).all() and (buf[-guard:] == sent).all()
    # the unpadded G of an unaligned mo is taken as before
    G2 = torch.full((mo, E, OP), SENTINEL, dtype=torch.bfloat16, device='cuda')
    ext.pack_g(grad, G2)
    assert torch.equal(G2, ref[:mo])


# --------------------------------------------------------------------------
# 4. ubuild
# --------------------------------------------------------------------------

UB_E = 37      # straddles the 32-edge forward tile and the 16-edge backward tile


@needs_gpu
@pytest.mark.parametrize('di,do', [(0, 0), (1, 1), (0, 3), (2, 1), (3, 3)])
@pytest.mark.parametrize('C', [1, 5, 8, 31, 33, 40, 48])
def test_ubuild_any_channel_count(C, di, do):
    """B is on the grid 1/8 in [-1, 1], x and dU on 1/4 in [-2, 2], all bf16
    values. U sums at most 7 products, multiples of 1/32 of size at most 2:
    below 16, 9 bits. dX sums at most 49 products B dU, multiples of 1/32 of
    size at most 2: below 98, 12 bits. dB sums at most 48 products x dU,
    multiples of 1/16 of size at most 4: below 192, 12 bits. Every partial
    sum is exact in f32 in any order (asserted), so U is bf16(f64), dX the
    f64 result rounded to its dtype and dB the f64 result."""
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    E = UB_E
    O, I, F_ = 2 * do + 1, 2 * di + 1, 2 * min(di, do) + 1
    OP = fused.opad(O)
    rows = C * F_
    rows_p = fused.pad_dims(1, rows)[1]
    gen = torch.Generator('cuda').manual_seed(1000 * C + 10 * di + do)
    B = _grid(gen, 1 / 8, 1.0, E, O, I, F_)
    x = _grid(gen, 1 / 4, 2.0, E, C, I)
    du = _grid(gen, 1 / 4, 2.0, rows, E, O)

    U64 = torch.einsum('eoif,eci->cfeo', B.double(), x.double()).reshape(rows, E, O)
    dX64 = torch.einsum('eoif,cfeo->eci', B.double(),
                        du.double().view(C, F_, E, O))
    dB64 = torch.einsum('eci,cfeo->eoif', x.double(),
                        du.double().view(C, F_, E, O))
    for t in (U64, dX64, dB64):
        assert torch.equal(t.float().double(), t)
    assert U64.abs().max() <= 14 and dX64.abs().max() <= 98 and dB64.abs().max() <= 192

    sent16 = torch.tensor(SENTINEL, dtype=torch.bfloat16, device='cuda')
    for xdt in (torch.float32, torch.bfloat16):
        xs = x.to(xdt)
        # forward into a padded U, and into one of the true rows alone
        guard = 64 * OP
        buf = torch.full((rows_p * E * OP + 2 * guard,), SENTINEL,
                         dtype=torch.bfloat16, device='cuda')
        U = buf[guard:guard + rows_p * E * OP].view(rows_p, E, OP)
        ext.ubuild_fwd(B, xs, U, O, I, F_)
        torch.cuda.synchronize()
        assert (buf[:guard] == sent16).all() and (buf[-guard:] == sent16).all()
        assert torch.equal(U[:rows, :, :O], U64.to(torch.bfloat16)), xdt
        assert not U[:rows, :, O:].any(), 'pad lanes'
        assert not U[rows:].any(), 'pad rows must be exactly zero'
        buf2 = torch.full((rows * E * OP + 2 * guard,), SENTINEL,
                          dtype=torch.bfloat16, device='cuda')
        U2 = buf2[guard:guard + rows * E * OP].view(rows, E, OP)
        ext.ubuild_fwd(B, xs, U2, O, I, F_)
        torch.cuda.synchronize()
        assert (buf2[:guard] == sent16).all() and (buf2[-guard:] == sent16).all()
        assert torch.equal(U2, U[:rows])

        for gdt in (torch.bfloat16, torch.float32):
            # padded dU: the pad rows hold a sentinel that must not be read
            dU = torch.full((rows_p, E, OP), SENTINEL, dtype=gdt, device='cuda')
            dU[:rows] = _pad_o(du, OP).to(gdt)
            for dUk in (dU, dU[:rows].contiguous()):
                bx = torch.full((E * C * I + 2 * 64,), SENTINEL, dtype=xdt,
                                device='cuda')
                dX = bx[64:64 + E * C * I].view(E, C, I)
                ext.ubuild_bwd_dx(B, dUk, dX, O, I, F_)
                bb = torch.full((E * O * I * F_ + 2 * 64,), SENTINEL,
                                device='cuda')
                dB = bb[64:64 + E * O * I * F_].view(E, O, I, F_)
                ext.ubuild_bwd_db(xs, dUk, dB, O, I, F_)
                torch.cuda.synchronize()
                for b in (bx, bb):
                    s = torch.tensor(SENTINEL, dtype=b.dtype, device='cuda')
                    assert (b[:64] == s).all() and (b[-64:] == s).all()
                assert torch.equal(dX, dX64.to(xdt)), (xdt, gdt)
                assert torch.equal(dB, dB64.float()), (xdt, gdt)


@needs_gpu
@pytest.mark.parametrize('C,di,do', [(5, 1, 1), (40, 2, 1)])
def test_ubuild_opad_returns_padded_rows_and_differentiates(C, di, do):
    """ubuild_opad hands fused_pairconv_opad a U with ceil32(C*F) rows, zero
    pads, and takes the padded dU back; ubuild() keeps the (C*F, O, E) view."""
    from se3_transformer_amd.ops import fused
    E = UB_E
    O, I, F_ = 2 * do + 1, 2 * di + 1, 2 * min(di, do) + 1
    gen = torch.Generator('cuda').manual_seed(C)
    B = _grid(gen, 1 / 8, 1.0, E, O, I, F_)
    x = _grid(gen, 1 / 4, 2.0, E, C, I).requires_grad_()
    U = fused.ubuild_opad(x, B, O, I, F_)
    rows_p = fused.pad_dims(1, C * F_)[1]
    assert U.shape == (rows_p, E, fused.opad(O)) and not U[C * F_:].any()
    dU = _grid(gen, 1 / 4, 2.0, rows_p, E, fused.opad(O)).to(torch.bfloat16)
    U.backward(dU)
    ref = torch.einsum('eoif,cfeo->eci', B.double(),
                       dU[:C * F_, :, :O].double().view(C, F_, E, O))
    assert torch.equal(x.grad, ref.float())
    assert fused.ubuild(x.detach(), B, O, I, F_).shape == (C * F_, O, E)


# --------------------------------------------------------------------------
# 5. switches on a ragged PairwiseConv
# --------------------------------------------------------------------------

def _ragged_pc(seed=3):
    from se3_transformer_amd.models.core import PairwiseConv
    torch.manual_seed(seed)
    di, do, mi, mo, E = 1, 2, 24, 5, 130
    pc = PairwiseConv(di, mi, do, mo, edge_dim=1).cuda()
    O, I, F_ = 2 * do + 1, 2 * di + 1, pc.num_freq
    ef = torch.randn(E, 2, device='cuda')
    b = torch.randn(E, O, I, F_, device='cuda')
    x0 = torch.randn(E, mi, I, device='cuda')
    return pc, ef, {(di, do): b}, x0


def _pc_grads(pc, ef, basis, x0, **sw):
    xg = x0.clone().requires_grad_()
    pc.zero_grad()
    with switches(**sw):
        out = pc.apply_fused(ef, basis, xg).float()
        out.pow(2).mean().backward()
    return {'out': out.detach(), 'x': xg.grad.clone(),
            'w6': pc.rp.net[6].weight.grad.clone(),
            'b6': pc.rp.net[6].bias.grad.clone(),
            'w0': pc.rp.net[0].weight.grad.clone()}


@needs_gpu
def test_ragged_hip_bwd_vs_torch_bwd():
    """As test_hip_bwd_vs_torch_bwd, at its 2e-2."""
    pc, ef, basis, x0 = _ragged_pc()
    hip = _pc_grads(pc, ef, basis, x0, SE3_FORCE_FUSED='1')
    tor = _pc_grads(pc, ef, basis, x0, SE3_FORCE_FUSED='1', SE3_TORCH_BWD='1')
    assert torch.equal(hip['out'], tor['out'])
    for k in ('x', 'w6', 'b6', 'w0'):
        err = _rel_err(hip[k].float(), tor[k].float())
        print(f'ragged hip vs torch bwd {k}: {err:.3e}')
        assert err < 2e-2, f'{k}: {err}'


@needs_gpu
def test_ragged_lowmem_pack_matches_default():
    """SE3_LOWMEM_PACK=1 pads in torch and re-packs in backward: bit-equal
    but for dH, whose split-K atomics leave order noise (1e-5) that the
    trunk gradient w0 and, through nothing else, inherits."""
    pc, ef, basis, x0 = _ragged_pc()
    ref = _pc_grads(pc, ef, basis, x0, SE3_FORCE_FUSED='1')
    low = _pc_grads(pc, ef, basis, x0, SE3_FORCE_FUSED='1', SE3_LOWMEM_PACK='1')
    for k in ('out', 'x', 'w6', 'b6'):
        assert torch.equal(low[k], ref[k]), f'{k} differs between pack modes'
    assert _rel_err(low['w0'], ref['w0']) < 1e-5


@needs_gpu
def test_ragged_kernel_path_vs_fp32_eager():
    """As test_pairconv_kernel_backward_parity: 5e-2 forward, 8e-2 grads."""
    pc, ef, basis, x0 = _ragged_pc()
    ref = _pc_grads(pc, ef, basis, x0)
    out = _pc_grads(pc, ef, basis, x0, SE3_FORCE_FUSED='1')
    errs = {k: _rel_err(out[k].float(), ref[k].float()) for k in ref}
    print('ragged kernel vs eager: '
          + ' '.join(f'{k}={v:.3e}' for k, v in errs.items()))
    assert errs['out'] < 5e-2
    for k in ('x', 'w6', 'b6', 'w0'):
        assert errs[k] < 8e-2, f'{k}: {errs[k]}'


@needs_gpu
@pytest.mark.parametrize('di,do', [(1, 1), (0, 2)])
def test_ragged_mo_from_nodes_equals_the_saved_u_path(di, do):
    """SE3_RECOMPUTE_U takes a pair with C % 32 == 0 whatever its mo (a
    dim_out = 3, 5 head on 32 channels): pairconv_from_nodes pads mo as
    fused_pairconv_opad does, on a U of the same bits, built again in the
    backward. Every edge has its own node, so the atomic sums of dXn have one
    term: all results are bit-equal but dH (1e-5: split-K atomics; here
    mo_p = 8 is one mo-block, so it is equal too)."""
    from se3_transformer_amd.ops import fused
    C, mo, E = 32, 5, 71
    O, I, F_ = 2 * do + 1, 2 * di + 1, 2 * min(di, do) + 1
    miF = C * F_
    assert fused.pad_dims(mo, miF) == (8, miF)
    gen = torch.Generator('cuda').manual_seed(40 + 10 * di + do)

    def r16(*shape):
        return torch.randn(*shape, generator=gen, device='cuda') \
            .to(torch.bfloat16).float()

    N = E + 3
    Xn0, B = r16(N, C, I), torch.randn(E, O, I, F_, generator=gen, device='cuda')
    rows = torch.randperm(N, generator=gen, device='cuda')[:E].to(torch.int32)
    H0, W0, b0 = r16(E, K), r16(mo * miF, K) / K ** 0.5, r16(mo * miF)
    gout = r16(E, mo, O)

    def run(nodes):
        Xn, H, W, bias = (t.clone().requires_grad_() for t in (Xn0, H0, W0, b0))
        if nodes:
            out = fused.pairconv_from_nodes(Xn, rows, B, H, W, bias, mo, O, I, F_)
        else:
            U = fused.ubuild_opad(Xn[rows.long()], B, O, I, F_)
            out = fused.fused_pairconv_opad(H, W, bias, U, mo, O)
        out.backward(gout)
        torch.cuda.synchronize()
        return dict(out=out.detach(), dXn=Xn.grad, dH=H.grad, dW=W.grad,
                    db=bias.grad)

    a, b = run(True), run(False)
    assert a['out'].shape == (E, mo, O) and a['dW'].shape == (mo * miF, K)
    for k in ('out', 'dXn', 'dW', 'db'):
        assert torch.equal(a[k], b[k]), k
    assert a['dXn'].abs().max() > 0
    assert _rel_err(a['dH'], b['dH']) < 1e-5


# --------------------------------------------------------------------------
# 6. models
# --------------------------------------------------------------------------

def _model_a():
    from se3_transformer_amd import SE3Transformer
    model = SE3Transformer(dim=16, heads=2, dim_head=8, depth=1,
                           num_degrees=2, num_neighbors=6).cuda()
    n = 24
    args = (torch.randn(1, n, 16, device='cuda'),
            torch.randn(1, n, 3, device='cuda'),
            torch.ones(1, n, dtype=torch.bool, device='cuda'))
    return model, args, dict(return_type=0)


def _model_b():
    """The fiber example of the reference README."""
    from se3_transformer_amd import SE3Transformer
    model = SE3Transformer(num_tokens=28, dim=64, num_edge_tokens=4,
                           edge_dim=16, depth=2, input_degrees=1,
                           num_degrees=3, output_degrees=1,
                           hidden_fiber_dict={0: 16, 1: 8, 2: 4},
                           out_fiber_dict={0: 16, 1: 1},
                           reduce_dim_out=False).cuda()
    n = 24
    args = (torch.randint(0, 28, (1, n), device='cuda'),
            torch.randn(1, n, 3, device='cuda'),
            torch.ones(1, n, dtype=torch.bool, device='cuda'))
    return model, args, dict(edges=torch.randint(0, 4, (1, n, n), device='cuda'))


def _flat(out):
    if isinstance(out, dict):
        return torch.cat([out[k].float().reshape(-1) for k in sorted(out)])
    return out.float().reshape(-1)


@needs_gpu
@pytest.mark.parametrize('make', [_model_a, _model_b], ids=['dim16', 'fiber'])
def test_ragged_model_runs_the_kernels_for_every_pair(make, monkeypatch):
    from se3_transformer_amd.models.core import ConvSE3
    from se3_transformer_amd.ops import fused
    torch.manual_seed(0)
    model, args, kw = make()
    ref = _flat(model(*args, **kw)).detach()

    ext = fused._load_ext()
    calls, pairs = [], []
    real = ext.pairconv_fwd_opad

    def spy(H, P, U, out, mo_p):
        calls.append((out.shape[1], U.shape[0]))
        return real(H, P, U, out, mo_p)

    monkeypatch.setattr(ext, 'pairconv_fwd_opad', spy)
    hooks = [m.register_forward_hook(
        lambda mod, a, o: pairs.extend(mod.kernel_unary.values()))
        for m in model.modules() if isinstance(m, ConvSE3)]
    assert hooks
    with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
        out = model(*args, **kw)
    for h in hooks:
        h.remove()
    # one kernel forward per degree pair of every ConvSE3 that ran
    assert len(calls) == len(pairs) > 0
    assert any(pc.nc_out % 8 or (pc.nc_in * pc.num_freq) % 32 for pc in pairs), \
        'no ragged pair in this model'
    # U reaches the kernel with ceil32(miF) rows, out with the true mo
    assert sorted(calls) == sorted(
        (pc.nc_out, -(-pc.nc_in * pc.num_freq // 32) * 32) for pc in pairs)
    err = _rel_err(_flat(out), ref)
    print(f'ragged model bf16 kernels vs fp32 eager: {err:.3e}')
    assert err < 0.1
    _flat(out).pow(2).mean().backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)

    # SE3_RECOMPUTE_U: the pairs with C % 32 != 0 keep the saved-U path
    model.zero_grad()
    n_default = len(calls)
    with switches(SE3_RECOMPUTE_U='1'), \
            torch.autocast(device_type='cuda', dtype=torch.bfloat16):
        out_r = model(*args, **kw)
        _flat(out_r).pow(2).mean().backward()
    torch.cuda.synchronize()
    assert len(calls) == 2 * n_default
    assert _rel_err(_flat(out_r), ref) < 0.1
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
