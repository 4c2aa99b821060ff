"""GPU tests of SE3_RECOMPUTE_U: the ubuild_gather_* kernels against their
gathered siblings, fused.pairconv_from_nodes against today's composition,
what a ConvSE3 saves, and the model with the switch on against off.

Kernel shapes: E = 77 is ragged against the 32-edge forward tile and the
16-edge backward tile, N = 19, C = 32 is one forward chunk and C = 64 makes
every chunk loop iterate. The dXn bound is the sum-order bound of fp32 fma
and add (derived in _dxn_bound), not a measured band.
"""
import pytest
import torch

from fused_helpers import no_switches, switches  # noqa: F401

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

E, N = 77, 19
SHAPES = [(1, 1, 1), (7, 1, 1), (3, 5, 3), (5, 5, 5), (7, 7, 7)]
DTYPES = [torch.float32, torch.bfloat16]
PLACEMENT = 1e-4     # between fp32 reordering (~1e-6) and a lost edge (~1e-2)


def _rows(pattern, gen):
    if pattern == 'random':
        r = torch.randint(0, N, (E,), generator=gen, device='cuda')
        r[3], r[E - 1] = 0, N - 1
    elif pattern == 'one_row':
        r = torch.full((E,), N - 1, device='cuda')
    else:
        r = torch.arange(E, device='cuda') % N
    return r.to(torch.int32)


PATTERNS = ('random', 'one_row', 'modulo')


def _inputs(O, I, F_, C, dtype, pattern, seed=0):
    gen = torch.Generator('cuda').manual_seed(1000 * O + 10 * I + F_ + C + seed)
    B = torch.randn(E, O, I, F_, generator=gen, device='cuda')
    Xn = torch.randn(N, C, I, generator=gen, device='cuda').to(dtype)
    return B, Xn, _rows(pattern, gen), gen


def _dxn_bound(B, dU, rows, n, O, I, F_):
    """f64 sum S[r,c,i] = sum_{e: rows[e]=r} sum_{f,o} B dU, and the bound on
    |dXn - S| of any fp32 evaluation: an edge's F*O-term fma chain is off by
    at most F*O * 2^-24 * sum|terms|, the m_r atomic adds of a row by at most
    m_r * 2^-24 * A; (F*O + m_r) 2^-24 <= m_r * F*O * 2^-23."""
    C = dU.shape[0] // F_
    g = dU[..., :O].reshape(C, F_, -1, O).double()
    b = B.double()
    per_edge = torch.einsum('eoif,cfeo->eci', b, g)
    per_edge_abs = torch.einsum('eoif,cfeo->eci', b.abs(), g.abs())
    idx = rows.long()
    S = torch.zeros(n, C, I, dtype=torch.float64, device='cuda')
    A = torch.zeros_like(S)
    S.index_add_(0, idx, per_edge)
    A.index_add_(0, idx, per_edge_abs)
    m = torch.bincount(idx, minlength=n).double().view(n, 1, 1)
    return S, A, m, m * F_ * O * 2.0 ** -23 * A


@needs_gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('O,I,F_', SHAPES)
def test_gather_fwd_is_ubuild_of_the_gathered_rows(O, I, F_, dtype):
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    for C in (32, 64):
        for pattern in PATTERNS:
            B, Xn, rows, _ = _inputs(O, I, F_, C, dtype, pattern)
            ref = fused.ubuild_opad(Xn[rows.long()], B, O, I, F_)
            U = torch.full((C * F_, E, OP), 7.0, dtype=torch.bfloat16,
                           device='cuda')
            ext.ubuild_gather_fwd(B, Xn, rows, U, O, I, F_)
            assert torch.equal(U, ref), (C, pattern)
            assert torch.equal(U[..., O:], torch.zeros_like(U[..., O:])), \
                'U pad lanes must be exactly zero'


@needs_gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('O,I,F_', SHAPES)
def test_gather_bwd_db_is_bwd_db_of_the_gathered_rows(O, I, F_, dtype):
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    for C in (32, 64):
        for pattern in PATTERNS:
            B, Xn, rows, gen = _inputs(O, I, F_, C, dtype, pattern, seed=1)
            # the pad lanes carry a cotangent too
            dU = torch.randn(C * F_, E, OP, generator=gen, device='cuda')
            ref = torch.full((E, O, I, F_), 7.0, device='cuda')
            ext.ubuild_bwd_db(Xn[rows.long()].contiguous(), dU, ref, O, I, F_)
            dB = torch.full((E, O, I, F_), -7.0, device='cuda')
            ext.ubuild_gather_bwd_db(Xn, rows, dU, dB, O, I, F_)
            assert torch.equal(dB, ref), (C, pattern)


@needs_gpu
@pytest.mark.parametrize('O,I,F_', SHAPES)
def test_gather_bwd_dx_within_the_sum_order_bound(O, I, F_):
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    OP = fused.opad(O)
    worst = 0.0
    for C in (32, 64):
        for pattern in PATTERNS:
            B, _, rows, gen = _inputs(O, I, F_, C, torch.float32, pattern, seed=2)
            dU = torch.randn(C * F_, E, OP, generator=gen, device='cuda')
            S, A, m, bound = _dxn_bound(B, dU, rows, N, O, I, F_)
            dXn = torch.zeros(N, C, I, device='cuda')
            ext.ubuild_gather_bwd_dx(B, dU, rows, dXn, O, I, F_)
            err = (dXn.double() - S).abs()
            worst = max(worst, (err / bound.clamp(min=1e-300)).max().item())
            assert (err <= bound).all(), (C, pattern, worst)
            untouched = (m.view(-1) == 0)
            assert torch.equal(dXn[untouched],
                               torch.zeros_like(dXn[untouched]))
            if pattern == 'one_row':
                assert untouched.sum() == N - 1 and m[N - 1].item() == E

            # accumulation: a nonzero dXn comes back as itself plus the sum
            # (one more add of |init| in the row's chain)
            init = torch.randn(N, C, I, generator=gen, device='cuda')
            acc = init.clone()
            ext.ubuild_gather_bwd_dx(B, dU, rows, acc, O, I, F_)
            bound1 = (m + 1) * F_ * O * 2.0 ** -23 * (A + init.abs().double())
            assert ((acc.double() - (init.double() + S)).abs() <= bound1).all()
            assert torch.equal(acc[untouched], init[untouched])
    print(f'gather_bwd_dx ({O},{I},{F_}): worst |err|/bound = {worst:.3f}')


def _rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


@needs_gpu
@pytest.mark.parametrize('switch', [None, 'SE3_TORCH_BWD', 'SE3_LOWMEM_PACK'])
@pytest.mark.parametrize('mo,oif,dtype,b_grad', [
    (8, (3, 5, 3), torch.float32, False),
    (16, (3, 5, 3), torch.bfloat16, True),
    (8, (7, 7, 7), torch.bfloat16, False),
    (16, (7, 7, 7), torch.float32, True)])
def test_pairconv_from_nodes_vs_composition(mo, oif, dtype, b_grad, switch):
    """pairconv_from_nodes against fused_pairconv_opad(ubuild_opad(Xn[rows]))
    under the same switch: out, dW, db (and dB) bit-equal; dH in the 1e-5
    band of its split-K atomics; dXn inside the bound built from the
    composition's own dU (plus the final cast for bf16 Xn)."""
    from se3_transformer_amd.ops import fused
    O, I, F_ = oif
    C = 32
    miF = C * F_
    B0, Xn0, rows, gen = _inputs(O, I, F_, C, dtype, 'random', seed=3 + mo)

    def r16(*shape):
        return torch.randn(*shape, generator=gen, device='cuda') \
            .to(torch.bfloat16).float()

    H0, W0, bias0 = r16(E, 128), r16(mo * miF, 128) / 128 ** 0.5, r16(mo * miF)
    gout = torch.randn(E, mo, O, generator=gen, device='cuda')

    def leaves():
        return (Xn0.clone().requires_grad_(), B0.clone().requires_grad_(b_grad),
                H0.clone().requires_grad_(), W0.clone().requires_grad_(),
                bias0.clone().requires_grad_())

    env = {switch: '1'} if switch else {}
    with switches(**env):
        Xn, B, H, W, bias = leaves()
        U = fused.ubuild_opad(Xn[rows.long()], B, O, I, F_)
        U.retain_grad()
        out_a = fused.fused_pairconv_opad(H, W, bias, U, mo, O)
        out_a.backward(gout)
        old = (Xn.grad, B.grad, H.grad, W.grad, bias.grad)
        dU = U.grad.float()

        Xn, B, H, W, bias = leaves()
        out_b = fused.pairconv_from_nodes(Xn, rows, B, H, W, bias, mo, O, I, F_)
        out_b.backward(gout)
        new = (Xn.grad, B.grad, H.grad, W.grad, bias.grad)

    assert out_b.shape == (E, mo, O) and torch.equal(out_a, out_b)
    assert torch.equal(new[3], old[3]), 'dW'
    assert torch.equal(new[4], old[4]), 'db'
    if b_grad:
        assert torch.equal(new[1], old[1]), 'dB'
    else:
        assert new[1] is None
    dh_err = _rel_err(new[2].float(), old[2].float())
    S, _, _, bound = _dxn_bound(B0, dU, rows, N, O, I, F_)
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * S.abs()
    assert new[0].dtype == dtype and new[0].shape == Xn0.shape
    err = (new[0].double() - S).abs()
    print(f'from_nodes mo={mo} {oif} {switch}: dH rel_err={dh_err:.3e} '
          f'dXn worst |err|/bound='
          f'{(err / bound.clamp(min=1e-300)).max().item():.3f} '
          f'dXn vs old={_rel_err(new[0].float(), old[0].float()):.3e}')
    assert dh_err < 1e-5
    assert (err <= bound).all()


def _conv_case(pool, self_interaction, n=16, k=4):
    from se3_transformer_amd.models.core import ConvSE3
    from se3_transformer_amd.models.fiber import Fiber
    from se3_transformer_amd.ops.basis import get_basis_packed
    from se3_transformer_amd.utils import batched_index_select
    torch.manual_seed(5)
    fiber = Fiber([(0, 32), (1, 32)])
    conv = ConvSE3(fiber, fiber, pool=pool,
                   self_interaction=self_interaction).to('cuda')
    feats = {'0': torch.randn(1, n, 32, 1, device='cuda'),
             '1': torch.randn(1, n, 32, 3, device='cuda')}
    coors = torch.randn(1, n, 3, device='cuda')
    idx = torch.cdist(coors, coors).topk(k + 1, largest=False).indices[..., 1:]
    rel_pos = coors.unsqueeze(2) - batched_index_select(coors, idx, dim=1)
    basis = get_basis_packed(rel_pos, 1)
    mask = torch.ones(1, n, k, dtype=torch.bool, device='cuda')

    def forward():
        leaves = {d: t.clone().requires_grad_() for d, t in feats.items()}
        with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
            out = conv(leaves, (idx, mask, None),
                       rel_dist=rel_pos.norm(dim=-1), basis=basis)
        return leaves, out

    return conv, forward


@needs_gpu
def test_what_a_convse3_saves():
    from se3_transformer_amd.ops import fused
    n, k, mi = 16, 4, 32
    Ecv = n * k
    conv, forward = _conv_case(pool=False, self_interaction=False, n=n, k=k)
    # pairs (di, do): U (mi*F, E, OP(2do+1)) bf16
    u_shapes = {(mi * (2 * min(di, do) + 1), Ecv, fused.opad(2 * do + 1))
                for di in (0, 1) for do in (0, 1)}
    u_bytes = sum(mi * (2 * min(di, do) + 1) * Ecv * fused.opad(2 * do + 1) * 2
                  for di in (0, 1) for do in (0, 1))
    node_bytes = sum(n * mi * (2 * di + 1) * 4 for di in (0, 1))   # fp32 feats
    gathered = {(Ecv, mi, I) for I in (1, 3)} | {(1, n, k, mi, I) for I in (1, 3)}

    def saved():
        seen = {}

        def pack(t):
            seen[(t.data_ptr(), tuple(t.shape))] = t.numel() * t.element_size()
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            forward()
        return {s for _, s in seen}, sum(seen.values())

    off_shapes, off_bytes = saved()
    with switches(SE3_RECOMPUTE_U='1'):
        on_shapes, on_bytes = saved()
    assert u_shapes <= off_shapes, 'the hook must see U where it is saved'
    assert not (u_shapes & on_shapes), u_shapes & on_shapes
    assert not (gathered & on_shapes), gathered & on_shapes
    print(f'ConvSE3 saved bytes: off {off_bytes} on {on_bytes} '
          f'(U set {u_bytes}, node features {node_bytes})')
    assert off_bytes - on_bytes >= u_bytes - node_bytes


@needs_gpu
@pytest.mark.parametrize('pool,self_interaction', [(False, False), (True, True)])
def test_convse3_switch_on_against_off(pool, self_interaction):
    conv, forward = _conv_case(pool, self_interaction)

    def run():
        conv.zero_grad(set_to_none=True)
        leaves, out = forward()
        cot = [torch.ones_like(o) / o.numel() ** 0.5 for o in out.values()]
        torch.autograd.backward([o for o in out.values()], cot)
        grads = {name: p.grad.clone() for name, p in conv.named_parameters()}
        grads.update({f'feats.{d}': t.grad for d, t in leaves.items()})
        return [o.detach() for o in out.values()], grads

    out_off, g_off = run()
    with switches(SE3_RECOMPUTE_U='1'):
        out_on, g_on = run()
    for a, b in zip(out_on, out_off):
        assert torch.equal(a, b)
    worst = 0.0
    for name, g in g_off.items():
        if 'rp.net.6' in name:
            assert torch.equal(g_on[name], g), name
        else:
            worst = max(worst, _rel_err(g_on[name].float(), g.float()))
    print(f'ConvSE3 pool={pool}: worst max-normalised gradient difference '
          f'on vs off = {worst:.3e}')
    assert worst < PLACEMENT


@needs_gpu
def test_convse3_stream_pool_with_the_switch_on():
    """SE3_STREAMS fans the pairs out over the stream pool; the pairs that
    read node features and rows made on the calling stream give the bits of
    the single-stream run, and the gradients of the switch-off pool run."""
    conv, forward = _conv_case(pool=True, self_interaction=True)

    def run():
        conv.zero_grad(set_to_none=True)
        leaves, out = forward()
        cot = [torch.ones_like(o) / o.numel() ** 0.5 for o in out.values()]
        torch.autograd.backward([o for o in out.values()], cot)
        torch.cuda.synchronize()
        grads = {name: p.grad.clone() for name, p in conv.named_parameters()}
        grads.update({f'feats.{d}': t.grad for d, t in leaves.items()})
        return [o.detach() for o in out.values()], grads

    with switches(SE3_RECOMPUTE_U='1'):
        out_one, _ = run()
    with switches(SE3_STREAMS='1'):
        out_off, g_off = run()
    with switches(SE3_STREAMS='1', SE3_RECOMPUTE_U='1'):
        out_on, g_on = run()
    for a, b, c in zip(out_on, out_off, out_one):
        assert torch.equal(a, b) and torch.equal(a, c)
    worst = max(_rel_err(g_on[name].float(), g.float())
                for name, g in g_off.items())
    print(f'ConvSE3 on the stream pool: worst max-normalised gradient '
          f'difference on vs off = {worst:.3e}')
    assert worst < PLACEMENT


def _model(**kw):
    from se3_transformer_amd import SE3Transformer
    torch.manual_seed(7)
    return SE3Transformer(dim=32, heads=2, dim_head=16, depth=1, num_degrees=2,
                          num_neighbors=4, **kw).to('cuda')


def _model_inputs(n=16):
    # seed: see test_hipgraph_step_with_the_switch_on
    gen = torch.Generator('cuda').manual_seed(18)
    return (torch.randn(1, n, 32, generator=gen, device='cuda'),
            torch.randn(1, n, 3, generator=gen, device='cuda'),
            torch.ones(1, n, dtype=torch.bool, device='cuda'))


@needs_gpu
@pytest.mark.parametrize('kw', [{}, {'reversible': True},
                                {'differentiable_coors': True}],
                         ids=['plain', 'reversible', 'diffcoors'])
def test_model_switch_on_against_off(kw):
    model = _model(**kw)
    feats, coors0, mask = _model_inputs()

    def run():
        model.zero_grad(set_to_none=True)
        coors = coors0.clone().requires_grad_('differentiable_coors' in kw)
        with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
            out = model(feats, coors, mask, return_type=0)
        out.float().pow(2).mean().backward()
        return out.detach(), coors.grad, \
            {n_: p.grad.clone() for n_, p in model.named_parameters()
             if p.grad is not None}

    out_off, dc_off, g_off = run()
    with switches(SE3_RECOMPUTE_U='1'):
        out_on, dc_on, g_on = run()
    assert torch.equal(out_on, out_off)
    assert g_on.keys() == g_off.keys()
    assert all(torch.isfinite(g).all() for g in g_on.values())
    if 'differentiable_coors' in kw:
        err = _rel_err(dc_on, dc_off)
        print(f'model diffcoors: coordinate gradient on vs off = {err:.3e}')
        assert err < PLACEMENT


@needs_gpu
def test_hipgraph_step_with_the_switch_on():
    """One forward+backward step captured with the switch on: two replays
    give the eager step's loss and its gradients within PLACEMENT (the
    zero-init of dXn sits inside the captured region, or the second replay
    would double them). The reference is one eager step.

    Why _model_inputs uses seed 18: the model's eager step does not always
    repeat itself, switch off or on. pairconv_bwd_dh sums dH over 4 split-K
    slices with atomics (mo = 32), so an element varies by an fp32 ulp from
    run to run, and dH is then rounded to bf16 for the radial-trunk
    backward. With input seed 8 element (40, 106) of to_k.(0,1)'s dH was
    3.3900139e-06 in some runs and 3.3900142e-06 in others, on either side
    of a bf16 rounding boundary, and exactly those runs moved
    to_k.(0,1).rp.net.3.weight's gradient by 1.084e-4; no other tensor
    differed. That is a property of the inputs, not of the switch or of the
    capture. Seed 18 showed no such element in 12 eager steps (every
    gradient within 2.7e-7); seeds 11 and 17 likewise, seeds 8-10, 12 and
    14-16 did not (profiles/recompute_u.md)."""
    model = _model()
    feats, coors, mask = _model_inputs()
    params = [p for p in model.parameters()]
    loss_buf = torch.zeros((), device='cuda')

    def step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
            out = model(feats, coors, mask, return_type=0)
            loss = out.float().pow(2).mean()
        loss.backward()
        loss_buf.copy_(loss.detach())

    with switches(SE3_RECOMPUTE_U='1'):
        for _ in range(2):        # allocator warmup; also the eager step
            step()
        torch.cuda.synchronize()
        eager_loss = loss_buf.clone()
        eager = [None if p.grad is None else p.grad.clone() for p in params]
        live = [i for i, e in enumerate(eager)
                if e is not None and e.abs().max() > 0]
        assert live
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for replay in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss_buf, eager_loss)
            worst = max(_rel_err(params[i].grad.float(), eager[i].float())
                        for i in live)
            print(f'hipGraph replay {replay}: worst gradient difference '
                  f'vs the eager step = {worst:.3e}')
            assert worst < PLACEMENT
