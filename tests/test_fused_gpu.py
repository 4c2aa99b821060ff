"""GPU parity tests: fused HIP pairconv kernel vs the eager chunked path.

The kernel computes in bf16 with fp32 accumulation; parity is checked
against an fp32 eager reference with bf16-grade tolerance bands.
"""
import pytest
import torch

from fused_helpers import switches

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')


def _rel_err(a, b):
    denom = b.abs().max().clamp(min=1e-6)
    return ((a - b).abs().max() / denom).item()


@needs_gpu
def test_ext_loaded():
    from se3_transformer_amd.ops import fused
    assert fused.ext_available(), 'HIP extension must be built in-tree'


@needs_gpu
@pytest.mark.parametrize('di,do', [(0, 0), (1, 2), (3, 3), (2, 1)])
def test_pairconv_kernel_vs_eager(di, do):
    from se3_transformer_amd.models.core import PairwiseConv
    from se3_transformer_amd.ops.basis import get_basis

    torch.manual_seed(0)
    device = torch.device('cuda')
    E, mi, mo = 1000, 64, 32
    pc = PairwiseConv(di, mi, do, mo, edge_dim=2).to(device)
    F_ = pc.num_freq
    O = 2 * do + 1
    I = 2 * di + 1

    ef = torch.randn(E, 3, device=device)
    b = torch.randn(E, O, I, F_, device=device)
    xg = torch.randn(E, mi, I, device=device)

    ref = pc.apply_fused(ef, {(di, do): b}, xg).float()

    with switches(SE3_FORCE_FUSED='1'):
        out = pc.apply_fused(ef, {(di, do): b}, xg.clone()).float()
    err = _rel_err(out, ref)
    assert err < 5e-2, f'forward parity {err}'


@needs_gpu
def test_pairconv_kernel_backward_parity():
    from se3_transformer_amd.models.core import PairwiseConv

    torch.manual_seed(1)
    device = torch.device('cuda')
    di, do = 1, 1
    E, mi, mo = 512, 32, 32
    pc = PairwiseConv(di, mi, do, mo, edge_dim=0).to(device)
    F_, O, I = pc.num_freq, 2 * do + 1, 2 * di + 1

    ef = torch.randn(E, 1, device=device)
    b = torch.randn(E, O, I, F_, device=device)
    xg0 = torch.randn(E, mi, I, device=device, requires_grad=True)
    xg1 = xg0.detach().clone().requires_grad_(True)

    ref = pc.apply_fused(ef, {(di, do): b}, xg0).float()
    ref.pow(2).mean().backward()
    gw_ref = pc.rp.net[6].weight.grad.clone()
    gb_ref = pc.rp.net[6].bias.grad.clone()
    g0_ref = pc.rp.net[0].weight.grad.clone()
    gx_ref = xg0.grad.clone()
    pc.zero_grad()

    with switches(SE3_FORCE_FUSED='1'):
        out = pc.apply_fused(ef, {(di, do): b}, xg1).float()
        out.pow(2).mean().backward()
    gw = pc.rp.net[6].weight.grad.clone()
    gb = pc.rp.net[6].bias.grad.clone()
    g0 = pc.rp.net[0].weight.grad.clone()
    gx = xg1.grad.clone()

    assert _rel_err(out, ref) < 5e-2
    assert _rel_err(gx, gx_ref) < 8e-2, 'du path'
    assert _rel_err(gw.float(), gw_ref.float()) < 8e-2, 'dW path'
    assert _rel_err(gb.float(), gb_ref.float()) < 8e-2, 'db path'
    assert _rel_err(g0.float(), g0_ref.float()) < 8e-2, 'dH path (trunk)'


@needs_gpu
@pytest.mark.parametrize('di,do', [(0, 0), (3, 3)])
def test_hip_bwd_vs_torch_bwd(di, do):
    """The three HIP backward kernels vs the torch chunked backward of the
    same fused Function (identical bf16 forward, so tight tolerance)."""
    from se3_transformer_amd.models.core import PairwiseConv

    torch.manual_seed(2)
    device = torch.device('cuda')
    E, mi, mo = 777, 64, 32
    pc = PairwiseConv(di, mi, do, mo, edge_dim=1).to(device)
    F_, O, I = pc.num_freq, 2 * do + 1, 2 * di + 1
    ef = torch.randn(E, 2, device=device)
    b = torch.randn(E, O, I, F_, device=device)

    grads = {}
    for mode in ('hip', 'torch'):
        xg = torch.randn(E, mi, I, device=device,
                         generator=torch.Generator(device).manual_seed(7),
                         requires_grad=True)
        pc.zero_grad()
        with switches(SE3_FORCE_FUSED='1',
                      SE3_TORCH_BWD='1' if mode == 'torch' else None):
            out = pc.apply_fused(ef, {(di, do): b}, xg).float()
            out.pow(2).mean().backward()
        grads[mode] = {
            'x': xg.grad.clone(),
            'w6': pc.rp.net[6].weight.grad.clone(),
            'b6': pc.rp.net[6].bias.grad.clone(),
            'w0': pc.rp.net[0].weight.grad.clone(),
        }
    for k in grads['hip']:
        err = _rel_err(grads['hip'][k].float(), grads['torch'][k].float())
        assert err < 2e-2, f'{k}: {err}'


@needs_gpu
def test_model_fused_bf16_close_to_eager_fp32():
    """Full model: autocast-bf16 fused path vs fp32 eager, loose band."""
    from se3_transformer_amd import SE3Transformer
    device = torch.device('cuda')
    torch.manual_seed(0)
    model = SE3Transformer(dim=64, heads=4, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=8).to(device)
    feats = torch.randn(1, 64, 64, device=device)
    coors = torch.randn(1, 64, 3, device=device)
    mask = torch.ones(1, 64, dtype=torch.bool, device=device)
    ref = model(feats, coors, mask, return_type=0)
    with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
        out = model(feats, coors, mask, return_type=0)
    err = _rel_err(out.float(), ref.float())
    assert err < 0.1, f'bf16 fused vs fp32 eager: {err}'


@needs_gpu
@pytest.mark.parametrize('max_degree', [1, 2, 3])
def test_sh_basis_kernel_vs_eager(max_degree):
    from se3_transformer_amd.ops.basis import get_basis_packed
    torch.manual_seed(3)
    rel = torch.randn(2, 100, 8, 3, device='cuda')
    with switches(SE3_EAGER_BASIS='1'):
        ref = get_basis_packed(rel, max_degree)
    fast = get_basis_packed(rel, max_degree)
    assert set(ref) == set(fast)
    for k in ref:
        err = (ref[k] - fast[k]).abs().max().item()
        assert err < 1e-4, f'{k}: {err}'


@needs_gpu
@pytest.mark.parametrize('m', [1, 3, 7])
def test_norm_se3_kernel_vs_eager(m):
    from se3_transformer_amd.models.core import NormSE3
    from se3_transformer_amd.models.fiber import Fiber
    torch.manual_seed(4)
    degree = (m - 1) // 2
    norm = NormSE3(Fiber([(degree, 24)])).to('cuda')
    t0 = torch.randn(3, 50, 24, m, device='cuda', requires_grad=True)
    t1 = t0.detach().clone().requires_grad_(True)

    with switches(SE3_EAGER_NORM='1'):
        ref = norm({str(degree): t0})[str(degree)]
    ref.pow(2).mean().backward()
    out = norm({str(degree): t1})[str(degree)]
    assert _rel_err(out, ref) < 1e-5
    gs_ref = norm.transform[str(degree)]['scale'].grad.clone()
    norm.zero_grad()
    out.pow(2).mean().backward()
    gs = norm.transform[str(degree)]['scale'].grad
    assert _rel_err(t1.grad, t0.grad) < 1e-4
    assert _rel_err(gs, gs_ref) < 1e-4


@needs_gpu
def test_fused_attention_vs_eager():
    from se3_transformer_amd.models.attention import AttentionSE3
    from se3_transformer_amd.models.fiber import Fiber
    torch.manual_seed(5)
    fiber = Fiber([(0, 32), (1, 32)])
    attn = AttentionSE3(fiber, dim_head=16, heads=2, attend_self=True,
                        use_null_kv=True).to('cuda')
    b, n, kn = 2, 40, 6
    feats = {'0': torch.randn(b, n, 32, 1, device='cuda', requires_grad=True),
             '1': torch.randn(b, n, 32, 3, device='cuda', requires_grad=True)}
    feats2 = {k: v.detach().clone().requires_grad_(True) for k, v in feats.items()}
    nbr_idx = torch.randint(0, n, (b, n, kn), device='cuda')
    nbr_mask = torch.rand(b, n, kn, device='cuda') > 0.2
    rel_dist = torch.rand(b, n, kn, device='cuda')
    from se3_transformer_amd.ops.basis import get_basis_packed
    rel_pos = torch.randn(b, n, kn, 3, device='cuda')
    basis = get_basis_packed(rel_pos, 1)
    edge_info = (nbr_idx, nbr_mask, None)

    with switches(SE3_EAGER_ATTN='1'):
        ref = attn(feats, edge_info, rel_dist, basis)
    (ref['0'].pow(2).mean() + ref['1'].pow(2).mean()).backward()
    gref = {k: v.grad.clone() for k, v in feats.items()}

    out = attn(feats2, edge_info, rel_dist, basis)
    for d in ref:
        assert _rel_err(out[d], ref[d]) < 1e-4, d
    (out['0'].pow(2).mean() + out['1'].pow(2).mean()).backward()
    for d in gref:
        assert _rel_err(feats2[d].grad, gref[d]) < 1e-3, d


@needs_gpu
def test_knn_kernel_vs_eager():
    from se3_transformer_amd import SE3Transformer
    torch.manual_seed(6)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=6,
                           valid_radius=2.5).to('cuda')
    feats = torch.randn(2, 50, 32, device='cuda')
    coors = torch.randn(2, 50, 3, device='cuda') * 1.3
    mask = torch.rand(2, 50, device='cuda') > 0.1
    with switches(SE3_EAGER_KNN='1'):
        ref = model(feats, coors, mask, return_type=0)
    out = model(feats, coors, mask, return_type=0)
    err = (out - ref).abs().max().item()
    assert err < 1e-4, f'knn path mismatch: {err}'


@needs_gpu
def test_fused_attention_one_headed_vs_eager():
    from se3_transformer_amd.models.attention import OneHeadedKVAttentionSE3
    from se3_transformer_amd.models.fiber import Fiber
    from se3_transformer_amd.ops.basis import get_basis_packed
    torch.manual_seed(7)
    fiber = Fiber([(0, 32), (1, 32)])
    attn = OneHeadedKVAttentionSE3(fiber, dim_head=16, heads=2,
                                   attend_self=True).to('cuda')
    b, n, kn = 2, 36, 5
    feats = {'0': torch.randn(b, n, 32, 1, device='cuda', requires_grad=True),
             '1': torch.randn(b, n, 32, 3, device='cuda', requires_grad=True)}
    feats2 = {k: v.detach().clone().requires_grad_(True) for k, v in feats.items()}
    edge_info = (torch.randint(0, n, (b, n, kn), device='cuda'),
                 torch.rand(b, n, kn, device='cuda') > 0.2, None)
    rel_dist = torch.rand(b, n, kn, device='cuda')
    basis = get_basis_packed(torch.randn(b, n, kn, 3, device='cuda'), 1)

    with switches(SE3_EAGER_ATTN='1'):
        ref = attn(feats, edge_info, rel_dist, basis)
    (ref['0'].pow(2).mean() + ref['1'].pow(2).mean()).backward()
    gref = {k: v.grad.clone() for k, v in feats.items()}

    out = attn(feats2, edge_info, rel_dist, basis)
    for d in ref:
        assert _rel_err(out[d], ref[d]) < 1e-4, d
    (out['0'].pow(2).mean() + out['1'].pow(2).mean()).backward()
    for d in gref:
        assert _rel_err(feats2[d].grad, gref[d]) < 1e-3, d


@needs_gpu
def test_knn_kernel_causal_vs_eager():
    from se3_transformer_amd import SE3Transformer
    torch.manual_seed(8)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=5, causal=True,
                           attend_self=True, valid_radius=3.).to('cuda')
    feats = torch.randn(1, 40, 32, device='cuda')
    coors = torch.randn(1, 40, 3, device='cuda')
    mask = torch.ones(1, 40, dtype=torch.bool, device='cuda')
    with switches(SE3_EAGER_KNN='1'):
        ref = model(feats, coors, mask, return_type=0)
    out = model(feats, coors, mask, return_type=0)
    err = (out - ref).abs().max().item()
    assert err < 1e-4, f'causal knn mismatch: {err}'


@needs_gpu
def test_pack_w_both_matches_python_permutes():
    """csrc/pack_w.hip: the one-pass pack kernel must reproduce the python
    permute layouts exactly (including the fp32 -> bf16 rounding)."""
    from se3_transformer_amd import _C
    from se3_transformer_amd.ops.fused import _pack_w_dh, _pack_w_fwd

    torch.manual_seed(3)
    device = torch.device('cuda')
    mo, miF = 16, 96
    for dtype in (torch.float32, torch.bfloat16):
        W = torch.randn(mo * miF, 128, device=device, dtype=dtype)
        Pf = torch.empty(mo * miF * 128, dtype=torch.bfloat16, device=device)
        Pdh = torch.empty_like(Pf)
        _C.pack_w_both(W, Pf, Pdh, mo)
        W16 = W.to(torch.bfloat16)
        ref_f = _pack_w_fwd(W16, mo, miF)
        ref_d = _pack_w_dh(W16, mo, miF)
        assert torch.equal(Pf.view_as(ref_f), ref_f), f'fwd pack {dtype}'
        assert torch.equal(Pdh.view_as(ref_d), ref_d), f'dh pack {dtype}'


def _fwd_mo16(O, mb2):
    """pairconv_fwd_opad at mo=16, miF=160, E=500 on fixed inputs: mb2=2 is one
    launch (two mo-blocks per workgroup, picked when mo % 16 == 0); mb2=1
    is two mo=8 launches (the one-block kernel) over the contiguous halves
    of the packed W, whose leading index is the mo-block, written into the
    matching halves of the output."""
    from se3_transformer_amd import _C
    from se3_transformer_amd.ops.fused import _pack_w_fwd, _to_opad

    device = torch.device('cuda')
    g = torch.Generator(device).manual_seed(4)
    mo, miF, E = 16, 160, 500
    H = torch.randn(E, 128, generator=g, device=device).to(torch.bfloat16)
    W = torch.randn(mo * miF, 128, generator=g, device=device).to(torch.bfloat16)
    Ut = torch.randn(miF, O, E, generator=g, device=device).to(torch.bfloat16)
    P = _pack_w_fwd(W, mo, miF).reshape(2, -1)
    U = _to_opad(Ut, O)

    out = torch.zeros(E, mo, O, device=device)
    if mb2 == 2:
        _C.pairconv_fwd_opad(H, P, U, out, mo)
        return out
    for half in range(2):
        out_h = torch.zeros(E, mo // 2, O, device=device)
        _C.pairconv_fwd_opad(H, P[half], U, out_h, mo // 2)
        out[:, half * 8:(half + 1) * 8] = out_h
    return out


@needs_gpu
@pytest.mark.parametrize('O', [1, 3, 5, 7])
def test_pairconv_fwd_mb2_variants_agree(O):
    """The two-mo-blocks-per-workgroup forward and the one-block forward
    must be numerically identical, at every output order."""
    assert torch.equal(_fwd_mo16(O, 2), _fwd_mo16(O, 1)), \
        f'O={O}: the MB2=2 and MB2=1 kernels differ'


@needs_gpu
@pytest.mark.parametrize('mb2', [pytest.param(1, id='0-1-0'),
                                 pytest.param(2, id='0-2-0')])
def test_pairconv_fwd_uu_variants_agree(mb2):
    """Forward variants against the one-block (MB2=1) forward at O=5, bit
    for bit. The ids are the (UU, MB2, WP) triples of the cases that remain
    from when the variants were picked by environment knobs: MB2 is the only
    axis left, and it now follows from mo."""
    assert torch.equal(_fwd_mo16(5, mb2), _fwd_mo16(5, 1)), \
        f'MB2={mb2} diverges from the MB2=1 forward'


def _pairconv_oracle_case(O, mo, miF, E):
    """fused_pairconv vs fp32 autograd of its docstring formula on the
    bf16-rounded inputs; returns the max-normalised error of each result."""
    from se3_transformer_amd.ops.fused import fused_pairconv

    device = torch.device('cuda')
    g = torch.Generator(device).manual_seed(1000 * O + mo)

    def rnd(*shape):
        x = torch.randn(*shape, generator=g, device=device)
        return x.to(torch.bfloat16).float()

    vals = [rnd(E, 128), rnd(mo * miF, 128), rnd(mo * miF), rnd(miF, O, E)]
    gout = rnd(E, mo, O)

    def leaves():
        return [v.clone().requires_grad_(True) for v in vals]

    H, W, bias, Ut = leaves()
    R = (H @ W.t() + bias).view(E, mo, miF)
    ref = torch.einsum('emc,coe->emo', R, Ut)
    ref_grads = torch.autograd.grad(ref, (H, W, bias, Ut), gout)

    H, W, bias, Ut = leaves()
    out = fused_pairconv(H, W, bias, Ut, mo)
    grads = torch.autograd.grad(out, (H, W, bias, Ut), gout)

    errs = {'out': _rel_err(out.detach(), ref.detach())}
    for name, a, b in zip(('dH', 'dW', 'db', 'dUt'), grads, ref_grads):
        errs[name] = _rel_err(a.float(), b)
    return errs


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E',
                         [(O, mo, 64, 77) for O in (1, 3, 5, 7)
                          for mo in (8, 16)] + [(3, 128, 256, 77)])
def test_pairconv_kernels_small_shapes_vs_oracle(O, mo, miF, E):
    """Every pairconv instantiation that ships, at the smallest shapes that
    reach each of its paths, against fp32 autograd of the Function's formula.

    E=77 is a full 64-edge block plus a 13-edge one: a whole 8-edge vector,
    a ragged run of 5, and rows that are not 16-byte aligned. miF=64 makes
    the chunk loops and the register staging iterate; mo=8 is one mo-block
    per workgroup (dh unsplit), mo=16 two. (3, 128, 256) is the one case
    that takes the XCD-cohort block mapping (fwd and du) and dh's 16-way
    split-K.

    Bands: 4x the worst max-normalised error over the nine cases, measured
    on the build before the kernels were pruned, rounded up to one figure
    (the errors are bf16 rounding of dR/R/db inside the kernels):
        out 1.88e-4 -> 8e-4    dH 1.93e-3 -> 8e-3    dW 2.15e-3 -> 9e-3
        db  2.64e-3 -> 2e-2    dUt 2.40e-3 -> 1e-2
    """
    errs = _pairconv_oracle_case(O, mo, miF, E)
    print(f'pairconv oracle O={O} mo={mo} miF={miF} E={E}: '
          + ' '.join(f'{k}={v:.3e}' for k, v in errs.items()))
    bands = {'out': 8e-4, 'dH': 8e-3, 'dW': 9e-3, 'db': 2e-2, 'dUt': 1e-2}
    for name, band in bands.items():
        assert errs[name] < band, (name, errs)


@needs_gpu
@pytest.mark.parametrize('edge_in', [1, 9])
def test_radial_trunk_kernel_vs_eager(edge_in):
    """csrc/radial.hip forward + backward vs the eager fp32 trunk
    (reference se3_transformer_pytorch.py:287-295 layer layout)."""
    from se3_transformer_amd.models.core import RadialFunc
    from se3_transformer_amd.ops import fused as _fused

    if not _fused.radial_trunk_ok(edge_in, 128):
        pytest.skip('radial trunk kernel unavailable')
    torch.manual_seed(6)
    device = torch.device('cuda')
    rp = RadialFunc(3, 8, 8, edge_dim=edge_in - 1).to(device)
    E = 1000
    x0 = torch.randn(E, edge_in, device=device, requires_grad=True)
    x1 = x0.detach().clone().requires_grad_(True)

    with switches(SE3_EAGER_RADIAL='1'):
        ref = rp.hidden(x0)
    ref.pow(2).mean().backward()
    ref_grads = {n: p.grad.clone() for n, p in rp.named_parameters()
                 if p.grad is not None}
    ref_gx = x0.grad.clone()
    rp.zero_grad()

    out = rp.hidden(x1)
    assert out.dtype == torch.bfloat16
    out.float().pow(2).mean().backward()

    assert _rel_err(out.float(), ref) < 2e-2, 'trunk forward'
    assert _rel_err(x1.grad, ref_gx) < 5e-2, 'dX'
    for n, p in rp.named_parameters():
        if n.startswith('net.6') or n not in ref_grads:
            continue
        err = _rel_err(p.grad.float(), ref_grads[n].float())
        assert err < 5e-2, f'{n}: {err}'


@needs_gpu
@pytest.mark.parametrize('kn', [6, 70])   # 70 neighbors => J > 64 tiles
def test_attn2_module_vs_eager_with_backward(kn):
    """attn2 kernel (online-softmax tiles, HIP backward) vs the eager einsum
    path through AttentionSE3, forward and gradients."""
    from se3_transformer_amd.models.attention import AttentionSE3
    from se3_transformer_amd.models.fiber import Fiber

    torch.manual_seed(8)
    n = 96
    fiber = Fiber([(0, 16), (1, 16)])
    attn = AttentionSE3(fiber, dim_head=8, heads=2, attend_self=True,
                        use_null_kv=True).to('cuda')
    b = 2
    nbr_idx = torch.randint(0, n, (b, n, kn), device='cuda')
    nbr_mask = torch.rand(b, n, kn, device='cuda') > 0.1
    rel_dist = torch.rand(b, n, kn, device='cuda') * 3
    basis = {}
    for di in (0, 1):
        for do in (0, 1):
            F_ = 2 * min(di, do) + 1
            basis[(di, do)] = torch.randn(b, n, kn, 2 * do + 1, 2 * di + 1,
                                          F_, device='cuda')
    results = {}
    for mode in ('eager', 'fused'):
        torch.manual_seed(9)
        feats = {'0': torch.randn(b, n, 16, 1, device='cuda',
                                  requires_grad=True),
                 '1': torch.randn(b, n, 16, 3, device='cuda',
                                  requires_grad=True)}
        with switches(SE3_EAGER_ATTN='1' if mode == 'eager' else None):
            out = attn(feats, (nbr_idx, nbr_mask, None), rel_dist, basis)
            loss = sum(t.pow(2).mean() for t in out.values())
            loss.backward()
        results[mode] = {'out0': out['0'].detach().clone(),
                         'out1': out['1'].detach().clone(),
                         'g0': feats['0'].grad.clone(),
                         'g1': feats['1'].grad.clone()}
        attn.zero_grad()
    for key in results['eager']:
        err = _rel_err(results['fused'][key], results['eager'][key])
        assert err < 2e-3, f'{key}: {err}'


@needs_gpu
def test_attn2_rotary_in_kernel_vs_eager():
    """Rotary q/k/v rotation folded into attn2 vs the eager apply_rotary
    path, full model forward AND backward (the in-kernel rotation's
    transpose map feeds dq/dk/dv), fp32."""
    from se3_transformer_amd import SE3Transformer
    torch.manual_seed(10)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=8, attend_self=True,
                           rotary_position=True, rotary_rel_dist=True).to('cuda')
    feats = torch.randn(2, 48, 32, device='cuda')
    coors = torch.randn(2, 48, 3, device='cuda')
    mask = torch.ones(2, 48, dtype=torch.bool, device='cuda')
    with switches(SE3_EAGER_ATTN='1'):
        ref = model(feats, coors, mask, return_type=0)
        ref.pow(2).mean().backward()
    gref = {n: p.grad.clone() for n, p in model.named_parameters()
            if p.grad is not None}
    model.zero_grad()
    out = model(feats, coors, mask, return_type=0)
    err = _rel_err(out, ref)
    assert err < 2e-3, f'rotary-in-kernel parity: {err}'
    out.pow(2).mean().backward()
    for n, p in model.named_parameters():
        if n not in gref:
            continue
        gerr = _rel_err(p.grad.float(), gref[n].float())
        assert gerr < 5e-3, f'rotary-in-kernel grad {n}: {gerr}'


@needs_gpu
def test_knn_kernel_large_k_and_neighbor_mask():
    """kNN kernel with k > 16 and a user neighbor_mask restricting
    candidate selection (both round-2 extensions), vs the eager build."""
    from se3_transformer_amd import SE3Transformer
    torch.manual_seed(11)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=40,
                           valid_radius=4.).to('cuda')
    b, n = 2, 150
    feats = torch.randn(b, n, 32, device='cuda')
    coors = torch.randn(b, n, 3, device='cuda') * 1.5
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    nbr_allow = torch.rand(b, n, n, device='cuda') > 0.3
    with switches(SE3_EAGER_KNN='1'):
        ref = model(feats, coors, mask, neighbor_mask=nbr_allow, return_type=0)
    out = model(feats, coors, mask, neighbor_mask=nbr_allow, return_type=0)
    err = (out - ref).abs().max().item()
    assert err < 1e-4, f'large-k/neighbor_mask knn mismatch: {err}'


@needs_gpu
def test_knn_kernel_sparse_adjacency():
    """kNN kernel with attend_sparse_neighbors + adjacency embeddings
    (qm9-style config) vs the eager build."""
    from se3_transformer_amd import SE3Transformer
    torch.manual_seed(12)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=4,
                           attend_sparse_neighbors=True, num_adj_degrees=2,
                           adj_dim=4, valid_radius=5.).to('cuda')
    b, n = 2, 29
    i = torch.arange(n, device='cuda')
    adj_mat = ((i[:, None] - i[None, :]).abs() == 1)
    feats = torch.randn(b, n, 32, device='cuda')
    coors = torch.randn(b, n, 3, device='cuda')
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    with switches(SE3_EAGER_KNN='1'):
        ref = model(feats, coors, mask, adj_mat=adj_mat, return_type=0)
    out = model(feats, coors, mask, adj_mat=adj_mat, return_type=0)
    err = (out - ref).abs().max().item()
    assert err < 1e-4, f'sparse-adjacency knn mismatch: {err}'


@needs_gpu
def test_ubuild_kernel_vs_einsum():
    """csrc/ubuild.hip: the basis x features precontraction vs the eager
    einsum, forward and dX backward."""
    from se3_transformer_amd.ops import fused as _fused

    torch.manual_seed(14)
    E, C, O, I, F_ = 500, 32, 7, 7, 7
    B = torch.randn(E, O, I, F_, device='cuda')
    x0 = torch.randn(E, C, I, device='cuda', requires_grad=True)
    x1 = x0.detach().clone().requires_grad_(True)

    ref = torch.einsum('eoif,eci->cfoe', B, x0).reshape(C * F_, O, E)
    ref.float().pow(2).mean().backward()

    out = _fused.ubuild(x1, B.contiguous(), O, I, F_)
    assert out.shape == (C * F_, O, E) and out.dtype == torch.bfloat16
    out.float().pow(2).mean().backward()

    assert _rel_err(out.float(), ref) < 1e-2, 'ubuild forward'
    # backward grads differ only by the bf16 rounding of the forward output
    assert _rel_err(x1.grad, x0.grad) < 3e-2, 'ubuild dX'


@needs_gpu
def test_egnn_kernels_vs_eager():
    """csrc/egnn.hip: gather-based rel-dists + htype update (no n^2
    intermediates) vs the eager full-matrix path, forward and grads."""
    from se3_transformer_amd import SE3Transformer

    torch.manual_seed(15)
    kwargs = dict(dim=32, depth=2, num_degrees=3, num_neighbors=6,
                  use_egnn=True, egnn_hidden_dim=16)
    model = SE3Transformer(**kwargs).to('cuda')
    feats = torch.randn(2, 32, 32, device='cuda')
    coors = torch.randn(2, 32, 3, device='cuda')
    mask = torch.ones(2, 32, dtype=torch.bool, device='cuda')

    with switches(SE3_EAGER_EGNN='1'):
        ref = model(feats, coors, mask, return_type=1)
        ref.pow(2).mean().backward()
    gref = {n: p.grad.clone() for n, p in model.named_parameters()
            if p.grad is not None}
    model.zero_grad()

    out = model(feats, coors, mask, return_type=1)
    assert _rel_err(out, ref) < 1e-4, 'egnn kernel forward'
    out.pow(2).mean().backward()
    g1 = {n: p.grad.clone() for n, p in model.named_parameters()
          if p.grad is not None}
    # HtypesNorm's bias/eps factor (~1e6 on self-edges) amplifies the f32
    # atomic-ordering noise of the scatter-add backward, so the kernel's
    # own run-to-run spread sets the honest tolerance: rerun and compare
    # kernel-vs-eager against a multiple of kernel-vs-kernel noise.
    model.zero_grad()
    out2 = model(feats, coors, mask, return_type=1)
    out2.pow(2).mean().backward()
    for n, p in model.named_parameters():
        if n not in gref:
            continue
        noise = _rel_err(p.grad.float(), g1[n].float())
        err = _rel_err(g1[n].float(), gref[n].float())
        assert err < max(5 * noise, 5e-3), \
            f'egnn kernel grad {n}: {err} (run noise {noise})'


@needs_gpu
def test_lowmem_pack_mode_matches_default():
    """SE3_LOWMEM_PACK=1 (save torch-layout W, re-pack in backward) must
    match the default save-both-packs path at the Function level: the
    forward kernel and dw/du/db are deterministic (bit-equal expected);
    dh uses split-K atomics (tight tolerance)."""
    from se3_transformer_amd.ops.fused import fused_pairconv

    torch.manual_seed(18)
    device = torch.device('cuda')
    mo, mi, F_, O, E = 16, 32, 5, 5, 700
    miF = mi * F_

    def run():
        g = torch.Generator(device).manual_seed(3)
        H = torch.randn(E, 128, generator=g, device=device,
                        requires_grad=True)
        W = torch.randn(mo * miF, 128, generator=g, device=device,
                        requires_grad=True)
        bias = torch.randn(mo * miF, generator=g, device=device,
                           requires_grad=True)
        Ut = torch.randn(miF, O, E, generator=g, device=device,
                         requires_grad=True)
        out = fused_pairconv(H, W, bias, Ut, mo)
        out.pow(2).mean().backward()
        return out.detach(), H.grad, W.grad, bias.grad, Ut.grad

    ref = run()
    with switches(SE3_LOWMEM_PACK='1'):
        low = run()
    names = ('out', 'dH', 'dW', 'db', 'dUt')
    for name, a, b in zip(names, low, ref):
        if name == 'dH':   # split-K atomics: order noise only
            assert _rel_err(a, b) < 1e-5, f'{name}'
        else:
            assert torch.equal(a, b), f'{name} differs between pack modes'
