"""Fused-kernel dispatch layer (MI355X HIP extension, se3_transformer_amd._C).

This module alone decides kernel vs eager. SWITCHES lists the runtime SE3_*
switches and switch() reads one, at call time. Each kernel family has one
gate (norm_ok ... egnn_ok) over shape arithmetic that needs no extension
(fused_shapes_ok, knn_ok, attn_shapes_ok, norm_shapes_ok). A gate tests
device, dtype, shape and switch before it touches the extension, so a CPU
forward never imports _C. Without the extension on a GPU pairconv_ok raises
and every other gate answers False (eager). _load_ext() checks the entry
points and the constants mirrored here once, at load.

Below them sit the autograd Functions wrapping the hand-written CDNA4
kernels in csrc/: pairwise convolution (fwd + the three dedicated backward
kernels + the one-pass dual-layout weight pack — the per-edge radial output
R of reference se3_transformer_pytorch.py:297-343 never touches HBM in
either direction), the radial trunk, the basis×features precontraction, the
SH basis, NormSE3, neighbor attention v2 (online softmax, in-kernel rotary,
HIP backward) and the EGNN higher-type ops. A chunked library-GEMM backward
for the pairconv remains behind SE3_TORCH_BWD as the parity oracle.
"""
from __future__ import annotations

import os

import torch

# Every runtime switch (the README table lists the same names). All are
# on/off, on when set to '1', except SE3_ATTN_MAX_J, which holds a number.
SWITCHES = {
    'SE3_EAGER_NORM': 'NormSE3 runs eager',
    'SE3_EAGER_RADIAL': 'the radial trunk runs eager',
    'SE3_EAGER_UBUILD': 'the basis x features precontraction runs eager',
    'SE3_EAGER_ATTN': 'neighbor attention (and its rotary) runs eager',
    'SE3_EAGER_KNN': 'the neighbor graph is built eager',
    'SE3_EAGER_BASIS': 'the SH basis runs eager',
    'SE3_EAGER_EGNN': 'the EGNN higher-type ops run eager',
    'SE3_FORCE_FUSED': 'pairconv kernels also for fp32 input outside autocast',
    'SE3_TORCH_BWD': 'pairconv backward through library GEMMs (parity oracle)',
    'SE3_LOWMEM_PACK': 'save W unpacked and re-pack in the pairconv backward',
    'SE3_RECOMPUTE_U': 'build U from node features and rebuild it in the '
                       'pairconv backward',
    'SE3_COMPACT_NEIGHBORS': 'cut neighbor columns that are invalid in every row',
    'SE3_STREAMS': 'run the degree pairs of a ConvSE3 on a stream pool',
    'SE3_ATTN_MAX_J': 'largest neighbor count the attention kernel takes',
}


def switch(name: str):
    """The environment's value of a runtime switch, read now: tests and
    scripts flip switches inside a process, so nothing is cached."""
    if name not in SWITCHES:
        raise KeyError(name)
    return os.environ.get(name)


def switch_on(name: str) -> bool:
    return switch(name) == '1'


_EXT = None
_EXT_ERR = None

# Every entry point the package calls. _load_ext() checks them once, so no
# caller probes the module again: a stale build is an error at load, not a
# reason to run eager.
_ENTRY_POINTS = (
    'pairconv_fwd_opad', 'pairconv_opad', 'pairconv_bwd_dh', 'pairconv_bwd_dw',
    'pairconv_bwd_du', 'pack_w_both', 'pack_g', 'radial_trunk_fwd',
    'radial_trunk_bwd', 'ubuild_fwd', 'ubuild_bwd_dx', 'ubuild_bwd_db',
    'ubuild_gather_fwd', 'ubuild_gather_bwd_dx', 'ubuild_gather_bwd_db',
    'sh_basis_fwd', 'sh_basis_bwd', 'knn_graph', 'knn_max_lds_bytes',
    'attn2_fwd', 'attn2_bwd', 'norm_se3_nl_fwd', 'norm_se3_nl_bwd',
    'norm_se3_gated_max_c', 'norm_se3_gated_fwd', 'norm_se3_gated_bwd',
    'egnn_rel_dist_fwd', 'egnn_rel_dist_bwd', 'egnn_htype_update_fwd',
    'egnn_htype_update_bwd',
)

# Channel ceiling of the gated kernels (GATED_MAX_C in csrc/norm_se3.hip):
# their LDS tile is 16*C bytes per block.
NORM_GATED_MAX_C = 2048

# Dynamic-LDS ceiling of the kNN kernel (KNN_MAX_LDS_BYTES in csrc/knn.hip):
# what a launch gets without raising the kernel's LDS attribute. A block
# holds 64 sorted lists of L = min(k, ceil(n/64)) (distance, index) pairs
# plus the k winners.
KNN_MAX_LDS = 65536

# Padded o width OP(O) of the edge-major tensors U (miF, E, OP),
# G (mo, E, OP) and dU (miF, E, OP) (opad_of in csrc/pairconv_common.h).
_OPAD = {1: 1, 3: 4, 5: 8, 7: 8}


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            from se3_transformer_amd import _C as mod
        except ImportError as e:  # pragma: no cover
            _EXT_ERR = e
            return None
        missing = [n for n in _ENTRY_POINTS if not hasattr(mod, n)]
        if not missing:
            if mod.norm_se3_gated_max_c() != NORM_GATED_MAX_C:
                missing.append(f'norm_se3_gated_max_c() == {NORM_GATED_MAX_C}')
            if mod.knn_max_lds_bytes() != KNN_MAX_LDS:
                missing.append(f'knn_max_lds_bytes() == {KNN_MAX_LDS}')
            missing += [f'pairconv_opad({O}) == {OP}' for O, OP in _OPAD.items()
                        if mod.pairconv_opad(O) != OP]
        if missing:
            raise RuntimeError(
                'se3_transformer_amd._C lacks ' + ', '.join(missing)
                + '; rebuild the extension (python scripts/build_ext.py)')
        _EXT = mod
    return _EXT


def ext_available() -> bool:
    return _load_ext() is not None


def require_ext():
    """On a CUDA/ROCm device the HIP extension must be present — fail loudly
    rather than silently falling back to eager."""
    if not ext_available():
        raise RuntimeError(
            'se3_transformer_amd._C HIP extension is not built but a GPU is '
            'present; run `python scripts/build_ext.py` '
            f'(import error: {_EXT_ERR})')


# Shape arithmetic first (no extension needed to ask), then one gate per family.

def knn_lds_bytes(n: int, k: int) -> int:
    return min(k, -(-n // 64)) * 64 * 8 + 4 * k


def knn_ok(n: int, k: int) -> bool:
    """True when the kNN kernel serves (n, k): any 1 <= k <= n-1 whose LDS
    footprint fits KNN_MAX_LDS (k = n-1 up to n ~ 5400)."""
    return 1 <= k <= n - 1 and knn_lds_bytes(n, k) <= KNN_MAX_LDS


def fused_shapes_ok(mo: int, miF: int, O: int, mid_dim: int) -> bool:
    """Any channel counts: the kernels run on tiles zero-padded to
    (ceil8(mo), ceil32(miF)), see pad_dims."""
    return mid_dim == 128 and miF >= 1 and mo >= 1 and O in (1, 3, 5, 7)


def pad_dims(mo: int, miF: int):
    """(mo_p, miF_p) = (ceil8(mo), ceil32(miF)): the MFMA tile of the pairconv
    kernels (ceil_mo, ceil_mif in csrc/pairconv_common.h). Packed W, bias, U
    and G are zero outside the true (mo, miF); out, dW and db keep the true
    sizes."""
    return -(-mo // 8) * 8, -(-miF // 32) * 32


def attn_shapes_ok(J: int, dm: int, rot: int = 0) -> bool:
    """csrc/attn2.hip: any J up to SE3_ATTN_MAX_J, DM bounded by the per-lane
    register chunking, in-kernel rotary width even, <= 64 and within DM."""
    max_j = switch('SE3_ATTN_MAX_J')
    return (J <= (100000 if max_j is None else int(max_j)) and dm <= 448
            and rot <= 64 and rot % 2 == 0 and rot <= dm)


def norm_shapes_ok(C: int, M: int, gated: bool) -> bool:
    """csrc/norm_se3.hip: order M = 2d+1 in {1,3,5,7}; the LDS tile of the
    gated kernels holds up to NORM_GATED_MAX_C channels."""
    return M in (1, 3, 5, 7) and not (gated and C > NORM_GATED_MAX_C)


RADIAL_TRUNK_DIMS = (1, 2, 3, 5, 9, 17, 21, 25)   # instantiated in csrc/radial.hip
_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


def norm_ok(t, gated: bool, nonlin) -> bool:
    """nonlin is the kernels' selector ('gelu' | 'identity') or None."""
    return (nonlin is not None and t.is_cuda and t.dim() >= 2
            and t.dtype in _KERNEL_DTYPES
            and norm_shapes_ok(t.shape[-2], t.shape[-1], gated)
            and not switch_on('SE3_EAGER_NORM') and ext_available())


def radial_trunk_ok(in_dim: int, mid_dim: int) -> bool:
    return mid_dim == 128 and in_dim in RADIAL_TRUNK_DIMS and ext_available()


def radial_ok(x, mid_dim: int, eps0: float = 1e-5, eps3: float = 1e-5) -> bool:
    """The kernel has one eps for both LayerNorms (net.1 and net.4)."""
    return (x.is_cuda and eps0 == eps3 and not switch_on('SE3_EAGER_RADIAL')
            and radial_trunk_ok(x.shape[-1], mid_dim))


def ubuild_ok(B, C, O, I, F) -> bool:
    return (B.is_cuda and B.dtype == torch.float32
            and C >= 1 and O * I * F <= 343
            and not switch_on('SE3_EAGER_UBUILD') and ext_available())


def recompute_u_ok(x_nodes, B, C, O, I, F) -> bool:
    """SE3_RECOMPUTE_U: the pair builds U from node features (N, C, I) and
    edge rows, and builds it again in backward instead of saving it. The
    gather kernels take C % 32 == 0 only: other pairs keep the saved U."""
    return (x_nodes.is_cuda and x_nodes.dtype in _KERNEL_DTYPES
            and C % 32 == 0
            and switch_on('SE3_RECOMPUTE_U') and ubuild_ok(B, C, O, I, F))


def pairconv_ok(x, mo: int, miF: int, O: int, mid_dim: int) -> bool:
    """bf16 compute: under autocast, for bf16 features, or SE3_FORCE_FUSED.
    The one gate that raises when the extension is missing on a GPU."""
    if not (x.is_cuda
            and (torch.is_autocast_enabled() or x.dtype == torch.bfloat16
                 or switch_on('SE3_FORCE_FUSED'))
            and fused_shapes_ok(mo, miF, O, mid_dim)):
        return False
    require_ext()
    return True


def attn_ok(q, J: int, dm: int, rot: int = 0) -> bool:
    return (q.is_cuda and q.dtype in _KERNEL_DTYPES
            and attn_shapes_ok(J, dm, rot)
            and not switch_on('SE3_EAGER_ATTN') and ext_available())


def rope_ok(q, j_pre, qpe, kpe, use_null_kv, global_feats) -> bool:
    """True if the rotary embedding can be folded into the attention kernel
    (q/k/v rotated in-registers, no rotated copies). The frequency tables
    must not need grad (rotary_rel_dist with differentiable coors is eager)."""
    gj = 0
    if global_feats is not None:   # fiber dict {'0': (b, gj, d, 1)}
        gj = next(iter(global_feats.values())).shape[1]
    j_fin = j_pre + (1 if use_null_kv else 0) + gj
    return (kpe.shape[2] == j_pre
            and not qpe.requires_grad and not kpe.requires_grad
            and attn_ok(q, j_fin, q.shape[-2] * q.shape[-1], qpe.shape[-1]))


def knn_kernel_ok(coors, n: int, k: int) -> bool:
    return (coors.is_cuda and coors.dtype == torch.float32 and knn_ok(n, k)
            and not switch_on('SE3_EAGER_KNN') and ext_available())


def sh_basis_ok(r_ij) -> bool:
    return (r_ij.is_cuda and r_ij.dtype == torch.float32
            and not switch_on('SE3_EAGER_BASIS') and ext_available())


def egnn_ok(nodes, n_htypes: int, max_m: int) -> bool:
    return (nodes.is_cuda and n_htypes > 0 and max_m <= 7
            and not switch_on('SE3_EAGER_EGNN') and ext_available())


def knn_graph(*args):
    """csrc/knn.hip: 4 inputs, 4 outputs (idx, dist, rel, m), k, radius, causal."""
    _load_ext().knn_graph(*args)


def _pad_rows(W, mo, miF):
    """W (mo*miF, ...) -> (mo_p*miF_p, ...) with zero rows outside the true
    (mo, miF); W itself where nothing is to pad."""
    mo_p, miF_p = pad_dims(mo, miF)
    if (mo_p, miF_p) == (mo, miF):
        return W
    Wp = W.new_zeros(mo_p, miF_p, *W.shape[1:])
    Wp[:mo, :miF] = W.view(mo, miF, *W.shape[1:])
    return Wp.view(mo_p * miF_p, *W.shape[1:])


def _pack_w_fwd(W16, mo, miF):
    """Rearrange W (mo*miF, 128) bf16 into the forward/du kernels' per-lane
    fragment order [mo_p/8][miF_p/32][wm4][mf4][kit4][lane64][j8] so each
    wave's MFMA A-fragment load is one contiguous 1 KiB read. Rows outside
    the true (mo, miF) are zero."""
    mo_p, miF_p = pad_dims(mo, miF)
    v = _pad_rows(W16, mo, miF) \
        .view(mo_p // 8, 4, 2, miF_p // 32, 2, 16, 4, 4, 8)
    return v.permute(0, 3, 1, 2, 4, 6, 7, 5, 8).contiguous()


def _pack_w_dh(W16, mo, miF):
    """Fragment order for the dH kernel's B-operand:
    [mo_p/8][miF_p/32][wk2][kf4][ns8][lane64][j8], zero outside (mo, miF)."""
    mo_p, miF_p = pad_dims(mo, miF)
    v = _pad_rows(W16, mo, miF) \
        .view(mo_p // 8, 8, miF_p // 32, 4, 8, 2, 4, 16)
    return v.permute(0, 2, 5, 6, 1, 3, 7, 4).contiguous()


def _pad_u_rows(U, miF):
    """U (miF or miF_p, E, OP) -> (miF_p, E, OP): a U that already has the
    padded rows is trusted to hold zeros there (ubuild_opad writes them)."""
    miF_p = pad_dims(1, miF)[1]
    if U.shape[0] == miF_p:
        return U
    if U.shape[0] != miF:
        raise ValueError(f'U has {U.shape[0]} rows, W implies {miF} '
                         f'(or {miF_p} with zero pad rows)')
    Up = U.new_zeros(miF_p, *U.shape[1:])
    Up[:miF] = U
    return Up


def opad(O: int) -> int:
    """Padded o width OP(O): 7, 5 -> 8; 3 -> 4; 1 -> 1."""
    return _OPAD[O]


def _to_opad(Ut, O):
    """(rows, O, E) -> (rows, E, OP) contiguous with zero pads."""
    return torch.nn.functional.pad(Ut.permute(0, 2, 1),
                                   (0, opad(O) - O)).contiguous()


class _FusedPairConvOpad(torch.autograd.Function):
    """out[e,mo,o] = sum_{c,h} (H[e,h] W[(mo,c),h] + bias[(mo,c)]) * U[c,e,o]

    H (E,128) bf16 | W (mo*miF,128) fp32/bf16 param | bias (mo*miF,) fp32
    U (miF,E,OP) bf16, pad lanes o in [O, OP) exactly zero | returns
    (E, mo, O) fp32. Any mo, miF >= 1 (miF is W's, rows / mo): U may also
    come with ceil32(miF) rows, the pad rows exactly zero (as ubuild_opad
    writes it), and is padded here otherwise. The gradient of U comes back
    with the rows and pads of U as passed, in bf16 (the du kernel rounds its
    fp32 sums once, as autograd's cast to U's dtype did) or in fp32 with
    SE3_TORCH_BWD. The kernels
    contract whole padded vectors and the bias term's library GEMM reads U
    as a (miF, E*OP) matrix: both rely on the zero pads.
    """

    @staticmethod
    def forward(ctx, H, W, bias, U, mo, O):
        U16 = _pad_u_rows(U.contiguous().to(torch.bfloat16), W.shape[0] // mo)
        out, H16, wsave, b16 = _pairconv_forward(ctx, H, W, bias, U16, mo, O)
        ctx.save_for_backward(H16, *wsave, U16, b16)
        ctx.u_rows = U.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        H16, *wsave, U16, b16 = ctx.saved_tensors
        dH, dW, db, dU = _pairconv_backward(ctx, H16, wsave, b16, U16, grad_out,
                                            ctx.needs_input_grad[:4])
        if dU is not None:
            dU = dU[:ctx.u_rows]
        return dH, dW, db, dU, None, None


def _pairconv_forward(ctx, H, W, bias, U16, mo, O):
    """The forward of both pairconv Functions on U16 (miF_p, E, OP) bf16,
    rows >= miF zero. Returns out (E, mo, O) and what the backward needs
    besides U: H16, wsave (both fragment packs of W, sized for the padded
    dims, or W16 alone: ctx.packed says which) and b16 (mo, miF)."""
    ext = _load_ext()
    E = H.shape[0]
    miF = W.shape[0] // mo
    mo_p, miF_p = pad_dims(mo, miF)
    OP = U16.shape[2]
    if W.shape[0] != mo * miF or U16.shape[0] != miF_p:
        raise ValueError(f'W {tuple(W.shape)} and U {tuple(U16.shape)} do not '
                         f'fit mo={mo}')
    H16 = H.contiguous().to(torch.bfloat16)
    # bias term: out0[e,mo,o] = sum_c bias[mo,c] U[c,e,o], on the true rows
    b16 = bias.detach().to(torch.bfloat16).view(mo, miF)
    out = (b16 @ U16[:miF].view(miF, E * OP)).view(mo, E, OP)[:, :, :O] \
        .permute(1, 0, 2).contiguous().float()
    hip_bwd = not switch_on('SE3_TORCH_BWD')
    # SE3_LOWMEM_PACK=1 trades ~6% step time for memory: save the
    # torch-layout bf16 W (1x) and re-pack in backward, instead of
    # holding both packed fragment layouts (2x) through autograd —
    # frees ~36 GB at the headline 18.2B-param config (enables larger
    # neighbor counts before the activation-memory wall).
    lowmem = switch_on('SE3_LOWMEM_PACK')
    if hip_bwd and not lowmem:
        # one-pass pack kernel: W read once, both fragment layouts
        # written; saved for backward so nothing re-packs per step
        Wd = W.detach().contiguous()
        n128 = mo_p * miF_p * 128
        Pf = torch.empty(n128, dtype=torch.bfloat16, device=Wd.device)
        Pdh = torch.empty(n128, dtype=torch.bfloat16, device=Wd.device)
        ext.pack_w_both(Wd, Pf, Pdh, mo)    # pad rows written as zeros
        ext.pairconv_fwd_opad(H16, Pf, U16, out, mo_p)
        wsave = (Pf, Pdh)
        ctx.packed = True
    else:
        W16 = W.detach().contiguous().to(torch.bfloat16)
        ext.pairconv_fwd_opad(H16, _pack_w_fwd(W16, mo, miF), U16, out, mo_p)
        wsave = (W16,)
        ctx.packed = False
    ctx.mo = mo
    ctx.O = O
    ctx.w_dtype = W.dtype
    ctx.b_dtype = bias.dtype
    return out, H16, wsave, b16


def _pairconv_backward(ctx, H16, wsave, b16, U16, grad_out, needs):
    """The backward of both pairconv Functions on U16, saved or rebuilt:
    (dH, dW, db, dU) for needs = (need_H, need_W, need_b, need_u)."""
    mo, O = ctx.mo, ctx.O
    if ctx.packed:
        Pf, Pdh = wsave
    else:
        W16, = wsave
    E, K = H16.shape
    miF = b16.shape[1]
    mo_p, miF_p = pad_dims(mo, miF)
    OP = U16.shape[2]
    g = grad_out.contiguous().float()              # (E, mo, O) fp32

    need_H, need_W, need_b, need_u = needs

    ext = _load_ext()
    if not switch_on('SE3_TORCH_BWD'):
        dH = dW = db = dU = None
        # one pass: cast, transpose and pad, (mo_p, E, OP) bf16, rows >= mo
        # written as zeros
        G = torch.empty(mo_p, E, OP, dtype=torch.bfloat16, device=g.device)
        ext.pack_g(g, G)
        P1 = Pu = None
        if ctx.packed:
            P1, Pu = Pdh, Pf
        elif need_H or need_u:
            # SE3_LOWMEM_PACK path: re-derive both fragment layouts in
            # one kernel pass from the saved torch-layout W
            n128 = mo_p * miF_p * K
            Pu = torch.empty(n128, dtype=torch.bfloat16,
                             device=H16.device)
            P1 = torch.empty_like(Pu)
            ext.pack_w_both(W16, Pu, P1, mo)
        if need_H:
            dH = torch.zeros(E, K, dtype=torch.float32, device=H16.device)
            ext.pairconv_bwd_dh(G, U16, P1, dH, mo_p, O)
        P1 = None
        if need_W or need_b:
            # db[(m,c)] = sum_e dR[e,(m,c)]: the dw kernel sums the fp32 dR
            # entries it builds anyway (an empty db: not wanted)
            Ht = H16.t().contiguous()              # (128, E)
            # 3-D: the true sizes, which the kernel guards its stores by
            dW = torch.empty(mo, miF, K, dtype=torch.float32,
                             device=H16.device)
            db = torch.empty(mo * miF if need_b else 0, dtype=torch.float32,
                             device=H16.device)
            ext.pairconv_bwd_dw(G, U16, Ht, dW, db, mo_p, O)
            dW = dW.view(mo * miF, K).to(ctx.w_dtype) if need_W else None
            db = db.to(ctx.b_dtype) if need_b else None
            del Ht
        if need_u:
            # bf16 as U: the kernel rounds its fp32 sums once
            dU = torch.empty(miF_p, E, OP, dtype=torch.bfloat16,
                             device=H16.device)
            ext.pairconv_bwd_du(H16, Pu, _pad_rows(b16.float().reshape(-1),
                                                   mo, miF),
                                G, dU, mo_p, O)
        return dH, dW, db, dU

    if ctx.packed:   # pragma: no cover - env toggled between fwd and bwd
        raise RuntimeError('SE3_TORCH_BWD enabled after a packed forward; '
                           'set it before the forward pass')
    g16 = g.to(torch.bfloat16)
    u_eco = U16[:miF, :, :O].permute(1, 0, 2)      # (E, miF, O) view
    dH = dW = db = dU = None
    if need_H:
        dH = torch.zeros(E, K, dtype=torch.float32, device=H16.device)
    if need_W:
        dW = torch.empty(mo * miF, K, dtype=torch.float32, device=H16.device)
    if need_b:
        db = torch.empty(mo * miF, dtype=torch.float32, device=H16.device)
    if need_u:
        dU = torch.zeros(miF_p, E, OP, dtype=torch.float32, device=H16.device)

    # chunk over mo so the dR slab stays ~<= 1 GiB
    per_mo = E * miF * 2
    cm = max(8, min(mo, (1 << 30) // max(per_mo, 1) // 8 * 8))
    for m0 in range(0, mo, cm):
        m1 = min(mo, m0 + cm)
        # dR[e,(m,c)] = sum_o g[e,m,o] * u[e,c,o]
        dR16 = torch.einsum('emo,eco->emc', g16[:, m0:m1], u_eco) \
            .reshape(E, (m1 - m0) * miF)
        Wslab = W16[m0 * miF:m1 * miF]             # ((m1-m0)*miF, K)
        if need_H:
            dH += (dR16 @ Wslab).float()
        if need_W:
            dW[m0 * miF:m1 * miF] = (dR16.t() @ H16).float()
        if need_b:
            db[m0 * miF:m1 * miF] = dR16.float().sum(dim=0)
        if need_u:
            # R[e,(m,c)] = H @ W^T + bias ; du[c,e,o] += sum_m R * g
            R = (H16 @ Wslab.t()).view(E, m1 - m0, miF).float() \
                + b16[m0:m1].float().unsqueeze(0)
            dU[:miF, :, :O] += torch.einsum('emc,emo->ceo', R, g[:, m0:m1])
        del dR16

    if need_W:
        dW = dW.to(ctx.w_dtype)
    if need_b:
        db = db.to(ctx.b_dtype)
    return dH, dW, db, dU


def fused_pairconv_opad(H, W, bias, U, mo, O=None):
    """Pairwise convolution on U in the o-padded edge-major layout
    (miF, E, OP(O)) with zero pads, for any mo, miF >= 1 (miF = W rows / mo);
    returns (E, mo, O) and differentiates to dU in the shape of U.

    U may instead carry ceil32(miF) rows, as ubuild_opad returns it. The pad
    rows [miF, ceil32(miF)) must then be EXACTLY ZERO, like the pad lanes:
    they are not checked (that would cost a pass over U and a host sync per
    call), the forward, dh and dw kernels contract them as they stand, and
    anything else there gives a wrong out, dH and dW without an error. Pass
    U with its miF true rows to have the pads made here. O may be omitted where OP decides
    it (OP 1 -> O 1, OP 4 -> O 3); OP 8 serves O 5 and 7, so say which."""
    OP = U.shape[2]
    if O is None:
        if OP == 8:
            raise ValueError('U with OP=8 serves O=5 and O=7: pass O')
        O = {1: 1, 4: 3}[OP]
    if opad(O) != OP:
        raise ValueError(f'U has o width {OP}, O={O} needs {opad(O)}')
    return _FusedPairConvOpad.apply(H, W, bias, U, mo, O)


def fused_pairconv(H, W, bias, Ut, mo):
    """The same on Ut in the e-contiguous (miF, O, E) layout: a
    differentiable torch repack around fused_pairconv_opad, for producers
    and callers that do not emit the padded layout themselves."""
    O = Ut.shape[1]
    return fused_pairconv_opad(H, W, bias, _to_opad(Ut, O), mo, O)


NORM_NONLIN = {'gelu': 0, 'identity': 1}   # selector of csrc/norm_se3.hip


class _NormSE3Fn(torch.autograd.Function):
    """Fused equivariant norm-gate (csrc/norm_se3.hip), scale path.
    nl selects the nonlinearity (NORM_NONLIN): exact-erf GELU or identity."""

    @staticmethod
    def forward(ctx, t, scale, eps, nl=0):
        ext = _load_ext()
        s32 = scale.detach().reshape(-1).float().contiguous()
        out = torch.empty_like(t)
        ext.norm_se3_nl_fwd(t, s32, out, eps, nl)
        ctx.save_for_backward(t, s32)
        ctx.eps = eps
        ctx.nl = nl
        ctx.scale_shape = scale.shape
        ctx.scale_dtype = scale.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = _load_ext()
        t, s32 = ctx.saved_tensors
        dt = torch.empty_like(t)
        dscale = torch.zeros_like(s32)
        ext.norm_se3_nl_bwd(t, s32, dout.contiguous(), dt, dscale,
                            ctx.eps, ctx.nl)
        return (dt, dscale.view(ctx.scale_shape).to(ctx.scale_dtype),
                None, None)


class _NormSE3GatedFn(torch.autograd.Function):
    """Fused gated-scale NormSE3 (csrc/norm_se3.hip):
    out = g(|t| @ w_gate) * t/|t| with w_gate (C, C) and the norms kept in
    fp32 in front of the nonlinearity. The forward saves gate (N, C) fp32;
    the backward kernel returns dt plus dgate and nu, and
    dW = nu^T @ dgate is one library GEMM (deterministic, no atomics).
    First order only."""

    @staticmethod
    def forward(ctx, t, w_gate, eps, nl=0):
        ext = _load_ext()
        w32 = w_gate.detach().float().contiguous()
        out = torch.empty_like(t)
        gate = torch.empty(t.shape[:-1], dtype=torch.float32, device=t.device)
        ext.norm_se3_gated_fwd(t, w32, out, gate, eps, nl)
        ctx.save_for_backward(t, w32, gate)
        ctx.eps = eps
        ctx.nl = nl
        ctx.w_dtype = w_gate.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        ext = _load_ext()
        t, w32, gate = ctx.saved_tensors
        C = w32.shape[0]
        dt = torch.empty_like(t)
        dgate = torch.empty_like(gate)
        nu = torch.empty_like(gate)
        ext.norm_se3_gated_bwd(t, w32.t().contiguous(), gate,
                               dout.contiguous(), dt, dgate, nu,
                               ctx.eps, ctx.nl)
        dW = None
        if ctx.needs_input_grad[1]:
            dW = torch.mm(nu.view(-1, C).t(), dgate.view(-1, C)) \
                .to(ctx.w_dtype)
        return dt, dW, None, None


def norm_se3(t, scale, eps, nonlin='gelu'):
    return _NormSE3Fn.apply(t, scale, eps, NORM_NONLIN[nonlin])


def norm_se3_gated(t, w_gate, eps, nonlin='gelu'):
    return _NormSE3GatedFn.apply(t, w_gate, eps, NORM_NONLIN[nonlin])


def _attn_optional(mask_u8, qf, kf, dev):
    """The kernels take an empty tensor where an optional input is absent."""
    return [t if t is not None else torch.empty(0, dtype=dtype, device=dev)
            for t, dtype in ((mask_u8, torch.uint8), (qf, None), (kf, None))]


class _AttnFn(torch.autograd.Function):
    """Fused neighbor attention v2 (csrc/attn2.hip): rows (b,h,i), keys in
    64-wide online-softmax tiles (J unbounded), rotary embeddings applied to
    q/k/v in-kernel on degree 0, HIP backward via the saved logsumexp.
    qf/kf are the RAW rotary frequency tables (or None); gradients do not
    flow into them (the wrapper gates on their requires_grad)."""

    @staticmethod
    def forward(ctx, q, k, v, mask_u8, qf, kf, n, heads, scale, kv_one=False):
        ext = _load_ext()
        R, DM = q.shape
        dev = q.device
        out = torch.empty(R, DM, dtype=torch.float32, device=dev)
        lse = torch.empty(R, dtype=torch.float32, device=dev)
        m, qf_, kf_ = _attn_optional(mask_u8, qf, kf, dev)
        jr = kf.shape[1] if kf is not None else 0
        rot = (qf.shape[-1] if qf is not None
               else (kf.shape[-1] if kf is not None else 0))
        ext.attn2_fwd(q, k, v, m, qf_, kf_, out, lse,
                      n, heads, scale, kv_one, jr, rot)
        ctx.save_for_backward(q, k, v, mask_u8, qf, kf, out, lse)
        ctx.dims = (n, heads, scale, kv_one, jr, rot)
        return out

    @staticmethod
    def backward(ctx, g):
        ext = _load_ext()
        q, k, v, mask_u8, qf, kf, out, lse = ctx.saved_tensors
        n, heads, scale, kv_one, jr, rot = ctx.dims
        R, DM = q.shape
        dev = q.device
        m, qf_, kf_ = _attn_optional(mask_u8, qf, kf, dev)
        dq = torch.empty(R, DM, dtype=torch.float32, device=dev)
        if kv_one:
            # heads share KV rows: the kernel accumulates atomically
            dk = torch.zeros(k.shape, dtype=torch.float32, device=dev)
            dv = torch.zeros(v.shape, dtype=torch.float32, device=dev)
        else:
            dk = torch.empty(k.shape, dtype=torch.float32, device=dev)
            dv = torch.empty(v.shape, dtype=torch.float32, device=dev)
        ext.attn2_bwd(q, k, v, m, qf_, kf_, out, lse,
                      g.contiguous().float(), dq, dk, dv,
                      n, heads, scale, kv_one, jr, rot)
        return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype),
                None, None, None, None, None, None, None)


def fused_attention(q, k, v, mask_u8, n, heads, scale, kv_one=False,
                    qf=None, kf=None):
    return _AttnFn.apply(q, k, v, mask_u8, qf, kf, n, heads, scale, kv_one)


class _UBuildFn(torch.autograd.Function):
    """Basis-feature precontraction (csrc/ubuild.hip):
    U[(c f), e, o] = sum_i B[e,o,i,f] x[e,c,i], emitted directly in the
    o-padded edge-major layout (miF_p, E, OP), miF_p = ceil32(C*F), the
    pairconv kernels consume, pad lanes and the pad rows [C*F, miF_p) zero.
    When the basis requires grad (differentiable_coors) x is saved too and backward also returns
    dB[e,o,i,f] = sum_c x[e,c,i] dU[(c f),e,o] in fp32, straight-through
    for the forward's bf16 rounding. First order only."""

    @staticmethod
    def forward(ctx, x, B, O, I, F):
        ext = _load_ext()
        E, C, _ = x.shape
        # ceil32(C*F) rows: the kernel writes the pad rows as zeros
        U = torch.empty(pad_dims(1, C * F)[1], E, opad(O),
                        dtype=torch.bfloat16, device=x.device)
        xc = x.contiguous()
        ext.ubuild_fwd(B, xc, U, O, I, F)
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(B, xc)
        else:
            ctx.save_for_backward(B)
        ctx.meta = (x.dtype, x.shape, O, I, F)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dU):
        ext = _load_ext()
        B = ctx.saved_tensors[0]
        dtype, (E, C, I_), O, I, F = ctx.meta
        dU = dU.contiguous()       # (ceil32(C*F), E, OP), bf16 as U: read as is
        dX = dB = None
        if ctx.needs_input_grad[0]:
            dX = torch.empty(E, C, I, dtype=dtype, device=B.device)
            ext.ubuild_bwd_dx(B, dU, dX, O, I, F)
        if ctx.needs_input_grad[1]:
            dB = torch.empty(E, O, I, F, dtype=torch.float32, device=B.device)
            ext.ubuild_bwd_db(ctx.saved_tensors[1], dU, dB, O, I, F)
        return dX, dB, None, None, None


def ubuild_opad(x, B, O, I, F):
    """U (ceil32(C*F), E, OP(O)) bf16, zero pad lanes and pad rows: what
    fused_pairconv_opad reads."""
    return _UBuildFn.apply(x, B, O, I, F)


def ubuild(x, B, O, I, F):
    """The e-contiguous (C*F, O, E) contract, as a view of ubuild_opad."""
    return ubuild_opad(x, B, O, I, F)[:x.shape[1] * F, :, :O].permute(0, 2, 1)


def edge_rows(neighbor_indices, n: int):
    """(b, n', k) neighbor indices into n nodes per batch -> (b*n'*k,) int32
    rows batch*n + index of the features flattened to (b*n, C, I)."""
    b = neighbor_indices.shape[0]
    base = torch.arange(b, device=neighbor_indices.device).view(b, 1, 1) * n
    return (neighbor_indices + base).reshape(-1).to(torch.int32).contiguous()


class _PairConvNodesFn(torch.autograd.Function):
    """ubuild and pairconv of one degree pair in one node, on the features
    per NODE (SE3_RECOMPUTE_U): out = _FusedPairConvOpad(H, W, bias, U) with
    U = ubuild(Xn[rows], B), the same bits, but U is a temporary of the
    forward and is built again in the backward. Saved instead: Xn (N, C, I),
    rows (E,) int32 and B. Neither the gathered features (E, C, I) nor their
    gradient exist: dXn (N, C, I) is summed in fp32 by atomic adds and cast
    once. dB comes back when the basis requires grad. First order only."""

    @staticmethod
    def forward(ctx, Xn, rows, B, H, W, bias, mo, O, I, F):
        Xc = Xn.contiguous()
        U16 = _PairConvNodesFn._build_u(Xc, rows, B, O, I, F)
        out, H16, wsave, b16 = _pairconv_forward(ctx, H, W, bias, U16, mo, O)
        ctx.save_for_backward(Xc, rows, B, H16, *wsave, b16)
        ctx.IF = (I, F)
        return out

    @staticmethod
    def _build_u(Xc, rows, B, O, I, F):
        U16 = torch.empty(Xc.shape[1] * F, rows.shape[0], opad(O),
                          dtype=torch.bfloat16, device=Xc.device)
        _load_ext().ubuild_gather_fwd(B, Xc, rows, U16, O, I, F)
        return U16

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ext = _load_ext()
        Xc, rows, B, H16, *wsave, b16 = ctx.saved_tensors
        O, (I, F) = ctx.O, ctx.IF
        need_X, _, need_B, need_H, need_W, need_b = ctx.needs_input_grad[:6]
        dH, dW, db, dU = _pairconv_backward(
            ctx, H16, wsave, b16,
            _PairConvNodesFn._build_u(Xc, rows, B, O, I, F), grad_out,
            (need_H, need_W, need_b, need_X or need_B))
        dXn = dB = None
        if dU is not None:
            # between _FusedPairConvOpad and _UBuildFn autograd casts dU to
            # the dtype of U, bf16. The du kernel has rounded it already; the
            # fp32 dU of SE3_TORCH_BWD is rounded here, so dXn and dB stay
            # those of the unfused path
            dU = dU.to(torch.bfloat16)
        if need_X:
            # zeroed here, inside whatever graph captures the backward
            dXn = torch.zeros(Xc.shape, dtype=torch.float32, device=Xc.device)
            ext.ubuild_gather_bwd_dx(B, dU, rows, dXn, O, I, F)
            dXn = dXn.to(Xc.dtype)
        if need_B:
            dB = torch.empty(B.shape, dtype=torch.float32, device=B.device)
            ext.ubuild_gather_bwd_db(Xc, rows, dU, dB, O, I, F)
        return dXn, None, dB, dH, dW, db, None, None, None, None


def pairconv_from_nodes(Xn, rows, B, H, W, bias, mo, O, I, F):
    """fused_pairconv_opad(H, W, bias, ubuild_opad(Xn[rows], B, O, I, F),
    mo, O) without saving U or gathering Xn: Xn (N, C, I) fp32/bf16, rows
    (E,) int32 in [0, N), B (E, O, I, F) fp32 contiguous. Returns (E, mo, O).
    The kernels do not fault on a row outside [0, N): they read its x as zero
    and drop its gradient, so a wrong index shows as a wrong result only."""
    return _PairConvNodesFn.apply(Xn, rows, B, H, W, bias, mo, O, I, F)


class _HtypeRelDistFn(torch.autograd.Function):
    """EGNN neighbor rel-htype distances (csrc/egnn.hip): straight from the
    gathered neighbor indices — the O(n^2 d m) pairwise rel tensor of the
    eager path never exists."""

    @staticmethod
    def forward(ctx, ht, idx):
        ext = _load_ext()
        b, n, d, m = ht.shape
        k = idx.shape[2]
        dist = torch.empty(b, n, k, d, dtype=torch.float32, device=ht.device)
        htc = ht.contiguous()
        ext.egnn_rel_dist_fwd(htc, idx.contiguous(), dist)
        ctx.save_for_backward(htc, idx)
        return dist

    @staticmethod
    def backward(ctx, gdist):
        ext = _load_ext()
        ht, idx = ctx.saved_tensors
        dht = torch.zeros(ht.shape, dtype=torch.float32, device=ht.device)
        ext.egnn_rel_dist_bwd(ht, idx, gdist.contiguous().float(), dht)
        return dht.to(ht.dtype), None


def htype_rel_dist(ht, idx):
    return _HtypeRelDistFn.apply(ht, idx)


class _HtypeUpdateFn(torch.autograd.Function):
    """EGNN htype update (csrc/egnn.hip): HtypesNorm of the neighbor
    rel-htypes + weighted sum over neighbors, fused and gather-based."""

    @staticmethod
    def forward(ctx, ht, idx, w, scale, bias, eps):
        ext = _load_ext()
        b, n, d, m = ht.shape
        htc = ht.contiguous()
        wc = w.detach().float().contiguous()
        s32 = scale.detach().reshape(-1).float().contiguous()
        b32 = bias.detach().reshape(-1).float().contiguous()
        upd = torch.empty(b, n, d, m, dtype=torch.float32, device=ht.device)
        ext.egnn_htype_update_fwd(htc, idx.contiguous(), wc, s32, b32,
                                  upd, eps)
        ctx.save_for_backward(htc, idx, wc, s32, b32)
        ctx.meta = (eps, w.dtype, scale.shape, scale.dtype)
        return upd

    @staticmethod
    def backward(ctx, g):
        ext = _load_ext()
        ht, idx, wc, s32, b32 = ctx.saved_tensors
        eps, w_dtype, p_shape, p_dtype = ctx.meta
        dht = torch.zeros(ht.shape, dtype=torch.float32, device=ht.device)
        dw = torch.empty(wc.shape, dtype=torch.float32, device=ht.device)
        dsc = torch.zeros_like(s32)
        dbi = torch.zeros_like(b32)
        ext.egnn_htype_update_bwd(ht, idx, wc, s32, b32,
                                  g.contiguous().float(), dht, dw, dsc, dbi,
                                  eps)
        return (dht.to(ht.dtype), None, dw.to(w_dtype),
                dsc.view(p_shape).to(p_dtype), dbi.view(p_shape).to(p_dtype),
                None)


def htype_update(ht, idx, w, scale, bias, eps):
    return _HtypeUpdateFn.apply(ht, idx, w, scale, bias, eps)


class _RadialTrunkFn(torch.autograd.Function):
    """Fused RadialFunc trunk (csrc/radial.hip): Linear(D->128) + LN + GELU
    + Linear(128->128) + LN + GELU in one kernel each way. Mirrors the
    autocast-bf16 eager numerics (GEMMs bf16/fp32-acc, LN+GELU fp32)."""

    @staticmethod
    def forward(ctx, x, w0, b0, g0, be0, w3, b3, g3, be3, eps):
        E, D = x.shape
        ctx.x_dtype = x.dtype
        if E == 0:      # nothing to launch: a grid of 0 blocks is an error
            ctx.shapes = [t.shape for t in (x, w0, b0, g0, be0, w3, b3, g3, be3)]
            return torch.empty(0, 128, dtype=torch.bfloat16, device=x.device)
        ext = _load_ext()
        x16 = x.contiguous().to(torch.bfloat16)
        w0_16 = w0.detach().contiguous().to(torch.bfloat16)
        w3_16 = w3.detach().contiguous().to(torch.bfloat16)
        p0 = torch.cat([b0.detach().float(), g0.detach().float(),
                        be0.detach().float()]).contiguous()
        p3 = torch.cat([b3.detach().float(), g3.detach().float(),
                        be3.detach().float()]).contiguous()
        H = torch.empty(E, 128, dtype=torch.bfloat16, device=x.device)
        yh0 = torch.empty_like(H)
        yh3 = torch.empty_like(H)
        rs = torch.empty(2, E, dtype=torch.float32, device=x.device)
        ext.radial_trunk_fwd(x16, w0_16, p0, w3_16, p3, H, yh0, yh3, rs, eps)
        ctx.save_for_backward(x16, w0_16, p0, w3_16, p3, yh0, yh3, rs)
        ctx.eps = eps
        return H

    @staticmethod
    def backward(ctx, dH):
        if dH.shape[0] == 0:
            grads = [torch.zeros(s, dtype=torch.float32, device=dH.device)
                     for s in ctx.shapes]
            return ((grads[0].to(ctx.x_dtype) if ctx.needs_input_grad[0]
                     else None), *grads[1:], None)
        ext = _load_ext()
        x16, w0_16, p0, w3_16, p3, yh0, yh3, rs = ctx.saved_tensors
        E, D = x16.shape
        dev = x16.device
        dH16 = dH.contiguous().to(torch.bfloat16)
        dW0 = torch.zeros(128, D, dtype=torch.float32, device=dev)
        dp0 = torch.zeros(3 * 128, dtype=torch.float32, device=dev)
        dW3 = torch.zeros(128, 128, dtype=torch.float32, device=dev)
        dp3 = torch.zeros(3 * 128, dtype=torch.float32, device=dev)
        need_x = ctx.needs_input_grad[0]
        dX = (torch.zeros(E, D, dtype=torch.float32, device=dev)
              if need_x else torch.empty(0, device=dev))
        w3t = w3_16.t().contiguous()
        ext.radial_trunk_bwd(dH16, x16, w0_16, p0, w3_16, w3t, p3,
                             yh0, yh3, rs, dW0, dp0, dW3, dp3, dX, ctx.eps)
        return ((dX.to(ctx.x_dtype) if need_x else None),
                dW0, dp0[:128], dp0[128:256], dp0[256:],
                dW3, dp3[:128], dp3[128:256], dp3[256:], None)


def radial_trunk(x, w0, b0, g0, be0, w3, b3, g3, be3, eps=1e-5):
    return _RadialTrunkFn.apply(x, w0, b0, g0, be0, w3, b3, g3, be3, eps)


class _ShBasisFn(torch.autograd.Function):
    """Fused SH + basis kernel with its HIP backward (csrc/sh_basis.hip):
    rel (E,3) fp32 -> packed basis (E,TOT) fp32, and dK -> d rel. First order
    only; second-order gradients need the eager path (SE3_EAGER_BASIS=1)."""

    @staticmethod
    def forward(ctx, rel, qcat, normtab, meta, TOT, L):
        out = torch.empty(rel.shape[0], TOT, dtype=torch.float32, device=rel.device)
        _load_ext().sh_basis_fwd(rel, qcat, normtab, meta, out, L)
        ctx.save_for_backward(rel, qcat, normtab, meta)
        ctx.L = L
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dK):
        rel, qcat, normtab, meta = ctx.saved_tensors
        drel = torch.empty_like(rel)
        _load_ext().sh_basis_bwd(rel, qcat, normtab, meta,
                                 dK.contiguous().float(), drel, ctx.L)
        return drel, None, None, None, None, None


def sh_basis(rel, qcat, normtab, meta, TOT, L, differentiable):
    """Packed basis (E, TOT) fp32 of rel (E, 3) fp32. With differentiable
    set, and rel requiring grad, the result carries a first-order autograd
    edge to rel; otherwise it is detached."""
    if differentiable and rel.requires_grad and torch.is_grad_enabled():
        return _ShBasisFn.apply(rel, qcat, normtab, meta, TOT, L)
    out = torch.empty(rel.shape[0], TOT, dtype=torch.float32, device=rel.device)
    _load_ext().sh_basis_fwd(rel.detach(), qcat, normtab, meta, out, L)
    return out
