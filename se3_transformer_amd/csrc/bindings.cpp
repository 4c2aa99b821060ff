// The Python module of the extension: one line per declaration in ops.h.
#include "ops.h"

#define OP(f, doc) m.def(#f, &f, doc)

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    OP(pairconv_fwd_opad, "fused radial-GEMM + basis contraction forward, U (ceil32(miF), E, OP), out (E, mo, O)");
    OP(pairconv_opad, "padded o width OP(O)");
    OP(pack_g, "grad_out (E, mo, O) f32 -> G (mo or ceil8(mo), E, OP) bf16, zero pads");
    OP(pairconv_bwd_dh, "dH backward");
    OP(pairconv_bwd_dw, "dW backward; also fills db (mo*miF,) f32 unless db is empty; a 3-D dW names the true (mo, miF)");
    OP(pairconv_bwd_du, "dU backward, dU (miF, E, OP) bf16 or f32");
    OP(knn_graph, "on-device kNN graph build");
    OP(knn_max_lds_bytes, "dynamic-LDS ceiling of the kNN kernel (bounds n and k)");
    OP(attn2_fwd, "fused neighbor attention fwd (online softmax, in-kernel rotary)");
    OP(attn2_bwd, "fused neighbor attention backward");
    OP(norm_se3_nl_fwd, "fused NormSE3 forward, nonlin 0 = GELU, 1 = identity");
    OP(norm_se3_nl_bwd, "fused NormSE3 backward, nonlin 0 = GELU, 1 = identity");
    OP(norm_se3_gated_max_c, "channel ceiling of the gated-scale NormSE3 kernels");
    OP(norm_se3_gated_fwd, "fused gated-scale NormSE3 forward (also writes gate)");
    OP(norm_se3_gated_bwd, "fused gated-scale NormSE3 backward (dt; dgate and nu for dW)");
    OP(sh_basis_fwd, "fused spherical-harmonics + equivariant basis (MI355X)");
    OP(sh_basis_bwd, "fused spherical-harmonics + basis backward: dK -> d rel");
    OP(pack_w_both, "one-pass pack of net.6 W into both MFMA fragment layouts, zero-padded to (ceil8(mo), ceil32(miF))");
    OP(radial_trunk_fwd, "fused radial trunk (Linear-LN-GELU x2) forward");
    OP(radial_trunk_bwd, "fused radial trunk backward");
    OP(ubuild_fwd, "basis x features precontraction, out (C*F or ceil32(C*F), E, OP)");
    OP(ubuild_bwd_dx, "ubuild dX backward");
    OP(ubuild_bwd_db, "ubuild dB backward (differentiable coordinates)");
    OP(ubuild_gather_fwd, "ubuild_fwd on node features: X[e] = Xn[rows[e]]");
    OP(ubuild_gather_bwd_dx, "its dXn backward: fp32 atomic adds into (N, C, I)");
    OP(ubuild_gather_bwd_db, "ubuild_bwd_db on node features");
    OP(egnn_rel_dist_fwd, "EGNN neighbor rel-htype distances (no n^2 intermediate)");
    OP(egnn_rel_dist_bwd, "its backward");
    OP(egnn_htype_update_fwd, "EGNN htype norm+weighted neighbor sum (no n^2 intermediate)");
    OP(egnn_htype_update_bwd, "its backward");
}
