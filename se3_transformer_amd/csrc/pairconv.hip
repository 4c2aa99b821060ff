// Fused pairwise-convolution forward for the SE(3)-Transformer TFN layer.
//
// Reference computation (se3_transformer_pytorch.py:301-343 + :251): per edge e,
//   R[e, mo, mi, f] = radial_net(edge_feats)   (the net.6 GEMM: H[e,:] @ W)
//   K[e] = sum_f R[...,f] * B[...,f]           (per-edge kernel matrix)
//   out  = K[e] @ x_gathered[e]                (matvec)
// materializing R (E x mo*mi*F, ~67 GB at the headline config) and K per edge.
//
// MI355X-native restructure: precontract u[e, (mi,f), o] = sum_i B[e,o,i,f] x[e,mi,i]
// (small), then
//   out[e, mo, o] += sum_{mi,f} (H[e,:] . W[:, (mo,mi,f)]) * u[e, (mi,f), o]
// i.e. a bf16 MFMA GEMM over (edges x radial-output-columns) with the
// (mi,f)->o contraction fused into the epilogue. R never touches HBM.
// The bias term sum_c bias[mo,c] u[e,c,o] is pre-added into `out` by the host.
//
// Layouts:
//   H   (E, 128)      bf16   radial trunk activations (k-contiguous)
//   P   (mo*miF*128)  bf16   net.6 weight packed in MFMA A-fragment order
//                            [mo/8][miF/32][wm4][mf4][kit4][lane64][8]
//   Ut  (miF, O, E)   bf16   basis-contracted features, e-contiguous
//   out (E, mo, O)    f32    pre-initialized with the bias term; kernel adds
//
// Tile: block = 512 threads (8 waves) owns (64 edges) x (8*MB2 mo). The H
// tile is staged to LDS once. The block then loops over miF in chunks of 32:
// the chunk's u tile goes global -> LDS directly (the co-resident block
// covers its latency; a register pipeline for it measured slower), and for
// each of the MB2 mo-sub-blocks in turn an MFMA GEMM of (256 n-rows x 64
// e-cols, K=128), n = 8mo x 32urow, is followed by a VALU contraction
// against u_lds into per-lane accumulators, a cross-lane reduce and an add
// into the LDS partial. Each (e, mo) output is owned by exactly one block:
// no atomics anywhere.

#include <hip/hip_runtime.h>
#include "pairconv_common.h"

#define BLK_E 64
#define BLK_MO 8
#define UCHUNK 32

// MB2 = mo-blocks (of 8) processed per workgroup against ONE staged u chunk.
// MB2=2 halves the u-chunk HBM traffic (u is re-read per mo-block otherwise)
// while keeping 2-blocks/CU residency: the two sub-blocks run serially, so
// the MFMA accumulator registers are reused, only the LDS `part` doubles
// (O=7: 16K h + 32K u + 28K part = 76 KiB <= 80 KiB per block).
// WP = W-fragment software pipeline: the next sub-block's 16 A-fragments
// are prefetched into registers during the current sub-block's epilogue
// (where the MFMA accumulators are dead), so each MFMA phase starts with
// its operands already in flight instead of paying a fresh L2/HBM round
// trip.
template <int O, int MB2, int WP>
__global__ void __launch_bounds__(NT, 4)   // cap VGPR<=128: 2 blocks/CU
pairconv_fwd_kernel(const __bf16* __restrict__ H,
                    const __bf16* __restrict__ P,
                    const __bf16* __restrict__ Ut,
                    float* __restrict__ out,
                    int E, int mo, int miF, int nmemb, int coh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // carve: H tile | u chunk | partial accumulator. The u chunk is stored
    // [urow][e][o] with o PADDED to 8 so the epilogue reads one 16B vector
    // per (urow, e) instead of O scalar ds_read_u16s — the epilogue VALU/LDS
    // issue rate was co-limiting with the MFMA pipe (measured ~240 TF/s vs
    // the ~380 TF/s W-stream roofline).
    __bf16* h_lds = reinterpret_cast<__bf16*>(smem);                       // [64][128] swizzled, 16 KiB
    __bf16* u_lds = reinterpret_cast<__bf16*>(smem + 16384);               // [32][64][8] 32 KiB
    float* part = reinterpret_cast<float*>(smem + 16384 + UCHUNK * BLK_E * 8 * 2); // [64][8*MB2][O]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;          // 0..7
    const int wm = wid >> 1;           // 0..3  (n-rows wm*64 .. +64)
    const int we = wid & 1;            // 0..1  (e-cols we*32 .. +32)
    const int l15 = lane & 15;
    const int l4 = lane >> 4;          // 0..3

    int eb, mb;                        // the cohort shares an mo-block group
    cohort_map(coh, nmemb, eb, mb);
    const int e0 = eb * BLK_E;
    const int mo0 = mb * BLK_MO * MB2;

    stage_h_tile(h_lds, H, e0, E, tid);
    // zero partial accumulator + the u pad lanes (o in [O, 8) are never
    // overwritten by staging, so one upfront clear keeps them zero)
    for (int i = tid; i < BLK_E * BLK_MO * MB2 * O; i += NT) part[i] = 0.f;
    for (int i = tid; i < UCHUNK * BLK_E * 8 / 8; i += NT)
        *reinterpret_cast<bf16x8*>(u_lds + (size_t)i * 8) = bf16x8(0);

    constexpr int UTOT = (UCHUNK * O * BLK_E) / 8;   // u chunk in 16B units
    const int nchunks = miF / UCHUNK;
    auto pb_of = [&](int cc, int ss) {
        return P + ((((size_t)(mb * MB2 + ss) * (miF / 32) + cc) * 4 + wm) * 4) * 4 * 64 * 8
               + (size_t)lane * 8;
    };
    // W-pipeline state: the 16 A-fragments of the NEXT (chunk, sub) pair
    bf16x8 a_pre[WP ? 16 : 1];
    if (WP) {
#pragma unroll
        for (int f = 0; f < 16; ++f) a_pre[f] = load_wfrag(pb_of(0, 0), f);
    }
    __syncthreads();

    for (int c = 0; c < nchunks; ++c) {
        // ---- stage the u chunk, scattered to [urow][e][o(pad 8)]
        for (int i = tid; i < UTOT; i += NT) {
            int ro = i >> 3;            // (urow*O + o)
            int eu = (i & 7) * 8;       // e offset within 64
            const int ur = ro / O, o = ro % O;
            bf16x8 v = load_edges8(Ut + ((size_t)(c * UCHUNK + ur) * O + o) * E, e0 + eu, E);
            commit_opad(u_lds, ur, eu, o, v);
        }
        __syncthreads();

        // ---- per mo-sub-block: GEMM + epilogue against the SAME u chunk.
        // Unrolled, but a sched_barrier between the sub-blocks keeps the
        // second sub-block's W-fragment loads from being hoisted into the
        // first (which would double the live A-operand registers and spill).
#pragma unroll
        for (int sub = 0; sub < MB2; ++sub) {
        if (MB2 > 1 && sub > 0) __builtin_amdgcn_sched_barrier(0);
        // ---- GEMM: R^T tile (256 n x 64 e), K=128
        f32x4 acc[4][2];
        const __bf16* pbase = pb_of(c, sub);
        mfma_rtile(acc, h_lds, we, l15, l4, [&](int mf, int kit) {
            return WP ? a_pre[mf * 4 + kit] : load_wfrag(pbase, mf * 4 + kit);
        });
        if (WP) {
            // prefetch the NEXT sub-block/chunk's fragments now — their
            // L2/HBM latency hides under the epilogue below (acc is the
            // only other register consumer left, and it dies there)
            int ns = sub + 1, nc2 = c;
            if (ns == MB2) { ns = 0; ++nc2; }
            if (nc2 == nchunks) { ns = sub; nc2 = c; }   // tail: benign refetch
            const __bf16* pn = pb_of(nc2, ns);
#pragma unroll
            for (int f = 0; f < 16; ++f) a_pre[f] = load_wfrag(pn, f);
        }

        // ---- epilogue: contract acc against u_lds into s[ef][moi][o-pair].
        // One ds_read_b128 per (row, e) covers all 8 padded o; the o-pair
        // float2 accumulation maps onto v_pk_fma_f32.
        f32x2 s[2][2][4];
#pragma unroll
        for (int ef = 0; ef < 2; ++ef)
#pragma unroll
            for (int mi_ = 0; mi_ < 2; ++mi_)
#pragma unroll
                for (int p_ = 0; p_ < 4; ++p_) s[ef][mi_][p_] = f32x2{0.f, 0.f};

#pragma unroll
        for (int mf = 0; mf < 2; ++mf) {   // mf and mf+2 share urow (rows r, r+32)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = wm * 64 + mf * 16 + l4 * 4 + reg;
                const int urow = r & 31;
#pragma unroll
                for (int ef = 0; ef < 2; ++ef) {
                    const int e = we * 32 + ef * 16 + l15;
                    const float rv0 = acc[mf][ef][reg];
                    const float rv1 = acc[mf + 2][ef][reg];
                    bf16x8 uv8 = *reinterpret_cast<const bf16x8*>(
                        u_lds + ((size_t)urow * BLK_E + e) * 8);
#pragma unroll
                    for (int p_ = 0; p_ < 4; ++p_) {
                        f32x2 u2 = {(float)uv8[2 * p_], (float)uv8[2 * p_ + 1]};
                        s[ef][0][p_] += rv0 * u2;
                        s[ef][1][p_] += rv1 * u2;
                    }
                }
            }
        }

        // cross-lane reduce over l4 groups (rows), then accumulate into LDS partial
#pragma unroll
        for (int ef = 0; ef < 2; ++ef)
#pragma unroll
            for (int mi_ = 0; mi_ < 2; ++mi_)
#pragma unroll
                for (int p_ = 0; p_ < 4; ++p_) {
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) {
                        if (2 * p_ + c2 >= O) break;
                        float v = s[ef][mi_][p_][c2];
                        v += __shfl_xor(v, 16);
                        v += __shfl_xor(v, 32);
                        s[ef][mi_][p_][c2] = v;
                    }
                }
        if (l4 == 0) {
#pragma unroll
            for (int ef = 0; ef < 2; ++ef) {
                const int e = we * 32 + ef * 16 + l15;
#pragma unroll
                for (int mi_ = 0; mi_ < 2; ++mi_) {
                    const int moi = sub * BLK_MO + wm * 2 + mi_;
#pragma unroll
                    for (int o = 0; o < O; ++o) {
                        float* p = part + ((size_t)e * (BLK_MO * MB2) + moi) * O + o;
                        *p += s[ef][mi_][o >> 1][o & 1];
                    }
                }
            }
        }
        }   // sub
        __syncthreads();
    }

    // ---- write out: out[e0+e][mo0+moi][o] += partial
    for (int i = tid; i < BLK_E * BLK_MO * MB2 * O; i += NT) {
        int o = i % O;
        int moi = (i / O) % (BLK_MO * MB2);
        int e = i / (O * BLK_MO * MB2);
        if (e0 + e < E) {
            float* p = out + ((size_t)(e0 + e) * mo + mo0 + moi) * O + o;
            *p += part[((size_t)e * (BLK_MO * MB2) + moi) * O + o];
        }
    }
}

// One kernel per (O, MB2); both choices are functions of the shape alone
// (measurements in profiles/LADDER.md):
//   MB2 = 2 wherever mo allows it — sharing a staged u chunk between two
//         mo-blocks halves the u traffic.
//   WP on at O=3,5 (+7% at O=5); at O=7 the held prefetch registers spill
//         the epilogue (108 B/lane, -9%); O=1 has only been run without it.
template <int O, int MB2>
static void launch_fwd(const torch::Tensor& H, const torch::Tensor& P,
                       const torch::Tensor& Ut, torch::Tensor& out,
                       int E, int mo, int miF) {
    constexpr int WP = (O == 3 || O == 5) ? 1 : 0;
    int nmemb = (E + BLK_E - 1) / BLK_E;
    int ng = mo / (BLK_MO * MB2);
    int coh = (ng % 8 == 0) ? 1 : 0;
    size_t lds = 16384 + (size_t)UCHUNK * BLK_E * 8 * 2
                 + (size_t)BLK_E * BLK_MO * MB2 * O * 4;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pairconv_fwd_kernel<O, MB2, WP>),
                       dim3(nmemb * ng), dim3(NT), lds,
                       at::cuda::getCurrentHIPStream(),
                       reinterpret_cast<const __bf16*>(H.data_ptr()),
                       reinterpret_cast<const __bf16*>(P.data_ptr()),
                       reinterpret_cast<const __bf16*>(Ut.data_ptr()),
                       out.data_ptr<float>(), E, mo, miF, nmemb, coh);
}

void pairconv_fwd(torch::Tensor H, torch::Tensor W, torch::Tensor Ut,
                  torch::Tensor out, int64_t mo_) {
    TORCH_CHECK(H.is_cuda() && W.is_cuda() && Ut.is_cuda() && out.is_cuda());
    TORCH_CHECK(H.dtype() == torch::kBFloat16 && W.dtype() == torch::kBFloat16 &&
                Ut.dtype() == torch::kBFloat16 && out.dtype() == torch::kFloat32);
    TORCH_CHECK(H.is_contiguous() && W.is_contiguous() && Ut.is_contiguous() &&
                out.is_contiguous());
    int E = H.size(0);
    int mo = (int)mo_;
    int miF = Ut.size(0);
    int O = Ut.size(1);
    TORCH_CHECK(H.size(1) == KDIM, "radial hidden dim must be 128");
    TORCH_CHECK(W.numel() == (int64_t)mo * miF * KDIM, "expect packed W");
    TORCH_CHECK(Ut.size(2) == E);
    TORCH_CHECK(out.size(0) == E && out.size(1) == mo && out.size(2) == O);
    TORCH_CHECK(miF % UCHUNK == 0, "miF must be a multiple of 32");
    TORCH_CHECK(mo % BLK_MO == 0, "mo must be a multiple of 8");
    DISPATCH_O(O, {
        if (mo % (BLK_MO * 2) == 0) launch_fwd<kO, 2>(H, W, Ut, out, E, mo, miF);
        else launch_fwd<kO, 1>(H, W, Ut, out, E, mo, miF);
    });
    hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "pairconv_fwd launch failed: ", hipGetErrorString(err));
}

void sh_basis_fwd(torch::Tensor rel, torch::Tensor qcat, torch::Tensor normtab,
                  torch::Tensor meta, torch::Tensor out, int64_t L);
void knn_graph(torch::Tensor coors, torch::Tensor nmask, torch::Tensor allow,
               torch::Tensor sparse, torch::Tensor idx,
               torch::Tensor dist, torch::Tensor rel, torch::Tensor m,
               int64_t k, double radius, bool causal);
int64_t knn_max_lds_bytes();
void attn2_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
               torch::Tensor mask, torch::Tensor qf, torch::Tensor kf,
               torch::Tensor out, torch::Tensor lse,
               int64_t n, int64_t heads, double scale, bool kv_one,
               int64_t jr, int64_t rot);
void attn2_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
               torch::Tensor mask, torch::Tensor qf, torch::Tensor kf,
               torch::Tensor out, torch::Tensor lse, torch::Tensor g,
               torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
               int64_t n, int64_t heads, double scale, bool kv_one,
               int64_t jr, int64_t rot);
void norm_se3_nl_fwd(torch::Tensor t, torch::Tensor scale, torch::Tensor out,
                     double eps, int64_t nonlin);
void norm_se3_nl_bwd(torch::Tensor t, torch::Tensor scale, torch::Tensor dout,
                     torch::Tensor dt, torch::Tensor dscale, double eps,
                     int64_t nonlin);
int64_t norm_se3_gated_max_c();
void norm_se3_gated_fwd(torch::Tensor t, torch::Tensor W, torch::Tensor out,
                        torch::Tensor gate, double eps, int64_t nonlin);
void norm_se3_gated_bwd(torch::Tensor t, torch::Tensor Wt, torch::Tensor gate,
                        torch::Tensor dout, torch::Tensor dt,
                        torch::Tensor dgate, torch::Tensor nu, double eps,
                        int64_t nonlin);
void pairconv_bwd_dh(torch::Tensor G, torch::Tensor Ut, torch::Tensor Wt,
                     torch::Tensor dH, int64_t mo_);
void pairconv_bwd_dw(torch::Tensor G, torch::Tensor Ut, torch::Tensor Ht,
                     torch::Tensor dW, int64_t mo_);
void pairconv_bwd_du(torch::Tensor H, torch::Tensor W, torch::Tensor bias,
                     torch::Tensor G, torch::Tensor dU, int64_t mo_);
void pack_w_both(torch::Tensor W, torch::Tensor Pf, torch::Tensor Pdh, int64_t mo_);
void ubuild_fwd(torch::Tensor B, torch::Tensor X, torch::Tensor Ut,
                int64_t O, int64_t I, int64_t F);
void ubuild_bwd_dx(torch::Tensor B, torch::Tensor dU, torch::Tensor dX,
                   int64_t O, int64_t I, int64_t F);
void ubuild_bwd_db(torch::Tensor X, torch::Tensor dU, torch::Tensor dB,
                   int64_t O, int64_t I, int64_t F);
void sh_basis_bwd(torch::Tensor rel, torch::Tensor qcat, torch::Tensor normtab,
                  torch::Tensor meta, torch::Tensor dK, torch::Tensor drel,
                  int64_t L);
void egnn_rel_dist_fwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor dist);
void egnn_rel_dist_bwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor gdist,
                       torch::Tensor dht);
void egnn_htype_update_fwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor w,
                           torch::Tensor sc, torch::Tensor bi,
                           torch::Tensor upd, double eps);
void egnn_htype_update_bwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor w,
                           torch::Tensor sc, torch::Tensor bi, torch::Tensor g,
                           torch::Tensor dht, torch::Tensor dw,
                           torch::Tensor dsc, torch::Tensor dbi, double eps);
void radial_trunk_fwd(torch::Tensor X, torch::Tensor W0, torch::Tensor p0,
                      torch::Tensor W3, torch::Tensor p3,
                      torch::Tensor H, torch::Tensor yh0, torch::Tensor yh3,
                      torch::Tensor rs01, double eps);
void radial_trunk_bwd(torch::Tensor dH, torch::Tensor X, torch::Tensor W0,
                      torch::Tensor p0, torch::Tensor W3, torch::Tensor W3t,
                      torch::Tensor p3, torch::Tensor yh0, torch::Tensor yh3,
                      torch::Tensor rs01, torch::Tensor dW0, torch::Tensor dp0,
                      torch::Tensor dW3, torch::Tensor dp3, torch::Tensor dX,
                      double eps);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("pairconv_fwd", &pairconv_fwd,
          "fused radial-GEMM + basis contraction forward (MI355X)");
    m.def("pairconv_bwd_dh", &pairconv_bwd_dh, "dH backward");
    m.def("pairconv_bwd_dw", &pairconv_bwd_dw, "dW backward");
    m.def("pairconv_bwd_du", &pairconv_bwd_du, "dU backward");
    m.def("knn_graph", &knn_graph, "on-device kNN graph build");
    m.def("knn_max_lds_bytes", &knn_max_lds_bytes,
          "dynamic-LDS ceiling of the kNN kernel (bounds n and k)");
    m.def("attn2_fwd", &attn2_fwd,
          "fused neighbor attention fwd (online softmax, in-kernel rotary)");
    m.def("attn2_bwd", &attn2_bwd, "fused neighbor attention backward");
    m.def("norm_se3_nl_fwd", &norm_se3_nl_fwd,
          "fused NormSE3 forward, nonlin 0 = GELU, 1 = identity");
    m.def("norm_se3_nl_bwd", &norm_se3_nl_bwd,
          "fused NormSE3 backward, nonlin 0 = GELU, 1 = identity");
    m.def("norm_se3_gated_max_c", &norm_se3_gated_max_c,
          "channel ceiling of the gated-scale NormSE3 kernels");
    m.def("norm_se3_gated_fwd", &norm_se3_gated_fwd,
          "fused gated-scale NormSE3 forward (also writes gate)");
    m.def("norm_se3_gated_bwd", &norm_se3_gated_bwd,
          "fused gated-scale NormSE3 backward (dt; dgate and nu for dW)");
    m.def("sh_basis_fwd", &sh_basis_fwd,
          "fused spherical-harmonics + equivariant basis (MI355X)");
    m.def("pack_w_both", &pack_w_both,
          "one-pass pack of net.6 W into both MFMA fragment layouts");
    m.def("radial_trunk_fwd", &radial_trunk_fwd,
          "fused radial trunk (Linear-LN-GELU x2) forward");
    m.def("radial_trunk_bwd", &radial_trunk_bwd,
          "fused radial trunk backward");
    m.def("ubuild_fwd", &ubuild_fwd,
          "basis x features precontraction (e-contiguous out)");
    m.def("ubuild_bwd_dx", &ubuild_bwd_dx, "ubuild dX backward");
    m.def("ubuild_bwd_db", &ubuild_bwd_db,
          "ubuild dB backward (differentiable coordinates)");
    m.def("sh_basis_bwd", &sh_basis_bwd,
          "fused spherical-harmonics + basis backward: dK -> d rel");
    m.def("egnn_rel_dist_fwd", &egnn_rel_dist_fwd,
          "EGNN neighbor rel-htype distances (no n^2 intermediate)");
    m.def("egnn_rel_dist_bwd", &egnn_rel_dist_bwd, "its backward");
    m.def("egnn_htype_update_fwd", &egnn_htype_update_fwd,
          "EGNN htype norm+weighted neighbor sum (no n^2 intermediate)");
    m.def("egnn_htype_update_bwd", &egnn_htype_update_bwd, "its backward");
}
