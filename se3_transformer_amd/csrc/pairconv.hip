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
//   P   (mo_p*miF_p*128) bf16 net.6 weight packed in MFMA A-fragment order
//                            [mo_p/8][miF_p/32][wm4][mf4][kit4][lane64][8],
//                            rows outside the true (mo, miF) zero
//   U   (miF_p, E, OP) bf16  basis-contracted features, edge-major with o
//                            padded to OP(O) (pairconv_common.h), pads zero,
//                            rows >= miF zero
//   out (E, mo, O)    f32    pre-initialized with the bias term; kernel adds.
//                            mo is the true width: the write-out skips the
//                            rows mo..mo_p of the last mo-block
//
// Tile: block = 512 threads (8 waves) owns (64 edges) x (8*MB2 mo). The H
// tile is staged to LDS once. The block then loops over miF in chunks of 32:
// the chunk's u tile goes global -> LDS as a straight vector copy (the
// co-resident block covers its latency; a register pipeline for it measured
// slower), and for
// each of the MB2 mo-sub-blocks in turn an MFMA GEMM of (256 n-rows x 64
// e-cols, K=128), n = 8mo x 32urow, is followed by a VALU contraction
// against u_lds into per-lane accumulators, a cross-lane reduce and an add
// into the LDS partial. Each (e, mo) output is owned by exactly one block:
// no atomics anywhere.

#include <hip/hip_runtime.h>
#include "pairconv_common.h"
#include "ops.h"

#define BLK_E 64
#define BLK_MO 8
#define UCHUNK 32

// MB2 = mo-blocks (of 8) processed per workgroup against ONE staged u chunk.
// MB2=2 halves the u-chunk HBM traffic (u is re-read per mo-block otherwise)
// while keeping 2-blocks/CU residency: the two sub-blocks run serially, so
// the MFMA accumulator registers are reused, only the LDS `part` doubles
// (O=7: 16K h + 32K u + 28K part = 76 KiB <= 80 KiB per block).
// LP = o width of the LDS u tile: OP(O), except that O=1 keeps its scatter
// into 8-wide slots (its global layout has no vectors to copy).
template <int O> struct FwdLP { static constexpr int v = (O == 1) ? 8 : opad_of(O); };

// WP = W-fragment software pipeline: the next sub-block's 16 A-fragments
// are prefetched into registers during the current sub-block's epilogue
// (where the MFMA accumulators are dead), so each MFMA phase starts with
// its operands already in flight instead of paying a fresh L2/HBM round
// trip.
template <int O, int MB2, int WP, int UNR>
__global__ void __launch_bounds__(NT, 4)   // cap VGPR<=128: 2 blocks/CU
pairconv_fwd_kernel(const __bf16* __restrict__ H,
                    const __bf16* __restrict__ P,
                    const __bf16* __restrict__ Ut,   // (miF, E, OP)
                    float* __restrict__ out,
                    int E, int mo /* out's, true */, int miF /* padded */,
                    int nmemb, int coh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // carve: H tile | u chunk | partial accumulator. The u chunk is stored
    // [urow][e][o] with o PADDED to LP, as it is in memory, so the epilogue
    // reads one vector per (urow, e) instead of O scalar ds_read_u16s — the
    // epilogue VALU/LDS issue rate was co-limiting with the MFMA pipe
    // (measured ~240 TF/s vs the ~380 TF/s W-stream roofline).
    constexpr int LP = FwdLP<O>::v;
    typedef typename OVec<LP>::type uvec;
    __bf16* h_lds = reinterpret_cast<__bf16*>(smem);                       // [64][128] swizzled, 16 KiB
    __bf16* u_lds = reinterpret_cast<__bf16*>(smem + 16384);               // [32][64][LP] <= 32 KiB
    float* part = reinterpret_cast<float*>(smem + 16384 + UCHUNK * BLK_E * LP * 2); // [64][8*MB2][O]

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
    for (int i = tid; i < BLK_E * BLK_MO * MB2 * O; i += NT) part[i] = 0.f;
    if constexpr (O == 1) {   // pad lanes of the scatter slots, cleared once
        for (int i = tid; i < UCHUNK * BLK_E * 8 / 8; i += NT)
            *reinterpret_cast<bf16x8*>(u_lds + (size_t)i * 8) = bf16x8(0);
    }

    constexpr int UTOT = (UCHUNK * O * BLK_E) / 8;   // O=1: u chunk in 16B units
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
        // ---- stage the u chunk [urow][e][LP]: one vector per (urow, e),
        // rows past E zero-filled
        if constexpr (O == 1) {
            for (int i = tid; i < UTOT; i += NT) {
                int ur = i >> 3;            // urow
                int eu = (i & 7) * 8;       // e offset within 64
                bf16x8 v = load_edges8(Ut + (size_t)(c * UCHUNK + ur) * E, e0 + eu, E);
                commit_opad(u_lds, ur, eu, 0, v);
            }
        } else {
            // 16 B units: one edge at LP=8, two at LP=4 (whose rows are
            // only 8 B aligned when E is odd: the load is declared so).
            // A wave covers RPW whole urows per pass, so the row base is
            // wave-uniform (scalar registers) and only the offset inside
            // the wave's rows is per lane. At LP=8 the wave's row is read
            // through a buffer resource that ends at the last valid edge
            // of the block: lanes past E read zeros by the range check, and
            // the load needs neither a 64-bit per-lane address nor a
            // predicate. The MFMA and epilogue phases have no vector
            // register to spare for either.
            constexpr int EPU = 8 / LP;             // edges per unit
            constexpr int UPR = BLK_E / EPU;        // units per urow
            constexpr int RPW = 64 / UPR;           // urows per wave per pass
            constexpr int RPK = NT / UPR;           // urows per pass of the block
            const int swid = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int eu = (lane % UPR) * EPU;
            const unsigned u_off = ((unsigned)(lane / UPR) * E + eu) * LP * 2;
            const char* ub = reinterpret_cast<const char*>(
                Ut + ((size_t)(c * UCHUNK + swid * RPW) * E + e0) * LP);
#pragma unroll(UNR)
            for (int k = 0; k < UCHUNK / RPK; ++k) {
                const char* src = ub + (size_t)k * RPK * E * LP * 2 + u_off;
                bf16x8 v(0);
                if constexpr (LP == 8) {
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    const int left = E - e0;        // > 0: the block exists
                    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<char*>(ub + (size_t)k * RPK * E * LP * 2), 0,
                        (left < BLK_E ? left : BLK_E) * 16, 0x00020000);
                    v = __builtin_bit_cast(
                        bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)u_off, 0, 0));
                } else if (e0 + eu + EPU <= E) {
                    v = *reinterpret_cast<const bf16x8_a8*>(src);
                } else if (EPU == 2 && e0 + eu < E) {   // last edge of an odd E
                    bf16x4 lo = *reinterpret_cast<const bf16x4*>(src);
                    v = bf16x8{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
                }
                *reinterpret_cast<bf16x8*>(u_lds + ((size_t)k * NT + tid) * 8) = v;
            }
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
        // One vector read per (row, e) covers all padded o; the o-pair
        // float2 accumulation maps onto v_pk_fma_f32.
        f32x2 s[2][2][LP / 2];
#pragma unroll
        for (int ef = 0; ef < 2; ++ef)
#pragma unroll
            for (int mi_ = 0; mi_ < 2; ++mi_)
#pragma unroll
                for (int p_ = 0; p_ < LP / 2; ++p_) s[ef][mi_][p_] = f32x2{0.f, 0.f};

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
                    uvec uv8 = *reinterpret_cast<const uvec*>(
                        u_lds + ((size_t)urow * BLK_E + e) * LP);
#pragma unroll
                    for (int p_ = 0; p_ < LP / 2; ++p_) {
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
                for (int p_ = 0; p_ < LP / 2; ++p_) {
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
        if (e0 + e < E && mo0 + moi < mo) {
            float* p = out + ((size_t)(e0 + e) * mo + mo0 + moi) * O + o;
            *p += part[((size_t)e * (BLK_MO * MB2) + moi) * O + o];
        }
    }
}

// One kernel per (O, MB2); both choices are functions of the shape alone
// (measurements in profiles/LADDER.md):
//   MB2 = 2 wherever mo allows it — sharing a staged u chunk between two
//         mo-blocks halves the u traffic.
//   WP on at O=5 (+7%, and +4% re-measured on the padded layout); at O=7
//         the held prefetch registers spill the epilogue (108 B/lane, -9%);
//         at O=3 the OP=4 epilogue is short enough that the prefetch only
//         adds spills (84 B/lane) and loses 11%; O=1 has only been run
//         without it.
//   UNR = u-staging loads in flight per thread. One at a time at OP=8
//         (2 and 4 tie or lose and add scratch); both of its two at OP=4,
//         where the MFMA phases are shortest and the exposed latency shows
//         (4.13 -> 3.96 ms at (1,1)). profiles/opad_layout.md.
template <int O, int MB2>
static void launch_fwd(const torch::Tensor& H, const torch::Tensor& P,
                       const torch::Tensor& Ut, torch::Tensor& out,
                       int E, int mo, int mo_p, int miF) {
    constexpr int WP = (O == 5) ? 1 : 0;
    constexpr int UNR = (O == 3) ? 2 : 1;
    int nmemb = (E + BLK_E - 1) / BLK_E;
    int ng = mo_p / (BLK_MO * MB2);
    int coh = (ng % 8 == 0) ? 1 : 0;
    size_t lds = 16384 + (size_t)UCHUNK * BLK_E * FwdLP<O>::v * 2
                 + (size_t)BLK_E * BLK_MO * MB2 * O * 4;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pairconv_fwd_kernel<O, MB2, WP, UNR>),
                       dim3(nmemb * ng), dim3(NT), lds,
                       at::cuda::getCurrentHIPStream(),
                       tptr<const __bf16>(H), tptr<const __bf16>(P),
                       tptr<const __bf16>(Ut),
                       out.data_ptr<float>(), E, mo, miF, nmemb, coh);
}

int64_t pairconv_opad(int64_t O) { return opad_of((int)O); }

// U is (miF_p, E, OP(O)) with zero pads; O is out's last dim. mo_ is the
// padded mo_p of the packed W; out has the true mo in (mo_p - 8, mo_p].
void pairconv_fwd_opad(torch::Tensor H, torch::Tensor W, torch::Tensor Ut,
                       torch::Tensor out, int64_t mo_) {
    TORCH_CHECK(H.is_cuda() && W.is_cuda() && Ut.is_cuda() && out.is_cuda());
    TORCH_CHECK(H.dtype() == torch::kBFloat16 && W.dtype() == torch::kBFloat16 &&
                Ut.dtype() == torch::kBFloat16 && out.dtype() == torch::kFloat32);
    TORCH_CHECK(H.is_contiguous() && W.is_contiguous() && Ut.is_contiguous() &&
                out.is_contiguous());
    TORCH_CHECK(Ut.dim() == 3 && out.dim() == 3);
    int E = H.size(0);
    int mo_p = (int)mo_;
    int mo = out.size(1);
    int miF = Ut.size(0);
    int O = out.size(2);
    TORCH_CHECK(H.size(1) == KDIM, "radial hidden dim must be 128");
    TORCH_CHECK(W.numel() == (int64_t)mo_p * miF * KDIM, "expect packed W");
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(Ut.size(1) == E && Ut.size(2) == opad_of(O),
                "expect U as (miF, E, OP(O))");
    TORCH_CHECK(miF >= UCHUNK && miF % UCHUNK == 0,
                "U must have ceil32(miF) rows (pad rows zero)");
    TORCH_CHECK(mo_p >= BLK_MO && mo_p % BLK_MO == 0,
                "mo_ must be the padded ceil8(mo)");
    TORCH_CHECK(out.size(0) == E && mo >= 1 && ceil_mo(mo) == mo_p,
                "expect out as (E, mo, O) with ceil8(mo) == mo_");
    DISPATCH_ORDER(O, kO, "O", {
        if (mo_p % (BLK_MO * 2) == 0) launch_fwd<kO, 2>(H, W, Ut, out, E, mo, mo_p, miF);
        else launch_fwd<kO, 1>(H, W, Ut, out, E, mo, mo_p, miF);
    });
    check_launch("pairconv_fwd launch failed: ");
}
