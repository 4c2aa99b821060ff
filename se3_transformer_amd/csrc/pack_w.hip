// Fused weight-pack kernel: one read of the radial net.6 weight (torch
// Linear layout, (mo*miF, 128), fp32 or bf16) produces BOTH per-lane
// fragment-order packed layouts the pairconv kernels consume:
//
//   P_fwd [mo_p/8][miF_p/32][wm4][mf4][kit4][lane64][j8]   (fwd + bwd_du A-operand)
//   P_dh  [mo_p/8][miF_p/32][wk2][kf4][ns8][lane64][j8]    (bwd_dh B-operand)
//
// mo_p = ceil8(mo) and miF_p = ceil32(miF) (pairconv_common.h): W has its
// true (mo*miF) rows, the packs are sized for the padded dims, and every
// packed row outside the true (mo, miF) is written as exactly zero.
//
// Replaces the per-step host-side chain (W.to(bf16) copy + two
// permute().contiguous() passes in forward and two more in backward =
// ~6% of the round-1 step, r01_final_kernel_stats.csv 'direct_copy' row)
// with a single kernel: W is read once, both outputs written once.
//
// pack_g (below) is the gradient's counterpart: one pass from the autograd
// layout to the o-padded edge-major layout the backward kernels read.
//
// Block = one padded (m, cb) tile: 32 rows (c) x 128 cols (k), rows outside
// the true range staged as zeros, in LDS as
// bf16 with a 16B-slot XOR swizzle so phase-2 reads are conflict-light.

#include <hip/hip_runtime.h>
#include "host_common.h"
#include "ops.h"
#include "pairconv_common.h"

#define NTP 256

template <typename TIN>
__global__ void __launch_bounds__(NTP)
pack_w_kernel(const TIN* __restrict__ W, __bf16* __restrict__ Pf,
              __bf16* __restrict__ Pdh, int mo, int miF) {
    __shared__ __bf16 lds[32 * 128];
    const int nc = (miF + 31) / 32;
    const int m = blockIdx.x / nc, cb = blockIdx.x % nc;   // m < ceil8(mo)
    const int tid = threadIdx.x;

    // phase 1: load + convert the (32 c) x (128 k) tile, coalesced per row
    for (int i = tid; i < 512; i += NTP) {            // 512 vec8 units
        int c32 = i >> 4, k8 = i & 15;
        const TIN* src = W + ((size_t)m * miF + (size_t)cb * 32 + c32) * 128 + k8 * 8;
        // one branch around the whole 8-element run, so the loads stay the
        // two 16 B vector loads they were (a select per element split them
        // into eight guarded dword loads); a pad row stages zeros
        bf16x8 v8(0);
        if (m < mo && cb * 32 + c32 < miF) {
            __bf16 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)(float)src[j];
            v8 = *reinterpret_cast<bf16x8*>(v);
        }
        *reinterpret_cast<bf16x8*>(&lds[c32 * 128 + ((k8 ^ (c32 & 15)) * 8)]) = v8;
    }
    __syncthreads();

    // phase 2a: P_fwd. m = a0*8 + a1*2 + a2; c = cb*32 + a4*16 + a5;
    // k = a6*32 + a7*8 + a8; out dims [a0][cb][a1][a2|a4][a6][a7|a5][a8].
    const int a0 = m >> 3, a1 = (m >> 1) & 3, a2 = m & 1;
    for (int t = tid; t < 512; t += NTP) {
        int a5 = t & 15, a7 = (t >> 4) & 3, a6 = (t >> 6) & 3, a4 = t >> 8;
        int c32 = a4 * 16 + a5;
        int k8 = a6 * 4 + a7;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(
            &lds[c32 * 128 + ((k8 ^ (c32 & 15)) * 8)]);
        size_t off = (((((size_t)a0 * nc + cb) * 4 + a1) * 4 + (a2 * 2 + a4)) * 4 + a6) * 512
                     + (a7 * 16 + a5) * 8;
        *reinterpret_cast<bf16x8*>(Pf + off) = v;
    }

    // phase 2b: P_dh. m = b0*8 + b1; c = cb*32 + b3*8 + b4;
    // k = b5*64 + b6*16 + b7; out dims [b0][cb][b5][b6][b1][b3|b7][b4].
    const int b0 = m >> 3, b1 = m & 7;
    for (int t = tid; t < 512; t += NTP) {
        int b7 = t & 15, b3 = (t >> 4) & 3, b6 = (t >> 6) & 3, b5 = t >> 8;
        int k = b5 * 64 + b6 * 16 + b7;
        int k8 = k >> 3, kj = k & 7;
        __bf16 v[8];
#pragma unroll
        for (int b4 = 0; b4 < 8; ++b4) {
            int c32 = b3 * 8 + b4;
            v[b4] = lds[c32 * 128 + ((k8 ^ (c32 & 15)) * 8) + kj];
        }
        size_t off = (((((size_t)b0 * nc + cb) * 2 + b5) * 4 + b6) * 8 + b1) * 512
                     + (b3 * 16 + b7) * 8;
        *reinterpret_cast<bf16x8*>(Pdh + off) = *reinterpret_cast<bf16x8*>(v);
    }
}

void pack_w_both(torch::Tensor W, torch::Tensor Pf, torch::Tensor Pdh, int64_t mo_) {
    TORCH_CHECK(W.is_cuda() && W.is_contiguous());
    TORCH_CHECK(Pf.is_cuda() && Pf.is_contiguous() && Pf.dtype() == torch::kBFloat16);
    TORCH_CHECK(Pdh.is_cuda() && Pdh.is_contiguous() && Pdh.dtype() == torch::kBFloat16);
    int mo = (int)mo_;
    int64_t N = W.size(0);
    TORCH_CHECK(W.dim() == 2 && W.size(1) == 128, "expect (N, 128) weight");
    TORCH_CHECK(mo >= 1 && N >= mo && N % mo == 0, "rows must split into mo blocks");
    int miF = (int)(N / mo);
    const int64_t mo_p = ceil_mo(mo), miF_p = ceil_mif(miF);
    TORCH_CHECK(Pf.numel() == mo_p * miF_p * 128 && Pdh.numel() == mo_p * miF_p * 128,
                "expect packs sized for (ceil8(mo), ceil32(miF))");
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid(mo_p * (miF_p / 32));
    DISPATCH_F32_BF16(W, __bf16, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(pack_w_kernel<T>), grid, dim3(NTP), 0, stream,
                           tptr<const T>(W), tptr<__bf16>(Pf), tptr<__bf16>(Pdh),
                           mo, miF);
    });
    check_launch("pack_w_both: ");
}

// ---------------------------------------------------------------------------
// pack_g: grad_out (E, mo, O) f32 -> G (mo_p, E, OP) bf16, OP = opad_of(O), pad
// lanes zero, round to nearest even; G may have ceil8(mo) rows, and the rows
// m >= mo are then written as zeros. One (32 e) x (32 mo) tile per block goes
// through LDS so both sides are coalesced: the read follows the mo*O-long
// rows of grad_out, the write stores one (m, e) vector per thread with e on
// the lanes. The odd LDS row length keeps the transposed read conflict-free.
// ---------------------------------------------------------------------------
#define PG_E 32
#define PG_M 32

template <int O>
__global__ void __launch_bounds__(NTP)
pack_g_kernel(const float* __restrict__ grad, __bf16* __restrict__ G,
              int E, int mo, int mo_p) {
    constexpr int OP = opad_of(O);
    constexpr int ROW = PG_M * O + 1;
    __shared__ float tile[PG_E * ROW];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * PG_E, m0 = blockIdx.y * PG_M;
    const int mw = (mo - m0 < PG_M) ? mo - m0 : PG_M;         // true rows, >= 1
    const int mwp = (mo_p - m0 < PG_M) ? mo_p - m0 : PG_M;    // rows written

    for (int t = tid; t < PG_E * PG_M * O; t += NTP) {
        int e = t / (PG_M * O), j = t % (PG_M * O);
        if (e0 + e < E && j < mw * O)
            tile[e * ROW + j] = grad[((size_t)(e0 + e) * mo + m0) * O + j];
    }
    __syncthreads();
    for (int t = tid; t < PG_M * PG_E; t += NTP) {
        int e = t % PG_E, m = t / PG_E;
        if (e0 + e < E && m < mwp) {
            __bf16 v[OP];
#pragma unroll
            for (int o = 0; o < OP; ++o) v[o] = (__bf16)0.f;
            if (m < mw) {        // else a pad row of G: zeros
#pragma unroll
                for (int o = 0; o < O; ++o) v[o] = (__bf16)tile[e * ROW + m * O + o];
            }
            __bf16* dst = G + ((size_t)(m0 + m) * E + e0 + e) * OP;
            if constexpr (OP == 1) dst[0] = v[0];
            else *reinterpret_cast<typename OVec<OP>::type*>(dst) =
                     *reinterpret_cast<typename OVec<OP>::type*>(v);
        }
    }
}

void pack_g(torch::Tensor grad, torch::Tensor G) {
    TORCH_CHECK(grad.is_cuda() && grad.is_contiguous() &&
                grad.dtype() == torch::kFloat32 && grad.dim() == 3);
    int E = grad.size(0), mo = grad.size(1), O = grad.size(2);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(G.is_cuda() && G.is_contiguous() && G.dtype() == torch::kBFloat16 &&
                G.dim() == 3 && (G.size(0) == mo || G.size(0) == ceil_mo(mo)) &&
                G.size(1) == E && G.size(2) == opad_of(O),
                "expect G as (mo or ceil8(mo), E, OP(O))");
    if (E == 0 || mo == 0) return;
    const int mo_p = G.size(0);
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + PG_E - 1) / PG_E, (mo_p + PG_M - 1) / PG_M);
    DISPATCH_ORDER(O, kO, "O", hipLaunchKernelGGL(
        HIP_KERNEL_NAME(pack_g_kernel<kO>), grid, dim3(NTP), 0, stream,
        grad.data_ptr<float>(), tptr<__bf16>(G), E, mo, mo_p));
    check_launch("pack_g: ");
}
