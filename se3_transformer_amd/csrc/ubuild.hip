// Basis-feature precontraction ("u build") for the fused pairwise conv:
//
//   U[(c*F + f), e, o] = sum_i  B[e, o, i, f] * X[e, c, i]
//
// U is (C*F, E, OP): edge-major with o padded to OP = opad_of(O)
// (pairconv_common.h), pad lanes written as zeros. Any C >= 1: the last
// channel chunk is guarded. Handed a U with ceil32(C*F) rows, the forward
// writes the rows [C*F, ceil32(C*F)) as zeros (the pad rows of the pairconv
// layout contract), and the backward kernels read the first C*F rows of a dU
// padded likewise. The ubuild_gather_* kernels take C % 32 == 0 only.
// dU has the same shape, in
// bf16 as pairconv_bwd_du rounds it or in f32; the backward kernels widen it
// into the f32 LDS tile they compute on, so both give the same bits.
//
// This is the `torch.einsum('eoif,eci->cfeo')` in PairwiseConv.apply_fused
// (reference contraction se3_transformer_pytorch.py:336-338 restructured,
// see models/core.py) — in eager torch it lowers to permute-copies + bmm +
// an output copy (the largest non-custom slice of the round-1/2 kernel
// stats). Here: one pass, B staged once per edge tile in LDS (it is re-used
// by all C channels), output written directly in the padded layout the
// pairconv kernels consume: the thread that owns a (row, e) computes all its
// o and writes the whole vector, pads included.
//
// Backward:
//   dX[e, c, i]    = sum_{f,o} B[e,o,i,f] * dU[(c*F+f), e, o]   (always)
//   dB[e, o, i, f] = sum_c     X[e,c,i]   * dU[(c*F+f), e, o]   (only when the
// basis requires grad, i.e. differentiable_coors). dB is a sibling kernel
// rather than a second output of the dX kernel: the dX kernel's LDS already
// holds B and a dU tile, and adding the fp32 dB tile would pass 64 KiB for
// the (7,7,7) pair. The price is one extra read of dU on that path only.
//
// The ubuild_gather_* entry points take x per NODE, Xn (N, C, I), and the
// row of every edge, rows (E,) int32: X[e] = Xn[rows[e]] without the gathered
// (E, C, I) tensor. Forward and dB are the kernels above with an indexed
// staging load (same bits). dXn (N, C, I) fp32 is summed over the edges of a
// row with atomicAdd: the backward of the gather, and the sum over the pairs
// that share a d_in when they accumulate into one buffer. An edge whose row
// is outside [0, N) reads x as zero and adds nothing.

#include <hip/hip_runtime.h>
#include "host_common.h"
#include "ops.h"
#include "pairconv_common.h"

#define UB_NT 256
#define UB_E 32          // edges per block (fwd)
#define UB_C 32          // channel chunk (fwd)
#define UB_EB 16         // edges per block (bwd)
#define UB_CB 8          // channel chunk (bwd)

typedef __attribute__((ext_vector_type(2))) __bf16 ub_bf16x2;

// Row of X that holds edge e's features: e itself, or rows[e] of the
// N-row node tensor. -1 past the last edge (and for a row outside [0, N)).
template <bool GATHER>
__device__ __forceinline__ long ub_x_row(const int* __restrict__ rows, int e,
                                         int E, int N) {
    if (e >= E) return -1;
    if constexpr (!GATHER) return e;
    else {
        int r = rows[e];
        return ((unsigned)r < (unsigned)N) ? r : -1;
    }
}

template <typename TX, int OP, bool GATHER>
__device__ __forceinline__ void
ubuild_fwd_body(const float* __restrict__ B,   // (E, O, I, F)
                const TX* __restrict__ X,      // (E, C, I) | (N, C, I)
                const int* __restrict__ rows,  // (E,) when GATHER
                __bf16* __restrict__ Ut,       // (urows, E, OP), urows >= C*F
                int E, int N, int C, int O, int I, int F, int urows) {
    // b and x tiles are stored [.., i PADDED to 8] bf16 so each output
    // element is two 16B LDS reads + 4 v_dot2_f32_bf16 over i
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* b_lds = reinterpret_cast<__bf16*>(smem);          // [32e][O*F][8i]
    __bf16* x_lds = b_lds + UB_E * O * F * 8;                 // [32c][32e][8i]

    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * UB_E;
    const int oif = O * I * F;
    const int of = O * F;

    for (int t = tid; t < UB_E * of; t += UB_NT) {   // zero-init b pad lanes
        *reinterpret_cast<bf16x8*>(b_lds + (size_t)t * 8) = bf16x8(0);
    }
    __syncthreads();
    for (int t = tid; t < UB_E * oif; t += UB_NT) {
        int e = t / oif, r = t % oif;
        int o = r / (I * F), rem = r % (I * F);
        int i = rem / F, f = rem % F;
        b_lds[((size_t)e * of + o * F + f) * 8 + i] =
            (__bf16)((e0 + e < E) ? B[(size_t)(e0 + e) * oif + r] : 0.f);
    }

    // the staging loop below strides by UB_NT = UB_E * 8: a thread stages
    // the same (e, i) of every channel, so its x row is fixed
    static_assert(UB_NT == UB_E * 8, "x staging: one (e, i) per thread");
    const long xr = ub_x_row<GATHER>(rows, e0 + tid / 8, E, N);

    for (int c0 = 0; c0 < C; c0 += UB_C) {
        __syncthreads();   // previous chunk's compute done with x_lds
        for (int t = tid; t < UB_C * UB_E * 8; t += UB_NT) {
            int c = t / (UB_E * 8), rem = t % (UB_E * 8);
            int e = rem / 8, i = rem % 8;
            // channels past C read as zero: their rows of U, where U has
            // them, are the zero pad rows
            x_lds[((size_t)c * UB_E + e) * 8 + i] = (__bf16)(
                (i < I && xr >= 0 && c0 + c < C)
                    ? (float)X[((size_t)xr * C + c0 + c) * I + i] : 0.f);
        }
        __syncthreads();
        // out vectors of this chunk: (c 32) x (f F) x (e 32), e minor; the
        // thread computes all O lanes of its vector and stores it whole
        const int nel = UB_C * F * UB_E;
        for (int t = tid; t < nel; t += UB_NT) {
            int e = t & (UB_E - 1);
            int cf = t / UB_E;         // c*F + f
            int f = cf % F, c = cf / F;
            bf16x8 xv = *reinterpret_cast<const bf16x8*>(
                x_lds + ((size_t)c * UB_E + e) * 8);
            const ub_bf16x2* x2 = reinterpret_cast<const ub_bf16x2*>(&xv);
            __bf16 v[OP];
#pragma unroll
            for (int o = 0; o < OP; ++o) {
                v[o] = (__bf16)0.f;
                if (o < O) {
                    bf16x8 bv = *reinterpret_cast<const bf16x8*>(
                        b_lds + ((size_t)e * of + o * F + f) * 8);
                    const ub_bf16x2* b2 = reinterpret_cast<const ub_bf16x2*>(&bv);
                    float acc = 0.f;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        acc = __builtin_amdgcn_fdot2_f32_bf16(b2[p], x2[p], acc, false);
                    v[o] = (__bf16)acc;
                }
            }
            if (e0 + e < E && (c0 + c) * F + f < urows) {
                __bf16* dst = Ut + (((size_t)(c0 + c) * F + f) * E + e0 + e) * OP;
                if constexpr (OP == 1) dst[0] = v[0];
                else *reinterpret_cast<typename OVec<OP>::type*>(dst) =
                         *reinterpret_cast<typename OVec<OP>::type*>(v);
            }
        }
    }
}

template <typename TX, int OP>
__global__ void __launch_bounds__(UB_NT)
ubuild_fwd_kernel(const float* __restrict__ B, const TX* __restrict__ X,
                  __bf16* __restrict__ Ut, int E, int C, int O, int I, int F,
                  int urows) {
    ubuild_fwd_body<TX, OP, false>(B, X, nullptr, Ut, E, E, C, O, I, F, urows);
}

template <typename TX, int OP>
__global__ void __launch_bounds__(UB_NT)
ubuild_gather_fwd_kernel(const float* __restrict__ B, const TX* __restrict__ Xn,
                         const int* __restrict__ rows, __bf16* __restrict__ Ut,
                         int E, int N, int C, int O, int I, int F) {
    ubuild_fwd_body<TX, OP, true>(B, Xn, rows, Ut, E, N, C, O, I, F, C * F);
}

template <typename TX, typename TG>
__global__ void __launch_bounds__(UB_NT)
ubuild_bwd_dx_kernel(const float* __restrict__ B,   // (E, O, I, F)
                     const TG* __restrict__ dU,     // (C*F, E, OP) f32 | bf16
                     TX* __restrict__ dX,           // (E, C, I)
                     int E, int C, int O, int I, int F) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* b_lds = reinterpret_cast<float*>(smem);            // [16e][O*I*F]
    float* g_lds = b_lds + UB_EB * O * I * F;                 // [8c][F*O][16e]

    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * UB_EB;
    const int oif = O * I * F;
    const int fo = F * O;
    const int OP = opad_of(O);

    for (int t = tid; t < UB_EB * oif; t += UB_NT) {
        int e = t / oif, r = t % oif;
        b_lds[e * oif + r] = (e0 + e < E) ? B[(size_t)(e0 + e) * oif + r] : 0.f;
    }

    for (int c0 = 0; c0 < C; c0 += UB_CB) {
        __syncthreads();
        // dU tile, read in memory order (o minor, pads skipped)
        for (int t = tid; t < UB_CB * F * UB_EB * OP; t += UB_NT) {
            int o = t % OP;
            int r = t / OP;
            int e = r % UB_EB;
            int cf = r / UB_EB;        // c*F + f
            int c = cf / F, f = cf % F;
            if (o < O)
                g_lds[(c * fo + f * O + o) * UB_EB + e] = (e0 + e < E && c0 + c < C)
                    ? (float)dU[(((size_t)(c0 + c) * F + f) * E + e0 + e) * OP + o] : 0.f;
        }
        __syncthreads();
        // dX elements: (c 8) x (i I) x (e 16), e minor
        const int nel = UB_CB * I * UB_EB;
        for (int t = tid; t < nel; t += UB_NT) {
            int e = t % UB_EB;
            int r = t / UB_EB;
            int i = r % I, c = r / I;
            float acc = 0.f;
            const float* g = g_lds + (c * fo) * UB_EB + e;
            const float* b = b_lds + e * oif + i * F;
            for (int f = 0; f < F; ++f)
                for (int o = 0; o < O; ++o)
                    acc = fmaf(b[(size_t)o * I * F + f], g[(f * O + o) * UB_EB], acc);
            if (e0 + e < E && c0 + c < C)
                dX[((size_t)(e0 + e) * C + c0 + c) * I + i] = (TX)acc;
        }
    }
}

// dB[e,o,i,f] = sum_c X[e,c,i] * dU[(c*F+f), o, e]. Same 16-edge dU tile as
// the dX kernel; every thread owns up to UB_DBK fixed (o,i,f,e) outputs and
// keeps their sums over all channel chunks in registers, so dB is written
// once and needs no atomics. Straight-through for the forward's bf16
// rounding of B and X.
#define UB_DBK 22        // ceil(16 * 343 / 256)

template <typename TX, typename TG, bool GATHER>
__device__ __forceinline__ void
ubuild_bwd_db_body(const TX* __restrict__ X,      // (E, C, I) | (N, C, I)
                   const int* __restrict__ rows,  // (E,) when GATHER
                   const TG* __restrict__ dU,     // (C*F, E, OP) f32 | bf16
                   float* __restrict__ dB,        // (E, O, I, F)
                   int E, int N, int C, int O, int I, int F) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* g_lds = reinterpret_cast<float*>(smem);            // [8c][F*O][16e]
    float* x_lds = g_lds + UB_CB * F * O * UB_EB;             // [8c][I][16e]

    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * UB_EB;
    const int oif = O * I * F;
    const int fo = F * O;
    const int OP = opad_of(O);
    const int nout = UB_EB * oif;

    // per-output LDS offsets (channel 0), packed: x offset | g offset << 10
    int offs[UB_DBK];
    float acc[UB_DBK];
#pragma unroll
    for (int k = 0; k < UB_DBK; ++k) {
        int t = tid + k * UB_NT;
        int e = t % UB_EB;
        int r = (t / UB_EB) % oif;     // wraps only for t >= nout (unused)
        int o = r / (I * F), rem = r % (I * F);
        int i = rem / F, f = rem % F;
        offs[k] = (i * UB_EB + e) | (((f * O + o) * UB_EB + e) << 10);
        acc[k] = 0.f;
    }
    // x staging strides by UB_NT, a multiple of UB_EB: one e per thread
    static_assert(UB_NT % UB_EB == 0, "x staging: one e per thread");
    const long xr = ub_x_row<GATHER>(rows, e0 + tid % UB_EB, E, N);

    for (int c0 = 0; c0 < C; c0 += UB_CB) {
        __syncthreads();
        for (int t = tid; t < UB_CB * F * UB_EB * OP; t += UB_NT) {
            int o = t % OP;
            int r = t / OP;
            int e = r % UB_EB;
            int cf = r / UB_EB;        // c*F + f
            int c = cf / F, f = cf % F;
            if (o < O)
                g_lds[(c * fo + f * O + o) * UB_EB + e] = (e0 + e < E && c0 + c < C)
                    ? (float)dU[(((size_t)(c0 + c) * F + f) * E + e0 + e) * OP + o] : 0.f;
        }
        for (int t = tid; t < UB_CB * I * UB_EB; t += UB_NT) {
            int r = t / UB_EB;         // c*I + i
            int c = r / I, i = r % I;
            x_lds[t] = (xr >= 0 && c0 + c < C)
                ? (float)X[((size_t)xr * C + c0 + c) * I + i] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < UB_DBK; ++k) {
            if (tid + k * UB_NT < nout) {
                const float* xp = x_lds + (offs[k] & 1023);
                const float* gp = g_lds + (offs[k] >> 10);
                float a = acc[k];
#pragma unroll
                for (int c = 0; c < UB_CB; ++c)
                    a = fmaf(xp[c * I * UB_EB], gp[c * fo * UB_EB], a);
                acc[k] = a;
            }
        }
    }

#pragma unroll
    for (int k = 0; k < UB_DBK; ++k) {
        int t = tid + k * UB_NT;
        int e = t % UB_EB, r = t / UB_EB;
        if (t < nout && e0 + e < E)
            dB[(size_t)(e0 + e) * oif + r] = acc[k];
    }
}

template <typename TX, typename TG>
__global__ void __launch_bounds__(UB_NT)
ubuild_bwd_db_kernel(const TX* __restrict__ X, const TG* __restrict__ dU,
                     float* __restrict__ dB, int E, int C, int O, int I, int F) {
    ubuild_bwd_db_body<TX, TG, false>(X, nullptr, dU, dB, E, E, C, O, I, F);
}

template <typename TX, typename TG>
__global__ void __launch_bounds__(UB_NT)
ubuild_gather_bwd_db_kernel(const TX* __restrict__ Xn,
                            const int* __restrict__ rows,
                            const TG* __restrict__ dU,
                            float* __restrict__ dB,
                            int E, int N, int C, int O, int I, int F) {
    ubuild_bwd_db_body<TX, TG, true>(Xn, rows, dU, dB, E, N, C, O, I, F);
}

// dXn[rows[e], c, i] += sum_{f,o} B[e,o,i,f] * dU[(c*F+f), e, o]
//
// The arithmetic of ubuild_bwd_dx_kernel, mapped for the atomics: a
// destination row is contiguous over (c, i), so the threads of a chunk run
// (c, i) minor, e major, and a wave's 64 adds are contiguous runs of CB*I
// floats (CB is chosen by the host so a run is at least 128 B): two rows
// per instruction, three where a 40- or 48-float run straddles, not 16. The dU tile sits [e][c][f*O+o]: lanes differ in c, F*O is odd, so
// the compute reads are conflict-free.
template <int CB, typename TG>
__global__ void __launch_bounds__(UB_NT)
ubuild_gather_bwd_dx_kernel(const float* __restrict__ B,   // (E, O, I, F)
                            const TG* __restrict__ dU,     // (C*F, E, OP) f32 | bf16
                            const int* __restrict__ rows,  // (E,)
                            float* __restrict__ dXn,       // (N, C, I) f32
                            int E, int N, int C, int O, int I, int F) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int r_lds[UB_EB];
    float* b_lds = reinterpret_cast<float*>(smem);            // [16e][O*I*F]
    float* g_lds = b_lds + UB_EB * O * I * F;                 // [16e][CB c][F*O]

    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * UB_EB;
    const int oif = O * I * F;
    const int fo = F * O;
    const int OP = opad_of(O);

    if (tid < UB_EB) r_lds[tid] = (int)ub_x_row<true>(rows, e0 + tid, E, N);
    for (int t = tid; t < UB_EB * oif; t += UB_NT) {
        int e = t / oif, r = t % oif;
        b_lds[e * oif + r] = (e0 + e < E) ? B[(size_t)(e0 + e) * oif + r] : 0.f;
    }

    for (int c0 = 0; c0 < C; c0 += CB) {
        __syncthreads();
        // dU tile, read in memory order (o minor, pads skipped)
        for (int t = tid; t < CB * F * UB_EB * OP; t += UB_NT) {
            int o = t % OP;
            int r = t / OP;
            int e = r % UB_EB;
            int cf = r / UB_EB;        // c*F + f
            int c = cf / F, f = cf % F;
            if (o < O)
                g_lds[(e * CB + c) * fo + f * O + o] = (e0 + e < E)
                    ? (float)dU[(((size_t)(c0 + c) * F + f) * E + e0 + e) * OP + o] : 0.f;
        }
        __syncthreads();
        // dXn elements: (e 16) x (c CB) x (i I), (c, i) minor as in memory
        const int run = CB * I;
        for (int t = tid; t < UB_EB * run; t += UB_NT) {
            int e = t / run, ci = t % run;
            int c = ci / I, i = ci % I;
            float acc = 0.f;
            const float* g = g_lds + (e * CB + c) * fo;
            const float* b = b_lds + e * oif + i * F;
            for (int f = 0; f < F; ++f)
                for (int o = 0; o < O; ++o)
                    acc = fmaf(b[(size_t)o * I * F + f], g[f * O + o], acc);
            int row = r_lds[e];
            if (row >= 0)
                atomicAdd(&dXn[((size_t)row * C + c0) * I + ci], acc);
        }
    }
}

// dU arrives f32, or bf16 as pairconv_bwd_du rounds it; the staging load
// widens to the f32 LDS tile either way.
static bool check_du_dtype(const torch::Tensor& dU) {
    return dU.dtype() == torch::kFloat32 || dU.dtype() == torch::kBFloat16;
}

// dU holds rows = C*F rows of E*OP, or ceil32(rows) of them (pad rows unread)
static bool check_du_rows(const torch::Tensor& dU, int rows, int E, int O) {
    const int64_t per = (int64_t)E * opad_of(O);
    return dU.numel() == rows * per || dU.numel() == ceil_mif(rows) * per;
}

void ubuild_fwd(torch::Tensor B, torch::Tensor X, torch::Tensor Ut,
                int64_t O, int64_t I, int64_t F) {
    TORCH_CHECK(B.is_cuda() && B.is_contiguous() && B.dtype() == torch::kFloat32);
    TORCH_CHECK(X.is_contiguous() && Ut.is_contiguous() &&
                Ut.dtype() == torch::kBFloat16);
    int E = B.size(0);
    int C = X.size(1);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    const int OP = opad_of((int)O);
    const int urows = Ut.dim() == 3 ? (int)Ut.size(0) : -1;
    TORCH_CHECK(C >= 1 && (urows == C * F || urows == ceil_mif(C * (int)F)) &&
                Ut.size(1) == E && Ut.size(2) == OP,
                "expect U as (C*F or ceil32(C*F), E, OP(O))");
    TORCH_CHECK(B.numel() == (int64_t)E * O * I * F && X.size(0) == E && X.size(2) == I);
    TORCH_CHECK(O * I * F <= 343, "degree pair too large for LDS staging");
    TORCH_CHECK(I <= 8, "I (2*d_in+1) must be <= 8");
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + UB_E - 1) / UB_E);
    size_t lds = (size_t)UB_E * O * F * 8 * 2 + (size_t)UB_C * UB_E * 8 * 2;
#define UB_LAUNCH_FWD(OPV)                                                    \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ubuild_fwd_kernel<T, OPV>), grid,      \
                       dim3(UB_NT), lds, stream, B.data_ptr<float>(),         \
                       tptr<const T>(X), tptr<__bf16>(Ut),                    \
                       E, C, (int)O, (int)I, (int)F, urows)
    DISPATCH_F32_BF16(X, __bf16, {
        if (OP == 8) UB_LAUNCH_FWD(8);
        else if (OP == 4) UB_LAUNCH_FWD(4);
        else UB_LAUNCH_FWD(1);
    });
#undef UB_LAUNCH_FWD
    check_launch("ubuild_fwd: ");
}

void ubuild_bwd_dx(torch::Tensor B, torch::Tensor dU, torch::Tensor dX,
                   int64_t O, int64_t I, int64_t F) {
    TORCH_CHECK(B.is_cuda() && B.is_contiguous() && B.dtype() == torch::kFloat32);
    TORCH_CHECK(dU.is_contiguous() && check_du_dtype(dU) && dX.is_contiguous());
    int E = B.size(0);
    int C = dX.size(1);
    TORCH_CHECK(O * I * F <= 343);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(C >= 1 && check_du_rows(dU, C * (int)F, E, (int)O),
                "expect dU as (C*F or ceil32(C*F), E, OP(O))");
    const bool du16 = dU.dtype() == torch::kBFloat16;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + UB_EB - 1) / UB_EB);
    size_t lds = (size_t)UB_EB * O * I * F * 4 + (size_t)UB_CB * F * O * UB_EB * 4;
#define UB_LAUNCH_DX(TG)                                                      \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ubuild_bwd_dx_kernel<T, TG>), grid,    \
                       dim3(UB_NT), lds, stream, B.data_ptr<float>(),         \
                       tptr<const TG>(dU), tptr<T>(dX),                       \
                       E, C, (int)O, (int)I, (int)F)
    DISPATCH_F32_BF16(dX, __bf16, {
        if (du16) UB_LAUNCH_DX(__bf16); else UB_LAUNCH_DX(float);
    });
#undef UB_LAUNCH_DX
    check_launch("ubuild_bwd_dx: ");
}

void ubuild_bwd_db(torch::Tensor X, torch::Tensor dU, torch::Tensor dB,
                   int64_t O, int64_t I, int64_t F) {
    TORCH_CHECK(X.is_cuda() && X.is_contiguous() && X.dim() == 3);
    TORCH_CHECK(dU.is_cuda() && dU.is_contiguous() && check_du_dtype(dU));
    TORCH_CHECK(dB.is_cuda() && dB.is_contiguous() &&
                dB.dtype() == torch::kFloat32);
    int E = X.size(0);
    int C = X.size(1);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(X.size(2) == I && C >= 1 && check_du_rows(dU, C * (int)F, E, (int)O) &&
                dB.numel() == (int64_t)E * O * I * F);
    TORCH_CHECK(O * I * F <= 343);
    if (E == 0) return;
    size_t lds = (size_t)UB_CB * UB_EB * (F * O + I) * 4;
    TORCH_CHECK(lds <= 64 * 1024, "degree pair too large for LDS staging");
    const bool du16 = dU.dtype() == torch::kBFloat16;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + UB_EB - 1) / UB_EB);
#define UB_LAUNCH_DB(TG)                                                      \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ubuild_bwd_db_kernel<T, TG>), grid,    \
                       dim3(UB_NT), lds, stream, tptr<const T>(X),            \
                       tptr<const TG>(dU), dB.data_ptr<float>(),              \
                       E, C, (int)O, (int)I, (int)F)
    DISPATCH_F32_BF16(X, __bf16, {
        if (du16) UB_LAUNCH_DB(__bf16); else UB_LAUNCH_DB(float);
    });
#undef UB_LAUNCH_DB
    check_launch("ubuild_bwd_db: ");
}

// The checks the three gather entry points share; returns N.
static int check_gather(const torch::Tensor& Xn, const torch::Tensor& rows,
                        int64_t E, int64_t I) {
    TORCH_CHECK(Xn.is_cuda() && Xn.is_contiguous() && Xn.dim() == 3 &&
                Xn.size(2) == I, "expect Xn as (N, C, I), contiguous");
    TORCH_CHECK(rows.is_cuda() && rows.is_contiguous() &&
                rows.dtype() == torch::kInt32 && rows.numel() == E,
                "expect rows as (E,) int32, contiguous");
    TORCH_CHECK(Xn.size(0) < (1LL << 31));
    return (int)Xn.size(0);
}

void ubuild_gather_fwd(torch::Tensor B, torch::Tensor Xn, torch::Tensor rows,
                       torch::Tensor Ut, int64_t O, int64_t I, int64_t F) {
    TORCH_CHECK(B.is_cuda() && B.is_contiguous() && B.dtype() == torch::kFloat32);
    TORCH_CHECK(Ut.is_cuda() && Ut.is_contiguous() &&
                Ut.dtype() == torch::kBFloat16);
    int E = B.size(0);
    int N = check_gather(Xn, rows, E, I);
    int C = Xn.size(1);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    const int OP = opad_of((int)O);
    TORCH_CHECK(Ut.dim() == 3 && Ut.size(0) == (int64_t)C * F && Ut.size(1) == E &&
                Ut.size(2) == OP, "expect U as (C*F, E, OP(O))");
    TORCH_CHECK(B.numel() == (int64_t)E * O * I * F);
    TORCH_CHECK(C % UB_C == 0, "channels must be a multiple of 32");
    TORCH_CHECK(O * I * F <= 343, "degree pair too large for LDS staging");
    TORCH_CHECK(I <= 8, "I (2*d_in+1) must be <= 8");
    if (E == 0) return;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + UB_E - 1) / UB_E);
    size_t lds = (size_t)UB_E * O * F * 8 * 2 + (size_t)UB_C * UB_E * 8 * 2;
#define UB_LAUNCH_GFWD(OPV)                                                   \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ubuild_gather_fwd_kernel<T, OPV>),     \
                       grid, dim3(UB_NT), lds, stream, B.data_ptr<float>(),   \
                       tptr<const T>(Xn), rows.data_ptr<int>(),               \
                       tptr<__bf16>(Ut), E, N, C, (int)O, (int)I, (int)F)
    DISPATCH_F32_BF16(Xn, __bf16, {
        if (OP == 8) UB_LAUNCH_GFWD(8);
        else if (OP == 4) UB_LAUNCH_GFWD(4);
        else UB_LAUNCH_GFWD(1);
    });
#undef UB_LAUNCH_GFWD
    check_launch("ubuild_gather_fwd: ");
}

void ubuild_gather_bwd_dx(torch::Tensor B, torch::Tensor dU, torch::Tensor rows,
                          torch::Tensor dXn, int64_t O, int64_t I, int64_t F) {
    TORCH_CHECK(B.is_cuda() && B.is_contiguous() && B.dtype() == torch::kFloat32);
    TORCH_CHECK(dU.is_cuda() && dU.is_contiguous() && check_du_dtype(dU));
    TORCH_CHECK(dXn.dtype() == torch::kFloat32,
                "dXn accumulates in fp32 (zero it, cast afterwards)");
    int E = B.size(0);
    int N = check_gather(dXn, rows, E, I);
    int C = dXn.size(1);
    TORCH_CHECK(C % UB_C == 0, "channels must be a multiple of 32");
    TORCH_CHECK(O * I * F <= 343);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(B.numel() == (int64_t)E * O * I * F &&
                dU.numel() == (int64_t)C * F * E * opad_of((int)O),
                "expect dU as (C*F, E, OP(O))");
    if (E == 0) return;
    // channel chunk: one edge's run of chunk*I floats is >= 128 B; halved
    // while B plus the dU tile would pass 64 KiB
    int cb = I >= 5 ? 8 : (I >= 3 ? 16 : 32);
    auto lds_of = [&](int c) {
        return (size_t)UB_EB * O * I * F * 4 + (size_t)c * F * O * UB_EB * 4;
    };
    while (cb > 8 && lds_of(cb) > 64 * 1024) cb /= 2;
    size_t lds = lds_of(cb);
    TORCH_CHECK(lds + UB_EB * 4 <= 64 * 1024,
                "degree pair too large for LDS staging");
    const bool du16 = dU.dtype() == torch::kBFloat16;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + UB_EB - 1) / UB_EB);
#define UB_LAUNCH_GDX(CBV, TG)                                                \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ubuild_gather_bwd_dx_kernel<CBV, TG>), \
                       grid, dim3(UB_NT), lds, stream, B.data_ptr<float>(),   \
                       tptr<const TG>(dU), rows.data_ptr<int>(),              \
                       dXn.data_ptr<float>(), E, N, C, (int)O, (int)I, (int)F)
#define UB_LAUNCH_GDX_CB(TG)                                                  \
    if (cb == 32) UB_LAUNCH_GDX(32, TG);                                      \
    else if (cb == 16) UB_LAUNCH_GDX(16, TG);                                 \
    else UB_LAUNCH_GDX(8, TG)
    if (du16) { UB_LAUNCH_GDX_CB(__bf16); } else { UB_LAUNCH_GDX_CB(float); }
#undef UB_LAUNCH_GDX_CB
#undef UB_LAUNCH_GDX
    check_launch("ubuild_gather_bwd_dx: ");
}

void ubuild_gather_bwd_db(torch::Tensor Xn, torch::Tensor rows, torch::Tensor dU,
                          torch::Tensor dB, int64_t O, int64_t I, int64_t F) {
    TORCH_CHECK(dU.is_cuda() && dU.is_contiguous() && check_du_dtype(dU));
    TORCH_CHECK(dB.is_cuda() && dB.is_contiguous() &&
                dB.dtype() == torch::kFloat32);
    TORCH_CHECK(dB.dim() == 4, "expect dB as (E, O, I, F)");
    int E = dB.size(0);
    int N = check_gather(Xn, rows, E, I);
    int C = Xn.size(1);
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(dU.numel() == (int64_t)C * F * E * opad_of((int)O) &&
                dB.numel() == (int64_t)E * O * I * F);
    TORCH_CHECK(C % UB_CB == 0, "channels must be a multiple of 8");
    TORCH_CHECK(O * I * F <= 343);
    if (E == 0) return;
    size_t lds = (size_t)UB_CB * UB_EB * (F * O + I) * 4;
    TORCH_CHECK(lds <= 64 * 1024, "degree pair too large for LDS staging");
    const bool du16 = dU.dtype() == torch::kBFloat16;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((E + UB_EB - 1) / UB_EB);
#define UB_LAUNCH_GDB(TG)                                                     \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ubuild_gather_bwd_db_kernel<T, TG>),   \
                       grid, dim3(UB_NT), lds, stream, tptr<const T>(Xn),     \
                       rows.data_ptr<int>(), tptr<const TG>(dU),              \
                       dB.data_ptr<float>(), E, N, C, (int)O, (int)I, (int)F)
    DISPATCH_F32_BF16(Xn, __bf16, {
        if (du16) UB_LAUNCH_GDB(__bf16); else UB_LAUNCH_GDB(float);
    });
#undef UB_LAUNCH_GDB
    check_launch("ubuild_gather_bwd_db: ");
}
