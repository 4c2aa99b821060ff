// Fused equivariant norm-nonlinearity (NormSE3, reference
// se3_transformer_pytorch.py:97-152), every variant the package builds:
// {scale, gated scale} x {exact-erf GELU, identity}.
//
// Scale path, one kernel each way (eager needs ~6 passes):
//   nu    = max(||t||_m, eps)
//   out   = g(nu * scale_c) * t / nu
// Backward solves the analytic Jacobian in one pass:
//   with p = t/nu, a = p . dout
//   dt     = g'(s nu) * s * a * p + g(s nu)/nu * (dout - a p)     (nu > eps)
//   dt     = g(s eps)/eps * dout                                   (clamped)
//   dscale = g'(s nu) * nu * a   (summed over rows -> atomicAdd per channel)
//
// Gated-scale path (w_gate, a CxC matrix): an output row needs the norms
// of every channel of its node, so a block owns a tile of GR nodes.
//   gate[n,e]  = sum_d nu[n,d] W[d,e]
//   out[n,e,:] = g(gate[n,e]) * t[n,e,:] / nu[n,e]
// Phase 1 puts the GR x C norms into LDS, phase 2 is a VALU fp32 matvec
// (thread owns channel e, W[d,.] coalesced along e, nu[.][d] one LDS
// broadcast read of all GR rows), phase 3 re-reads t (L2-hot). Backward:
//   dgate[n,e] = g'(gate) * a[n,e]
//   dnu[n,d]   = sum_e W[d,e] dgate[n,e]        (against W^T: coalesced)
//   dt         = g(gate)/nu * (dout - a p) + dnu * p              (nu > eps)
//   dt         = g(gate)/eps * dout                               (clamped)
// and writes dgate and nu (N x C fp32) so the caller forms
// dW = nu^T @ dgate with one library GEMM: deterministic, no atomics.
// Exact-erf GELU matches torch.nn.GELU; all math in fp32 registers.

#include <hip/hip_runtime.h>
#include "host_common.h"
#include "ops.h"
#include <hip/hip_bf16.h>

#define NTN 256
// Gated kernels: nodes per block, and the channel ceiling. LDS is one
// float4 per channel (GR rows): 16*C bytes, 32 KiB at the ceiling, so five
// blocks still share a CU's 160 KiB; above it the caller stays on eager.
#define GR 4
#define GATED_MAX_C 2048

__device__ __forceinline__ float gelu_f(float x) {
    return 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
}
__device__ __forceinline__ float gelu_grad_f(float x) {
    float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
    float pdf = 0.3989422804014327f * expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// compile-time nonlinearity selector: NL 0 = exact-erf GELU, 1 = identity
template <int NL>
__device__ __forceinline__ float nl_f(float x) {
    if constexpr (NL == 0) return gelu_f(x);
    else return x;
}
template <int NL>
__device__ __forceinline__ float nl_grad_f(float x) {
    if constexpr (NL == 0) return gelu_grad_f(x);
    else return 1.f;
}

template <typename T, int M, int NL>
__global__ void __launch_bounds__(NTN)
norm_se3_fwd_kernel(const T* __restrict__ t, const float* __restrict__ scale,
                    T* __restrict__ out, long rows, int C, float eps) {
    long i = (long)blockIdx.x * NTN + threadIdx.x;   // row = (bn, c)
    if (i >= rows) return;
    int c = (int)(i % C);
    float v[M];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        v[j] = (float)t[i * M + j];
        ss += v[j] * v[j];
    }
    float nu = fmaxf(sqrtf(ss), eps);
    float g = nl_f<NL>(nu * scale[c]) / nu;
#pragma unroll
    for (int j = 0; j < M; ++j) out[i * M + j] = (T)(v[j] * g);
}

template <typename T, int M, int NL>
__global__ void __launch_bounds__(NTN)
norm_se3_bwd_kernel(const T* __restrict__ t, const float* __restrict__ scale,
                    const T* __restrict__ dout, T* __restrict__ dt,
                    float* __restrict__ dscale, long rows, int C, float eps) {
    long i = (long)blockIdx.x * NTN + threadIdx.x;
    if (i >= rows) return;
    int c = (int)(i % C);
    float v[M], d[M];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        v[j] = (float)t[i * M + j];
        d[j] = (float)dout[i * M + j];
        ss += v[j] * v[j];
    }
    float nraw = sqrtf(ss);
    float s = scale[c];
    if (nraw <= eps) {
        float k = nl_f<NL>(s * eps) / eps;
#pragma unroll
        for (int j = 0; j < M; ++j) dt[i * M + j] = (T)(k * d[j]);
        return;
    }
    float inv = 1.f / nraw;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < M; ++j) a += v[j] * inv * d[j];
    float x = s * nraw;
    float g = nl_f<NL>(x) * inv;
    float gp = nl_grad_f<NL>(x);
#pragma unroll
    for (int j = 0; j < M; ++j) {
        float p = v[j] * inv;
        dt[i * M + j] = (T)(gp * s * a * p + g * (d[j] - a * p));
    }
    atomicAdd(&dscale[c], gp * nraw * a);
}

// ---- gated scale -----------------------------------------------------------
// t (N, C, M), W (C, C) fp32 [d, e], gate (N, C) fp32. Block b owns nodes
// [GR*b, GR*b + GR); LDS holds float4 s[c] = the GR rows' value at channel c.

template <typename T, int M, int NL>
__global__ void __launch_bounds__(NTN)
norm_se3_gated_fwd_kernel(const T* __restrict__ t, const float* __restrict__ W,
                          T* __restrict__ out, float* __restrict__ gate,
                          long N, int C, float eps) {
    extern __shared__ float4 s_nu4[];
    float* s_nu = reinterpret_cast<float*>(s_nu4);
    const long n0 = (long)blockIdx.x * GR;

    // phase 1: norms of the tile; rows past N hold 0 and are never written
    for (int i = threadIdx.x; i < GR * C; i += NTN) {
        int r = i / C, c = i - r * C;
        long n = n0 + r;
        float nu = 0.f;
        if (n < N) {
            const T* tp = t + (n * C + c) * M;
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                float v = (float)tp[j];
                ss += v * v;
            }
            nu = fmaxf(sqrtf(ss), eps);
        }
        s_nu[c * GR + r] = nu;
    }
    __syncthreads();

    for (int e = threadIdx.x; e < C; e += NTN) {
        // phase 2: gate[r][e] = sum_d nu[r][d] W[d][e]
        float acc[GR];
#pragma unroll
        for (int r = 0; r < GR; ++r) acc[r] = 0.f;
#pragma unroll 8
        for (int d = 0; d < C; ++d) {
            float w = W[(long)d * C + e];
            float4 u = s_nu4[d];
            acc[0] += u.x * w;
            acc[1] += u.y * w;
            acc[2] += u.z * w;
            acc[3] += u.w * w;
        }
        // phase 3
        float4 nu4 = s_nu4[e];
        float nus[GR] = {nu4.x, nu4.y, nu4.z, nu4.w};
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            long n = n0 + r;
            if (n < N) {
                long row = n * C + e;
                gate[row] = acc[r];
                float g = nl_f<NL>(acc[r]) / nus[r];
#pragma unroll
                for (int j = 0; j < M; ++j)
                    out[row * M + j] = (T)((float)t[row * M + j] * g);
            }
        }
    }
}

template <typename T, int M, int NL>
__global__ void __launch_bounds__(NTN)
norm_se3_gated_bwd_kernel(const T* __restrict__ t, const float* __restrict__ Wt,
                          const float* __restrict__ gate,
                          const T* __restrict__ dout, T* __restrict__ dt,
                          float* __restrict__ dgate, float* __restrict__ nu_out,
                          long N, int C, float eps) {
    extern __shared__ float4 s_dg4[];
    float* s_dg = reinterpret_cast<float*>(s_dg4);
    const long n0 = (long)blockIdx.x * GR;

    // phase 1: nu, a = p . dout, dgate = g'(gate) a
    for (int i = threadIdx.x; i < GR * C; i += NTN) {
        int r = i / C, c = i - r * C;
        long n = n0 + r;
        float dg = 0.f;
        if (n < N) {
            long row = n * C + c;
            float ss = 0.f, vd = 0.f;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                float v = (float)t[row * M + j];
                ss += v * v;
                vd += v * (float)dout[row * M + j];
            }
            float nu = fmaxf(sqrtf(ss), eps);
            dg = nl_grad_f<NL>(gate[row]) * (vd / nu);
            dgate[row] = dg;
            nu_out[row] = nu;
        }
        s_dg[c * GR + r] = dg;
    }
    __syncthreads();

    for (int c = threadIdx.x; c < C; c += NTN) {
        // phase 2: dnu[r][c] = sum_e Wt[e][c] dgate[r][e]
        float acc[GR];
#pragma unroll
        for (int r = 0; r < GR; ++r) acc[r] = 0.f;
#pragma unroll 8
        for (int e = 0; e < C; ++e) {
            float w = Wt[(long)e * C + c];
            float4 u = s_dg4[e];
            acc[0] += u.x * w;
            acc[1] += u.y * w;
            acc[2] += u.z * w;
            acc[3] += u.w * w;
        }
        // phase 3
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            long n = n0 + r;
            if (n < N) {
                long row = n * C + c;
                float v[M], d[M];
                float ss = 0.f;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    v[j] = (float)t[row * M + j];
                    d[j] = (float)dout[row * M + j];
                    ss += v[j] * v[j];
                }
                float nraw = sqrtf(ss);
                float gv = nl_f<NL>(gate[row]);
                if (nraw <= eps) {
                    float k = gv / eps;
#pragma unroll
                    for (int j = 0; j < M; ++j)
                        dt[row * M + j] = (T)(k * d[j]);
                } else {
                    // true division: at M = 1 it makes p exactly +-1, so
                    // dout - a p cancels to exactly 0 (its true value)
                    // instead of g/nu times rounding noise, which for a
                    // small |t| would dominate dt
                    float p[M];
                    float a = 0.f;
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        p[j] = v[j] / nraw;
                        a += p[j] * d[j];
                    }
                    float g = gv / nraw;
#pragma unroll
                    for (int j = 0; j < M; ++j)
                        dt[row * M + j] =
                            (T)(g * (d[j] - a * p[j]) + acc[r] * p[j]);
                }
            }
        }
    }
}

#define DISPATCH_NL(NL, ...)                                      \
    switch (NL) {                                                 \
        case 0: { constexpr int kNL = 0; __VA_ARGS__; break; }    \
        case 1: { constexpr int kNL = 1; __VA_ARGS__; break; }    \
        default: TORCH_CHECK(false, "unsupported nonlinearity ", NL); \
    }

// Body runs with T (float | bf16), kM (order) and kNL (nonlinearity) bound.
#define DISPATCH_NORM(t, M, nonlin, ...)                          \
    DISPATCH_NL(nonlin, DISPATCH_ORDER(M, kM, "order",            \
        DISPATCH_F32_BF16(t, __hip_bfloat16, __VA_ARGS__)))

void norm_se3_nl_fwd(torch::Tensor t, torch::Tensor scale, torch::Tensor out,
                     double eps, int64_t nonlin) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && out.is_contiguous());
    TORCH_CHECK(scale.dtype() == torch::kFloat32 && scale.is_contiguous());
    TORCH_CHECK(out.dtype() == t.dtype() && out.numel() == t.numel());
    int M = t.size(-1), C = t.size(-2);
    TORCH_CHECK(scale.numel() == C, "norm_se3: scale must hold C values");
    long rows = t.numel() / M;
    if (rows == 0) return;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((rows + NTN - 1) / NTN);
    DISPATCH_NORM(t, M, nonlin, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(norm_se3_fwd_kernel<T, kM, kNL>),
                           grid, dim3(NTN), 0, stream,
                           tptr<const T>(t), scale.data_ptr<float>(),
                           tptr<T>(out), rows, C, (float)eps);
    });
    check_launch("norm_se3_fwd: ");
}

void norm_se3_nl_bwd(torch::Tensor t, torch::Tensor scale, torch::Tensor dout,
                     torch::Tensor dt, torch::Tensor dscale, double eps,
                     int64_t nonlin) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && dout.is_contiguous() &&
                dt.is_contiguous() && dscale.is_contiguous());
    TORCH_CHECK(scale.dtype() == torch::kFloat32 && scale.is_contiguous() &&
                dscale.dtype() == torch::kFloat32);
    TORCH_CHECK(dout.dtype() == t.dtype() && dt.dtype() == t.dtype() &&
                dout.numel() == t.numel() && dt.numel() == t.numel());
    int M = t.size(-1), C = t.size(-2);
    TORCH_CHECK(scale.numel() == C && dscale.numel() == C,
                "norm_se3: scale/dscale must hold C values");
    long rows = t.numel() / M;
    if (rows == 0) return;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((rows + NTN - 1) / NTN);
    DISPATCH_NORM(t, M, nonlin, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(norm_se3_bwd_kernel<T, kM, kNL>),
                           grid, dim3(NTN), 0, stream,
                           tptr<const T>(t), scale.data_ptr<float>(),
                           tptr<const T>(dout), tptr<T>(dt),
                           dscale.data_ptr<float>(), rows, C, (float)eps);
    });
    check_launch("norm_se3_bwd: ");
}

int64_t norm_se3_gated_max_c() { return GATED_MAX_C; }

static void check_f32_nc(const torch::Tensor& x, long N, int C, const char* name) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                x.dtype() == torch::kFloat32 && x.numel() == N * C,
                "norm_se3_gated: ", name, " must be contiguous fp32 (N, C)");
}

void norm_se3_gated_fwd(torch::Tensor t, torch::Tensor W, torch::Tensor out,
                        torch::Tensor gate, double eps, int64_t nonlin) {
    TORCH_CHECK(t.is_cuda() && t.dim() >= 2 && t.is_contiguous() &&
                out.is_contiguous());
    TORCH_CHECK(out.dtype() == t.dtype() && out.numel() == t.numel());
    int M = t.size(-1), C = t.size(-2);
    TORCH_CHECK(C >= 1 && C <= GATED_MAX_C,
                "norm_se3_gated: C must be in [1, ", GATED_MAX_C, "], got ", C);
    TORCH_CHECK(W.is_cuda() && W.is_contiguous() &&
                W.dtype() == torch::kFloat32 && W.dim() == 2 &&
                W.size(0) == C && W.size(1) == C,
                "norm_se3_gated: w_gate must be contiguous fp32 (C, C)");
    long N = t.numel() / ((long)M * C);
    check_f32_nc(gate, N, C, "gate");
    if (N == 0) return;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((N + GR - 1) / GR);
    size_t lds = (size_t)C * GR * sizeof(float);
    DISPATCH_NORM(t, M, nonlin, {
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(norm_se3_gated_fwd_kernel<T, kM, kNL>),
            grid, dim3(NTN), lds, stream,
            tptr<const T>(t), W.data_ptr<float>(), tptr<T>(out),
            gate.data_ptr<float>(), N, C, (float)eps);
    });
    check_launch("norm_se3_gated_fwd: ");
}

// Wt is w_gate transposed ([e, d], contiguous); dgate and nu come back as
// (N, C) fp32 for the caller's dW = nu^T @ dgate.
void norm_se3_gated_bwd(torch::Tensor t, torch::Tensor Wt, torch::Tensor gate,
                        torch::Tensor dout, torch::Tensor dt,
                        torch::Tensor dgate, torch::Tensor nu, double eps,
                        int64_t nonlin) {
    TORCH_CHECK(t.is_cuda() && t.dim() >= 2 && t.is_contiguous() &&
                dout.is_contiguous() && dt.is_contiguous());
    TORCH_CHECK(dout.dtype() == t.dtype() && dt.dtype() == t.dtype() &&
                dout.numel() == t.numel() && dt.numel() == t.numel());
    int M = t.size(-1), C = t.size(-2);
    TORCH_CHECK(C >= 1 && C <= GATED_MAX_C,
                "norm_se3_gated: C must be in [1, ", GATED_MAX_C, "], got ", C);
    TORCH_CHECK(Wt.is_cuda() && Wt.is_contiguous() &&
                Wt.dtype() == torch::kFloat32 && Wt.dim() == 2 &&
                Wt.size(0) == C && Wt.size(1) == C,
                "norm_se3_gated: w_gate^T must be contiguous fp32 (C, C)");
    long N = t.numel() / ((long)M * C);
    check_f32_nc(gate, N, C, "gate");
    check_f32_nc(dgate, N, C, "dgate");
    check_f32_nc(nu, N, C, "nu");
    if (N == 0) return;
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((N + GR - 1) / GR);
    size_t lds = (size_t)C * GR * sizeof(float);
    DISPATCH_NORM(t, M, nonlin, {
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(norm_se3_gated_bwd_kernel<T, kM, kNL>),
            grid, dim3(NTN), lds, stream,
            tptr<const T>(t), Wt.data_ptr<float>(), gate.data_ptr<float>(),
            tptr<const T>(dout), tptr<T>(dt), dgate.data_ptr<float>(),
            nu.data_ptr<float>(), N, C, (float)eps);
    });
    check_launch("norm_se3_gated_bwd: ");
}
