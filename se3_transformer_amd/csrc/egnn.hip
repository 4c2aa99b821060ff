// EGNN higher-type kernels (reference se3_transformer_pytorch.py:707-932).
//
// The reference (and any eager translation) materializes the FULL pairwise
// rel-htype tensor `htype[:,:,None] - htype[:,None,:]` of shape
// (b, n, n, d, m) — O(n^2 d m) memory — just to (a) gather k neighbor
// rel-distances for the edge MLP and (b) norm + weighted-sum k neighbors
// for the htype update (:801-836). These kernels compute both straight
// from the gathered neighbor indices: nothing O(n^2) ever exists.
//
//   rel[i,j,d,:] = htype[i,d,:] - htype[idx[i,j],d,:]
//   dist[i,j,d]  = ||rel||                                  (kernel 1)
//   upd[i,d,:]   = sum_j w[i,j,d] * rel * (u*s_d + t_d)/max(u, eps)
//                  with u = ||rel||                          (kernel 2;
//                  HtypesNorm semantics, reference :693-705)
//
// Backward: per-(i,j,d) recompute of rel/u; dhtype needs a scatter-add to
// the neighbor rows (atomic f32); dscale/dbias accumulate per-d atomics.

#include <hip/hip_runtime.h>
#include "host_common.h"
#include "ops.h"

#define EG_NT 256
#define EG_MAXM 7

// --------------------------------------------------------------------------
// kernel 1: neighbor rel-htype distances (fwd)  out (b,n,k,d)
// --------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(EG_NT)
egnn_rel_dist_fwd_kernel(const T* __restrict__ ht,     // (b,n,d,m)
                         const long* __restrict__ idx, // (b,n,k)
                         float* __restrict__ dist,     // (b,n,k,d)
                         long total, int n, int k, int d, int m) {
    for (long t = (long)blockIdx.x * EG_NT + threadIdx.x; t < total;
         t += (long)gridDim.x * EG_NT) {
        long dd = t % d, r = t / d;
        long jj = r % k, r2 = r / k;
        long i = r2 % n, b = r2 / n;
        long j = idx[(b * n + i) * k + jj];
        const T* a = ht + ((b * n + i) * d + dd) * m;
        const T* c = ht + ((b * n + j) * d + dd) * m;
        float s = 0.f;
        for (int mm = 0; mm < m; ++mm) {
            float rl = (float)a[mm] - (float)c[mm];
            s += rl * rl;
        }
        dist[t] = sqrtf(s);
    }
}

// backward of kernel 1: dht from ddist (atomic scatter for the j rows)
template <typename T>
__global__ void __launch_bounds__(EG_NT)
egnn_rel_dist_bwd_kernel(const T* __restrict__ ht, const long* __restrict__ idx,
                         const float* __restrict__ gdist,  // (b,n,k,d)
                         float* __restrict__ dht,          // (b,n,d,m) f32
                         long total, int n, int k, int d, int m) {
    for (long t = (long)blockIdx.x * EG_NT + threadIdx.x; t < total;
         t += (long)gridDim.x * EG_NT) {
        long dd = t % d, r = t / d;
        long jj = r % k, r2 = r / k;
        long i = r2 % n, b = r2 / n;
        long j = idx[(b * n + i) * k + jj];
        const T* a = ht + ((b * n + i) * d + dd) * m;
        const T* c = ht + ((b * n + j) * d + dd) * m;
        float rl[EG_MAXM], s = 0.f;
        for (int mm = 0; mm < m; ++mm) {
            rl[mm] = (float)a[mm] - (float)c[mm];
            s += rl[mm] * rl[mm];
        }
        const float u = sqrtf(s);
        const float g = gdist[t];
        if (u <= 0.f || g == 0.f) continue;   // norm subgradient at 0
        const float f = g / u;
        float* di = dht + ((b * n + i) * d + dd) * m;
        float* dj = dht + ((b * n + j) * d + dd) * m;
        for (int mm = 0; mm < m; ++mm) {
            atomicAdd(&di[mm], f * rl[mm]);
            atomicAdd(&dj[mm], -f * rl[mm]);
        }
    }
}

// --------------------------------------------------------------------------
// kernel 2: htype update (fwd)  upd (b,n,d,m)
//   factor(u) = (u*s + t) / max(u, eps)
// --------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(EG_NT)
egnn_htype_update_fwd_kernel(const T* __restrict__ ht,     // (b,n,d,m)
                             const long* __restrict__ idx, // (b,n,k)
                             const float* __restrict__ w,  // (b,n,k,d)
                             const float* __restrict__ sc, // (d) scale
                             const float* __restrict__ bi, // (d) bias
                             float* __restrict__ upd,      // (b,n,d,m) f32
                             long total, int n, int k, int d, int m,
                             float eps) {
    for (long t = (long)blockIdx.x * EG_NT + threadIdx.x; t < total;
         t += (long)gridDim.x * EG_NT) {
        long dd = t % d, r = t / d;
        long i = r % n, b = r / n;
        const T* a = ht + ((b * n + i) * d + dd) * m;
        const float s_ = sc[dd], t_ = bi[dd];
        float acc[EG_MAXM];
        for (int mm = 0; mm < m; ++mm) acc[mm] = 0.f;
        for (int jj = 0; jj < k; ++jj) {
            long j = idx[(b * n + i) * k + jj];
            const T* c = ht + ((b * n + j) * d + dd) * m;
            float rl[EG_MAXM], ss = 0.f;
            for (int mm = 0; mm < m; ++mm) {
                rl[mm] = (float)a[mm] - (float)c[mm];
                ss += rl[mm] * rl[mm];
            }
            const float u = sqrtf(ss);
            const float fac = (u * s_ + t_) / fmaxf(u, eps);
            const float wf = w[((b * n + i) * k + jj) * d + dd] * fac;
            for (int mm = 0; mm < m; ++mm) acc[mm] = fmaf(wf, rl[mm], acc[mm]);
        }
        float* o = upd + ((b * n + i) * d + dd) * m;
        for (int mm = 0; mm < m; ++mm) o[mm] = acc[mm];
    }
}

// backward of kernel 2: one thread per (b,i,jj,d) edge; recompute rel/u.
//   out_j = w * rel * f(u),  f(u) = (u s + t)/max(u,eps)
//   dw    = g . (rel f)
//   drel  = w [ f g + f'(u)/u * (rel.g) rel ],  f'(u) = d f/d u
//   (u > eps: f = s + t/u, f' = -t/u^2 ; u <= eps: f = (u s + t)/eps,
//    f' = s/eps)
//   dscale_d += w (rel.g) u/max(u,eps);  dbias_d += w (rel.g)/max(u,eps)
template <typename T>
__global__ void __launch_bounds__(EG_NT)
egnn_htype_update_bwd_kernel(const T* __restrict__ ht, const long* __restrict__ idx,
                             const float* __restrict__ w,
                             const float* __restrict__ sc,
                             const float* __restrict__ bi,
                             const float* __restrict__ g,   // (b,n,d,m)
                             float* __restrict__ dht,       // (b,n,d,m)
                             float* __restrict__ dw,        // (b,n,k,d)
                             float* __restrict__ dsc,       // (d)
                             float* __restrict__ dbi,       // (d)
                             long total, int n, int k, int d, int m,
                             float eps) {
    for (long t = (long)blockIdx.x * EG_NT + threadIdx.x; t < total;
         t += (long)gridDim.x * EG_NT) {
        long dd = t % d, r = t / d;
        long jj = r % k, r2 = r / k;
        long i = r2 % n, b = r2 / n;
        long j = idx[(b * n + i) * k + jj];
        const T* a = ht + ((b * n + i) * d + dd) * m;
        const T* c = ht + ((b * n + j) * d + dd) * m;
        const float* gr = g + ((b * n + i) * d + dd) * m;
        float rl[EG_MAXM], ss = 0.f, rg = 0.f;
        for (int mm = 0; mm < m; ++mm) {
            rl[mm] = (float)a[mm] - (float)c[mm];
            ss += rl[mm] * rl[mm];
            rg += rl[mm] * gr[mm];
        }
        const float u = sqrtf(ss);
        const float s_ = sc[dd], t_ = bi[dd];
        const float cden = fmaxf(u, eps);
        const float f = (u * s_ + t_) / cden;
        // f'(u), with the clamp's derivative handled piecewise
        const float fp = (u > eps) ? (-t_ / (u * u)) : (s_ / eps);
        const float wv = w[((b * n + i) * k + jj) * d + dd];
        // dw
        dw[((b * n + i) * k + jj) * d + dd] = rg * f;
        // dscale/dbias
        atomicAdd(&dsc[dd], wv * rg * u / cden);
        atomicAdd(&dbi[dd], wv * rg / cden);
        // drel -> dht_i (+) and dht_j (-)
        const float k2 = (u > 0.f) ? wv * fp * rg / u : 0.f;
        float* di = dht + ((b * n + i) * d + dd) * m;
        float* dj = dht + ((b * n + j) * d + dd) * m;
        for (int mm = 0; mm < m; ++mm) {
            const float dr = wv * f * gr[mm] + k2 * rl[mm];
            atomicAdd(&di[mm], dr);
            atomicAdd(&dj[mm], -dr);
        }
    }
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
static long eg_grid(long total) {
    long gb = (total + EG_NT - 1) / EG_NT;
    return gb > 1048576 ? 1048576 : gb;
}

void egnn_rel_dist_fwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor dist) {
    int b = ht.size(0), n = ht.size(1), d = ht.size(2), m = ht.size(3);
    int k = idx.size(2);
    TORCH_CHECK(ht.is_cuda() && ht.is_contiguous() && idx.is_contiguous() &&
                dist.is_contiguous() && m <= EG_MAXM);
    long total = (long)b * n * k * d;
    auto stream = at::cuda::getCurrentHIPStream();
    DISPATCH_F32_BF16(ht, __bf16, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(egnn_rel_dist_fwd_kernel<T>),
                           dim3(eg_grid(total)), dim3(EG_NT), 0, stream,
                           tptr<const T>(ht),
                           idx.data_ptr<long>(), dist.data_ptr<float>(),
                           total, n, k, d, m);
    });
    check_launch("egnn_rel_dist_fwd: ");
}

void egnn_rel_dist_bwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor gdist,
                       torch::Tensor dht) {
    int b = ht.size(0), n = ht.size(1), d = ht.size(2), m = ht.size(3);
    int k = idx.size(2);
    TORCH_CHECK(gdist.is_contiguous() && dht.is_contiguous() &&
                dht.dtype() == torch::kFloat32);
    long total = (long)b * n * k * d;
    auto stream = at::cuda::getCurrentHIPStream();
    DISPATCH_F32_BF16(ht, __bf16, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(egnn_rel_dist_bwd_kernel<T>),
                           dim3(eg_grid(total)), dim3(EG_NT), 0, stream,
                           tptr<const T>(ht),
                           idx.data_ptr<long>(), gdist.data_ptr<float>(),
                           dht.data_ptr<float>(), total, n, k, d, m);
    });
    check_launch("egnn_rel_dist_bwd: ");
}

void egnn_htype_update_fwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor w,
                           torch::Tensor sc, torch::Tensor bi,
                           torch::Tensor upd, double eps) {
    int b = ht.size(0), n = ht.size(1), d = ht.size(2), m = ht.size(3);
    int k = idx.size(2);
    TORCH_CHECK(ht.is_cuda() && ht.is_contiguous() && idx.is_contiguous() &&
                w.is_contiguous() && upd.is_contiguous() && m <= EG_MAXM);
    TORCH_CHECK(w.dtype() == torch::kFloat32 && sc.numel() == d && bi.numel() == d);
    long total = (long)b * n * d;
    auto stream = at::cuda::getCurrentHIPStream();
    DISPATCH_F32_BF16(ht, __bf16, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(egnn_htype_update_fwd_kernel<T>),
                           dim3(eg_grid(total)), dim3(EG_NT), 0, stream,
                           tptr<const T>(ht),
                           idx.data_ptr<long>(), w.data_ptr<float>(),
                           sc.data_ptr<float>(), bi.data_ptr<float>(),
                           upd.data_ptr<float>(), total, n, k, d, m, (float)eps);
    });
    check_launch("egnn_htype_update_fwd: ");
}

void egnn_htype_update_bwd(torch::Tensor ht, torch::Tensor idx, torch::Tensor w,
                           torch::Tensor sc, torch::Tensor bi, torch::Tensor g,
                           torch::Tensor dht, torch::Tensor dw,
                           torch::Tensor dsc, torch::Tensor dbi, double eps) {
    int b = ht.size(0), n = ht.size(1), d = ht.size(2), m = ht.size(3);
    int k = idx.size(2);
    TORCH_CHECK(g.is_contiguous() && dht.is_contiguous() && dw.is_contiguous());
    long total = (long)b * n * k * d;
    auto stream = at::cuda::getCurrentHIPStream();
    DISPATCH_F32_BF16(ht, __bf16, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(egnn_htype_update_bwd_kernel<T>),
                           dim3(eg_grid(total)), dim3(EG_NT), 0, stream,
                           tptr<const T>(ht),
                           idx.data_ptr<long>(), w.data_ptr<float>(),
                           sc.data_ptr<float>(), bi.data_ptr<float>(),
                           g.data_ptr<float>(), dht.data_ptr<float>(),
                           dw.data_ptr<float>(), dsc.data_ptr<float>(),
                           dbi.data_ptr<float>(), total, n, k, d, m, (float)eps);
    });
    check_launch("egnn_htype_update_bwd: ");
}
