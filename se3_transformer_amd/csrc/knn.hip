// On-device k-NN graph construction (reference se3_transformer_pytorch.py
// :1221-1294): replaces the dense (b,n,n,3) rel-pos tensor, the self-removal
// gathers, the norm, the masked topk and the three neighbor gathers with one
// kernel. One wave per query node: each lane keeps a sorted top-L list of
// its strided j-candidates in LDS (L = min(k, ceil(n/64)) — a lane can
// never contribute more than its own candidate count), then the 64 lists
// are merged across lanes: a round takes every list head below the wave-wide
// minimum of the lists' second entries (about ten winners per round on
// random points), falls back to a single cross-lane argmin on a tie, and
// the merge stops as soon as no lane has a candidate left; the k winners'
// relative geometry and validity mask are written directly, 64 slots per
// pass.
//
// Any 1 <= k <= n-1 is served. The only ceiling is the block's dynamic LDS,
// L*64*8 bytes of lists plus 4*k of winners, which has to fit the
// KNN_MAX_LDS_BYTES a launch gets without raising the kernel's LDS
// attribute: at k = n-1 that is ~12 bytes per point, n up to ~5400.
//
// Selection semantics match the eager path exactly (:1250-1283):
//   * self excluded; causal keeps only j < i (overrides everything);
//   * `allow` (the user neighbor_mask, (b,n,n)) removes candidates from
//     selection (eager gives them +max distance => only unmaskable
//     padding, which comes out mask=0 either way);
//   * `sparse` (attend_sparse_neighbors adjacency, (b,n,n)) gives its
//     candidates priority distance 0 and exempts them from the radius
//     test — and from `allow`, as in the eager fill order;
//   * the node validity mask ANDs into the output mask only.
// Invalid slots emit index 0/1 with ZERO geometry (consumers that ignore
// the mask see no fabricated edge).

#include <hip/hip_runtime.h>
#include "host_common.h"
#include "ops.h"

// dynamic LDS a launch may ask for without hipFuncSetAttribute; mirrored by
// KNN_MAX_LDS in ops/fused.py and checked against it when the extension loads
#define KNN_MAX_LDS_BYTES 65536

__global__ void __launch_bounds__(64)
knn_kernel(const float* __restrict__ coors,        // (b, n, 3)
           const unsigned char* __restrict__ nmask, // (b, n) or nullptr
           const unsigned char* __restrict__ allow, // (b, n, n) or nullptr
           const unsigned char* __restrict__ sparse,// (b, n, n) or nullptr
           long* __restrict__ out_idx,              // (b, n, k)
           float* __restrict__ out_dist,            // (b, n, k)
           float* __restrict__ out_rel,             // (b, n, k, 3)
           unsigned char* __restrict__ out_m,       // (b, n, k)
           int b, int n, int k, int L, float radius, int causal) {
    extern __shared__ __attribute__((aligned(8))) char smem[];
    float* ld = reinterpret_cast<float*>(smem);            // [L][64]
    int* li = reinterpret_cast<int*>(smem + (size_t)L * 64 * 4); // [L][64]
    int* sel = reinterpret_cast<int*>(smem + (size_t)L * 64 * 8); // [k]

    const int lane = threadIdx.x & 63;
    const long q = blockIdx.x;                   // query row = bi*n + i
    if (q >= (long)b * n) return;
    const int bi = (int)(q / n), i = (int)(q % n);

    const float xi = coors[q * 3], yi = coors[q * 3 + 1], zi = coors[q * 3 + 2];
    const unsigned char* arow = allow ? allow + q * n : nullptr;
    const unsigned char* srow = sparse ? sparse + q * n : nullptr;

    int cnt = 0;  // entries in this lane's list (sorted ascending by eff)
    for (int s = 0; s < L; ++s) { ld[(size_t)s * 64 + lane] = 3.0e38f; li[(size_t)s * 64 + lane] = 0; }
    for (int j = lane; j < n; j += 64) {
        if (j == i) continue;
        if (causal && j >= i) continue;
        const bool sp = srow && srow[j];
        if (!sp && arow && arow[j] == 0) continue;
        float eff = 0.f;
        if (!sp) {
            float dx = xi - coors[((long)bi * n + j) * 3];
            float dy = yi - coors[((long)bi * n + j) * 3 + 1];
            float dz = zi - coors[((long)bi * n + j) * 3 + 2];
            eff = dx * dx + dy * dy + dz * dz;
        }
        if (cnt == L && eff >= ld[(size_t)(L - 1) * 64 + lane]) continue;
        // insertion sort (ascending)
        int p = (cnt < L) ? cnt : L - 1;
        while (p > 0 && ld[(size_t)(p - 1) * 64 + lane] > eff) {
            ld[(size_t)p * 64 + lane] = ld[(size_t)(p - 1) * 64 + lane];
            li[(size_t)p * 64 + lane] = li[(size_t)(p - 1) * 64 + lane];
            --p;
        }
        ld[(size_t)p * 64 + lane] = eff;
        li[(size_t)p * 64 + lane] = j;
        if (cnt < L) ++cnt;
    }

    // merge the 64 sorted lists into sel[0..k) in (eff, lane) order. A round
    // takes every head that lies below t, the wave-wide minimum of the
    // lists' SECOND entries: nothing behind a head is smaller than t, so
    // those heads are exactly the next winners, and each one's slot is its
    // rank among them. When no head is below t (the smallest head ties with
    // t, or nothing is left) the round falls back to one cross-lane argmin
    // over the heads, which takes one winner or ends the merge. Every branch
    // below is wave-uniform; each round adds at least one winner or breaks.
    int head = 0;
    int r = 0;
    while (r < k) {
        float v = (head < cnt) ? ld[(size_t)head * 64 + lane] : 3.0e38f;
        float t = (head + 1 < cnt) ? ld[(size_t)(head + 1) * 64 + lane] : 3.0e38f;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t = fminf(t, __shfl_xor(t, off));
        const bool win = v < t;
        unsigned long long winners = __ballot(win);
        if (winners == 0ull) {
            int l = lane;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                float ov = __shfl_xor(v, off);
                int ol = __shfl_xor(l, off);
                if (ov < v || (ov == v && ol < l)) { v = ov; l = ol; }
            }
            // v is wave-uniform after the butterfly. The sentinel means no
            // candidate is left anywhere (causal rows, rows thinned by
            // `allow`, k = n-1 past the real candidates): every later round
            // would find the same, so stop; the rest is marked invalid below.
            if (!(v < 3.0e38f)) break;
            if (lane == l) {
                sel[r] = li[(size_t)head * 64 + lane];
                ++head;
            }
            ++r;
            continue;
        }
        const int nwin = __popcll(winners);
        int rank = 0;
        while (winners) {
            const int s = __ffsll(winners) - 1;
            winners &= winners - 1;
            const float vs = __int_as_float(
                __builtin_amdgcn_readlane(__float_as_int(v), s));
            rank += (vs < v || (vs == v && s < lane)) ? 1 : 0;
        }
        if (win) {
            if (r + rank < k) sel[r + rank] = li[(size_t)head * 64 + lane];
            ++head;
        }
        r += nwin;
    }
    if (r > k) r = k;
    for (int s = r + lane; s < k; s += 64) sel[s] = -1;
    __builtin_amdgcn_wave_barrier();

    // write the selected neighbors' geometry + validity, 64 slots per pass
    for (int s = lane; s < k; s += 64) {
        int j = sel[s];
        bool valid = j >= 0;
        if (!valid) j = (i == 0) ? (n > 1 ? 1 : 0) : 0;  // any real node != i
        float dx = 0.f, dy = 0.f, dz = 0.f, d = 0.f;
        bool sp = false;
        if (valid) {
            dx = xi - coors[((long)bi * n + j) * 3];
            dy = yi - coors[((long)bi * n + j) * 3 + 1];
            dz = zi - coors[((long)bi * n + j) * 3 + 2];
            d = sqrtf(dx * dx + dy * dy + dz * dz);
            sp = srow && srow[j];
        }
        long o = q * k + s;
        out_idx[o] = j;
        out_dist[o] = d;
        out_rel[o * 3] = dx;
        out_rel[o * 3 + 1] = dy;
        out_rel[o * 3 + 2] = dz;
        unsigned char ok = valid && (sp || d <= radius);
        if (nmask != nullptr)
            ok = ok & nmask[(long)bi * n + i] & nmask[(long)bi * n + j];
        out_m[o] = ok;
    }
}

static const unsigned char* knn_opt_u8(const torch::Tensor& t) {
    if (t.defined() && t.numel() > 0) {
        TORCH_CHECK(t.dtype() == torch::kUInt8 && t.is_contiguous());
        return t.data_ptr<unsigned char>();
    }
    return nullptr;
}

int64_t knn_max_lds_bytes() { return KNN_MAX_LDS_BYTES; }

void knn_graph(torch::Tensor coors, torch::Tensor nmask, torch::Tensor allow,
               torch::Tensor sparse, torch::Tensor idx,
               torch::Tensor dist, torch::Tensor rel, torch::Tensor m,
               int64_t k, double radius, bool causal) {
    TORCH_CHECK(coors.is_cuda() && coors.dtype() == torch::kFloat32 &&
                coors.is_contiguous());
    int b = coors.size(0), n = coors.size(1);
    TORCH_CHECK(k >= 1 && k <= n - 1, "knn_graph: need 1 <= k <= n-1, got n=",
                n, " k=", k);
    TORCH_CHECK(idx.is_contiguous() && dist.is_contiguous() &&
                rel.is_contiguous() && m.is_contiguous());
    TORCH_CHECK(idx.numel() == (int64_t)b * n * k && dist.numel() == idx.numel() &&
                m.numel() == idx.numel() && rel.numel() == 3 * idx.numel(),
                "knn_graph: outputs must be (b,n,k) / (b,n,k,3)");
    int L = (int)std::min<long>(k, (n + 63) / 64);
    size_t lds = (size_t)L * 64 * 8 + 4 * (size_t)k;
    TORCH_CHECK(lds <= KNN_MAX_LDS_BYTES, "knn_graph: n=", n, " k=", k,
                " needs ", lds, " bytes of LDS per block, the limit is ",
                KNN_MAX_LDS_BYTES);
    auto stream = at::cuda::getCurrentHIPStream();
    dim3 grid((long)b * n);
    hipLaunchKernelGGL(knn_kernel, grid, dim3(64), lds, stream,
                       coors.data_ptr<float>(), knn_opt_u8(nmask),
                       knn_opt_u8(allow), knn_opt_u8(sparse),
                       idx.data_ptr<long>(),
                       dist.data_ptr<float>(), rel.data_ptr<float>(),
                       m.data_ptr<unsigned char>(), b, n, (int)k, L,
                       (float)radius, causal ? 1 : 0);
    check_launch("knn_graph: ");
}
