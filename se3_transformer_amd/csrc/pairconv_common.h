// Building blocks shared by the pairconv kernels (pairconv.hip: forward;
// pairconv_bwd.hip: dh, dw, du). Everything here is used by at least two of
// them; what only one kernel needs stays next to that kernel.
#pragma once

#include "host_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
// 16 B load from an address that is only 8 B aligned (two OP=4 vectors)
typedef bf16x8 bf16x8_a8 __attribute__((aligned(8)));
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

#define KDIM 128   // radial hidden width = GEMM K
#define NT 512     // threads per block (8 waves) in all four kernels

// Padded o width OP(O) of the edge-major tensors U (miF, E, OP) bf16,
// G (mo, E, OP) bf16 and dU (miF, E, OP) bf16 or f32: all o of one (row, edge) are
// one aligned vector, and the pad lanes o in [O, OP) are exactly zero, so a
// consumer contracts whole vectors. The one definition; ops/fused.py mirrors
// it and checks pairconv_opad() at load.
__host__ __device__ constexpr int opad_of(int O) {
    return O == 1 ? 1 : (O <= 3 ? 4 : 8);
}

// Channel padding: the MFMA tiles are 8 mo x 32 urows, and the kernels serve
// any mo >= 1, miF >= 1 on tensors padded to mo_p = ceil_mo(mo) and
// miF_p = ceil_mif(miF) with exact zeros:
//
//   P_fwd, P_dh (packed W)  sized for (mo_p, miF_p); every row outside the
//                           true (mo, miF) is exactly zero (pack_w_both)
//   bias handed to du       mo_p*miF_p f32, zero outside
//   U   (miF_p, E, OP) bf16 rows >= miF exactly zero, written by the producer
//   G   (mo_p, E, OP) bf16  rows >= mo exactly zero, written by pack_g
//   dU  (miF_p, E, OP)      rows >= miF are written (zeros by construction)
//                           and ignored
//   out (E, mo, O), dW (mo*miF, 128), db (mo*miF), dH   TRUE sizes: fwd and dw
//                           guard their stores, nothing padded reaches autograd
//
// Zero W rows and zero bias give R = 0 on the pads, zero U and G rows give
// dR = 0 there, so the pads add exact zeros to out, dH and dU and the inner
// loops are those of the aligned case. The cost: U and dU grow by miF_p/miF
// and the MFMA work is done on the padded tile.
__host__ __device__ constexpr int ceil_mo(int mo) { return (mo + 7) / 8 * 8; }
__host__ __device__ constexpr int ceil_mif(int miF) { return (miF + 31) / 32 * 32; }

// The (row, edge) vector of an o-padded tensor: 16 B at OP=8, 8 B at OP=4.
// O=1 has no vector form (its layout is the plain [row][E] the kernels
// always used); OVec<1> only keeps the O=1 instantiations well-formed.
template <int OP> struct OVec { typedef bf16x8 type; };
template <> struct OVec<4> { typedef bf16x4 type; };

template <int OP>
__device__ __forceinline__ typename OVec<OP>::type
load_ovec(const __bf16* __restrict__ T, size_t row, int e, int E) {
    typedef typename OVec<OP>::type V;
    if (e < E) return *reinterpret_cast<const V*>(T + (row * E + e) * OP);
    return V(0);
}

// sum_o a[o] b[o] over one padded vector: OP/2 v_dot2_f32_bf16.
template <int OP>
__device__ __forceinline__ float dot_ovec(typename OVec<OP>::type a,
                                          typename OVec<OP>::type b) {
    const bf16x2* a2 = reinterpret_cast<const bf16x2*>(&a);
    const bf16x2* b2 = reinterpret_cast<const bf16x2*>(&b);
    float acc = 0.f;
#pragma unroll
    for (int p = 0; p < OP / 2; ++p)
        acc = __builtin_amdgcn_fdot2_f32_bf16(a2[p], b2[p], acc, false);
    return acc;
}

__device__ __forceinline__ float b2f(__bf16 x) { return (float)x; }

__device__ __forceinline__ f32x2 b2f2(bf16x2 v) {
    return f32x2{(float)v[0], (float)v[1]};
}

// 8 consecutive edges e..e+7 of one e-contiguous row (Ut, Gt, Ht rows are
// E long and in general not 16B aligned): one full vector when the run is
// inside E, element by element with zero fill across the ragged end.
// Used by the O=1 instantiations of fwd and dh, whose [row][E] tensors are
// not o-padded.
__device__ __forceinline__ bf16x8 load_edges8(const __bf16* __restrict__ row,
                                              int e, int E) {
    const __bf16* src = row + e;
    if (e + 8 <= E) return *reinterpret_cast<const bf16x8*>(src);
    bf16x8 v(0);
    for (int j = 0; j < 8; ++j)
        if (e + j < E) v[j] = src[j];
    return v;
}

// Scatter 8 edges of (row, o) into an LDS tile laid out [row][64 e][o PADDED
// to 8], so the consumer reads all o of one (row, e) as a single 16B vector.
// The pad lanes o in [O, 8) are zeroed once by the caller and never written.
// Only the O=1 instantiations of fwd and dh still stage this way.
__device__ __forceinline__ void commit_opad(__bf16* tile, int row, int eu,
                                            int o, bf16x8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        tile[((size_t)row * 64 + eu + j) * 8 + o] = v[j];
}

// Stage the (64 e x 128 k) H tile of edge block e0 into LDS, rows past E
// zero-filled. The 16B slots of a row are XOR-swizzled by (e & 15) so the
// MFMA B-fragment reads in mfma_rtile are bank-conflict free.
__device__ __forceinline__ void stage_h_tile(__bf16* h_lds,
                                             const __bf16* __restrict__ H,
                                             int e0, int E, int tid) {
    for (int i = tid; i < (64 * KDIM) / 8; i += NT) {   // 16B units
        int e = i >> 4;             // 16 units per row
        int k16 = i & 15;           // 16B slot
        int dst = e * 256 + ((k16 * 16) ^ ((e & 15) << 4));
        bf16x8 v;
        if (e0 + e < E) {
            v = *reinterpret_cast<const bf16x8*>(H + (size_t)(e0 + e) * KDIM + k16 * 8);
        } else {
            v = bf16x8(0);
        }
        *reinterpret_cast<bf16x8*>(reinterpret_cast<char*>(h_lds) + dst) = v;
    }
}

// Fragment f (= mf*4 + kit) of one wave's 16 A-fragments in the packed W
// [mo/8][miF/32][wm4][mf4][kit4][lane64][8]; pbase already includes lane*8.
__device__ __forceinline__ bf16x8 load_wfrag(const __bf16* pbase, int f) {
    return *reinterpret_cast<const bf16x8*>(pbase + (size_t)f * 64 * 8);
}

// R^T tile GEMM: acc = W-fragments (256 n x K=128) @ H tile (K x 64 e).
// Wave (wm, we) owns n-rows wm*64..+64 (4 frags mf) x e-cols we*32..+32
// (2 frags ef). afrag(mf, kit) supplies the A operand: straight from global
// (load_wfrag) or out of a prefetched register array.
template <class AFrag>
__device__ __forceinline__ void mfma_rtile(f32x4 (&acc)[4][2], const __bf16* h_lds,
                                           int we, int l15, int l4, AFrag afrag) {
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int ef = 0; ef < 2; ++ef) acc[mf][ef] = f32x4(0.f);
#pragma unroll
    for (int kit = 0; kit < 4; ++kit) {
        const int k0 = kit * 32 + l4 * 8;
        bf16x8 a[4], b[2];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) a[mf] = afrag(mf, kit);
#pragma unroll
        for (int ef = 0; ef < 2; ++ef) {
            int e = we * 32 + ef * 16 + l15;
            int byte = e * 256 + ((k0 * 2) ^ ((e & 15) << 4));
            b[ef] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(h_lds) + byte);
        }
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
#pragma unroll
            for (int ef = 0; ef < 2; ++ef)
                acc[mf][ef] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mf], b[ef], acc[mf][ef], 0, 0, 0);
    }
}

// Block index -> (edge block eb, W-slice group grp). With coh set (the group
// count is a multiple of 8) blockIdx & 7, which the dispatcher maps to the
// XCD, picks the group within a cohort of 8: all concurrently-resident
// blocks on one XCD share a group, so its packed-W slice stays in that XCD's
// L2 while the edge blocks stream past.
__device__ __forceinline__ void cohort_map(int coh, int nmemb, int& eb, int& grp) {
    if (coh) {
        int x = blockIdx.x & 7, r = blockIdx.x >> 3;
        eb = r % nmemb;
        grp = x + 8 * (r / nmemb);
    } else {
        eb = blockIdx.x % nmemb;
        grp = blockIdx.x / nmemb;
    }
}
