// Backward kernels for the fused pairwise convolution (see pairconv.hip).
//
//   R[e,n]  = H[e,:] . W[n,:] + bias[n],   n = (mo, c),  c = (mi,f) "urow"
//   out[e,mo,o] = sum_c R[e,(mo,c)] * u[c,e,o]
//
// u, g and du are o-padded and edge-major (OP = opad_of(O), pads zero):
//   U (miF, E, OP) bf16 | G (mo, E, OP) bf16 (pack_g) | dU (miF, E, OP) bf16 or f32
// Here mo and miF are the PADDED mo_p, miF_p of pairconv_common.h: the pad
// rows of U, G, the packed W and the bias are zero, so dh and du run on them
// as they are. Only dw writes tensors of the true sizes, and guards them.
// so every kernel stages whole (row, edge) vectors with plain copies. At
// O=1 that layout is the [row][E] the kernels always read, and the O=1
// instantiations stage as they always did.
//
// Gradients (g = dL/dout):
//   dR[e,n]   = sum_o g[mo,e,o] * u[c,e,o]          (v_dot2, recomputed on the fly)
//   dH[e,k]   = sum_n dR[e,n] * W[n,k]              (kernel B1, MFMA, needs W^T)
//   dW[n,k]   = sum_e dR[e,n] * H[e,k]              (kernel B2, MFMA, needs H^T)
//   db[n]     = sum_e dR[e,n]                       (kernel B2, f32 sums of its dR entries)
//   du[c,e,o] = sum_mo R[e,(mo,c)] * g[mo,e,o]      (kernel B3, recomputes R)
//
// dR / R are never written to global memory anywhere.

#include <hip/hip_runtime.h>
#include "pairconv_common.h"
#include "ops.h"

// ---------------------------------------------------------------------------
// B1: dH[e,k] = sum_n dR[e,n] W[n,k]
// block: 64 e x 128 k, loops (urow-chunk 32) x (mo-block 8) over its n; a
// tile is 64 e x 256 n x 128 k. The W fragments come packed (P1) so the MFMA
// operand of a lane (8 consecutive n at fixed k) is one 16 B load.
//
// dR build: a thread owns e = lane and the run of 8 urows c = 8 (wid & 3)..
// of the chunk, and keeps those eight u[c][e] vectors in registers for all
// tiles of the chunk: u never goes through LDS. Per tile it contracts them
// with the g vectors of its four m = (wid >> 2) + 2 it (v_dot2_f32_bf16) and
// writes one swizzled 16 B run of the [64 e][256 n] bf16 dR tile per m. The
// next chunk's u is loaded into the same registers right after the last
// build of a chunk, ahead of that tile's W loads: it is in flight together
// with them and under the MFMA phase, and costs no second set of registers.
// O=1 has no o-vector and keeps its u chunk in LDS ([row][E] tensors
// scattered into 8-wide slots), 8 KiB more.
//
// MFMA phase: wave wid owns all 64 e x the 16 k of fragment wid of P1's
// [wk2][kf4], so every W fragment is fetched once per block (32 KiB of the
// 64 KiB tile per SIMD pair, not four times over) and meets four dR
// fragments from LDS. The W fragments sit in an explicit ring four n-steps
// deep (16 VGPRs); eight deep spilled at O >= 5. Every (e, k) sum runs over
// the n-steps of a tile and over the tiles in the one order it always had,
// so with nsplit = 1 dH is bit for bit what the (we4, wk2) mapping gave.
// LDS: dR 32 KiB + g 8 KiB at OP = 8: two blocks per CU by LDS and by the
// 128-VGPR cap (profiles/dh_wshare.md).
// ---------------------------------------------------------------------------
#define DH_RD 4   // W ring depth, n-steps

template <int O>
__global__ void __launch_bounds__(NT, 4)   // cap VGPR<=128: 2 blocks/CU
pairconv_bwd_dh_kernel(const __bf16* __restrict__ Gt,  // (mo, E, OP) bf16
                       const __bf16* __restrict__ Ut,  // (miF, E, OP) bf16
                       const __bf16* __restrict__ P1,  // packed W: [mo/8][miF/32][wk2][kf4][ns8][lane64][8]
                       float* __restrict__ dH,         // (E, 128) f32 (zeroed)
                       int E, int mo, int miF, int nsplit, int nmemb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the g tile (and at O=1 the u chunk) is [row][e][o PADDED to LP], as in
    // memory: the dR build reads ONE vector per (row, e) and contracts with
    // v_dot2_f32_bf16 — no scalar LDS reads, no bf16->f32 conversion ops.
    constexpr int LP = (O == 1) ? 8 : opad_of(O);
    constexpr bool UREG = O != 1;     // u of a chunk in registers
    typedef typename OVec<LP>::type ovec;
    __bf16* dr_lds = reinterpret_cast<__bf16*>(smem);                 // [64e][256n] 32 KiB
    __bf16* g_lds = reinterpret_cast<__bf16*>(smem + 32768);          // [8][64][LP]
    __bf16* u_lds = g_lds + 8 * 64 * LP;                              // [32][64][8], O=1 only

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // the wave index as a scalar: the W-fragment addresses are a scalar base
    // plus one lane offset
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15;
    const int l4 = lane >> 4;
    // panel mapping: the grid is cut into panels of PS split-slices x PE
    // e-blocks, numbered e-block fastest, so the blocks in flight together
    // re-read the packed-W of few split-slices and the u/g tiles of few
    // edge blocks. The launcher rounds the grid up to whole panels.
    const int PS = 4, PE = 128;
    int panels_x = (nmemb + PE - 1) / PE;
    int within = blockIdx.x % (PS * PE);
    int panel = blockIdx.x / (PS * PE);
    int eb = (panel % panels_x) * PE + within % PE;
    int sp = (panel / panels_x) * PS + within / PE;
    if (eb >= nmemb || sp >= nsplit) return;
    const int e0 = eb * 64;

    f32x4 acc[4];                      // 64 e (4 fragments) x 16 k per wave
#pragma unroll
    for (int ef = 0; ef < 4; ++ef) acc[ef] = {0.f, 0.f, 0.f, 0.f};

    const int nmo = mo / 8, nuc = miF / 32;
    const int mb_lo = (nmo / nsplit) * sp;
    const int mb_hi = mb_lo + nmo / nsplit;

    // T14 register staging: the next g tile (every mb) loads under the dR +
    // MFMA phases. A staging unit is one (row, e) vector; at O=1 it is 8
    // edges of one row.
    constexpr int GTOT = (O == 1) ? (8 * 64) / 8 : 8 * 64;      // g tile units (<= NT)
    constexpr int UTOT1 = (32 * 64) / 8;                        // u chunk units at O=1 (<= NT)
    ovec g_reg;
    auto ld_unit = [&](const __bf16* __restrict__ T, int row0, int i) -> ovec {
        if constexpr (O == 1)
            return load_edges8(T + (size_t)(row0 + (i >> 3)) * E, e0 + (i & 7) * 8, E);
        else
            return load_ovec<LP>(T, (size_t)(row0 + (i >> 6)), e0 + (i & 63), E);
    };
    auto st_unit = [&](__bf16* tile, int i, ovec v) {
        if constexpr (O == 1) commit_opad(tile, i >> 3, (i & 7) * 8, 0, v);
        else *reinterpret_cast<ovec*>(tile + (size_t)i * LP) = v;
    };
    auto load_g = [&](int mb) {
        if (tid < GTOT) g_reg = ld_unit(Gt, mb * 8, tid);
    };
    // u: the thread's own eight vectors (e = lane, c = crun + j), bare
    // predicated loads into registers zeroed once (a thread's edge is in or
    // out of range for the whole kernel). At O=1 one staged unit of the
    // chunk, committed to u_lds at the top of the chunk.
    constexpr int NU = UREG ? 8 : 1;
    ovec u[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) u[j] = ovec(0);
    const int crun = (wid & 3) * 8;
    const bool e_in = e0 + lane < E;
    auto load_u = [&](int cb) {
        if constexpr (UREG) {
            if (e_in) {
                const __bf16* up = Ut + ((size_t)(cb * 32 + crun) * E + e0 + lane) * LP;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    u[j] = *reinterpret_cast<const ovec*>(up + (size_t)j * E * LP);
            }
        } else {
            if (tid < UTOT1) u[0] = ld_unit(Ut, cb * 32, tid);
        }
    };
    load_u(0);
    load_g(mb_lo);
    if constexpr (O == 1) {   // pad lanes of the scatter slots, cleared once
        for (int i = tid; i < (8 + 32) * 64; i += NT)
            *reinterpret_cast<bf16x8*>(g_lds + (size_t)i * 8) = bf16x8(0);
    }

    for (int cb = 0; cb < nuc; ++cb) {
        if constexpr (!UREG) {
            // commit the staged u chunk [urow][e][8]
            __syncthreads();
            if (tid < UTOT1) st_unit(u_lds, tid, u[0]);
            if (cb + 1 < nuc) load_u(cb + 1);
        }
        for (int mb = mb_lo; mb < mb_hi; ++mb) {
            // commit the staged g tile [m][e][LP]
            if (tid < GTOT) st_unit(g_lds, tid, g_reg);
            load_g(mb + 1 < mb_hi ? mb + 1 : mb_lo);   // next mb (or next cb's first)
            __syncthreads();
            // cooperative dR tile [64e][256n]: thread owns (e, run of 8 n);
            // per n: one g vector (shared over the run) dot one u vector
            // via LP/2 v_dot2_f32_bf16; one swizzled b128 write per run.
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int e = lane, n8 = wid + 8 * it;
                const int m = n8 >> 2;
                ovec g8 = *reinterpret_cast<const ovec*>(
                    g_lds + ((size_t)m * 64 + e) * LP);
                __bf16 v0[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ovec u8;
                    if constexpr (UREG) u8 = u[j];
                    else u8 = *reinterpret_cast<const ovec*>(
                        u_lds + ((size_t)(crun + j) * 64 + e) * LP);
                    v0[j] = (__bf16)dot_ovec<LP>(g8, u8);
                }
                *reinterpret_cast<bf16x8*>(reinterpret_cast<char*>(dr_lds)
                    + e * 512 + (((n8 ^ (e & 15)) << 4))) = *reinterpret_cast<bf16x8*>(v0);
            }
            if constexpr (UREG) {
                // the chunk's last build is done with u: fetch the next chunk's
                if (mb + 1 == mb_hi && cb + 1 < nuc) load_u(cb + 1);
            }
            __syncthreads();
            // MFMA: dH_tile += dR(64e x 256n) @ W(256n x 128k); this wave's
            // fragment wid of [wk2][kf4], n-step ns
            const __bf16* pbase = P1 + (((size_t)mb * (miF / 32) + cb) * 8 + wid) * 8 * 64 * 8
                                  + (size_t)lane * 8;
            bf16x8 w[DH_RD];
#pragma unroll
            for (int s = 0; s < DH_RD; ++s)
                w[s] = *reinterpret_cast<const bf16x8*>(pbase + (size_t)s * 64 * 8);
#pragma unroll
            for (int ns = 0; ns < 8; ++ns) {      // 8 n-steps of 32
                // A: dR rows e = ef*16 + l15, n = ns*32 + l4*8.. (tile n index
                // = m*32+c; global n = (mb*8+m)*miF + cb*32 + c). The swizzle
                // is by l15 alone, so the four reads differ by whole rows.
                bf16x8 a[4];
#pragma unroll
                for (int ef = 0; ef < 4; ++ef)
                    a[ef] = *reinterpret_cast<const bf16x8*>(
                        reinterpret_cast<char*>(dr_lds) + (ef * 16 + l15) * 512
                        + (((ns * 4 + l4) ^ l15) << 4));
#pragma unroll
                for (int ef = 0; ef < 4; ++ef)
                    acc[ef] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        w[ns % DH_RD], a[ef], acc[ef], 0, 0, 0);
                if (ns + DH_RD < 8)
                    w[ns % DH_RD] = *reinterpret_cast<const bf16x8*>(
                        pbase + (size_t)(ns + DH_RD) * 64 * 8);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // mfma(X = W fragment: rows k, contraction n; Y = dR: contraction n, cols e)
    // => D rows = k, cols = e: row = l4*4+reg (k), col = l15 (e).
#pragma unroll
    for (int ef = 0; ef < 4; ++ef)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            int k = wid * 16 + l4 * 4 + reg;
            int e = e0 + ef * 16 + l15;
            if (e < E) atomicAdd(&dH[(size_t)e * KDIM + k], acc[ef][reg]);
        }
}

// ---------------------------------------------------------------------------
// B2 pieces shared by the dw kernel and its O=1 form: the H^T chunk load, the
// MFMA step over one 32-edge chunk and the dW tile write.
// ---------------------------------------------------------------------------
// spelled out, not load_edges8: with the helper the compiler schedules dw
// differently and it measured slower (+1.3 % at O=5; profiles/pairconv_prune.md)
__device__ __forceinline__ bf16x8 dw_load_h(const __bf16* __restrict__ Ht, int E,
                                            int e0, int tid) {
    int k = tid >> 2, eu = (tid & 3) * 8;
    const __bf16* src = Ht + (size_t)k * E + e0 + eu;
    bf16x8 h(0);
    if (e0 + eu + 8 <= E) h = *reinterpret_cast<const bf16x8*>(src);
    else { for (int j = 0; j < 8; ++j) h[j] = (e0 + eu + j < E) ? src[j] : (__bf16)0.f; }
    return h;
}

// dW_tile += dR^T(128n x 32e) @ H(32e x 128k); wave (wn, wk) owns 32 n x 64 k
__device__ __forceinline__ void dw_mfma_chunk(f32x4 (&acc)[2][4], const __bf16* dr_lds,
                                              const __bf16* h_lds, int wn, int wk,
                                              int l15, int l4) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(
            dr_lds + (size_t)(wn * 32 + nf * 16 + l15) * 32 + l4 * 8);
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) {
            bf16x8 b = *reinterpret_cast<const bf16x8*>(
                h_lds + (size_t)(wk * 64 + kf * 16 + l15) * 32 + l4 * 8);
            acc[nf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nf][kf], 0, 0, 0);
        }
    }
}

// D rows = n ((l4*4+reg within frag)), cols = k (l15). mo and miF are the
// true sizes of dW (mo*miF, 128); with RAG the tile may reach past either and
// the rows that do not exist are not stored.
template <bool RAG>
__device__ __forceinline__ void dw_write_tile(float* __restrict__ dW, const f32x4 (&acc)[2][4],
                                              int mb, int cb, int mo, int miF, int wn, int wk,
                                              int l15, int l4) {
    const size_t nbase = (size_t)(mb * 4) * miF + cb * 32;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                int ntile = wn * 32 + nf * 16 + l4 * 4 + reg;
                int m = ntile >> 5, c = ntile & 31;
                int k = wk * 64 + kf * 16 + l15;
                if (RAG && !(mb * 4 + m < mo && cb * 32 + c < miF)) continue;
                dW[(nbase + (size_t)m * miF + c) * KDIM + k] = acc[nf][kf][reg];
            }
}

// db[n] = sum_e dR[e,n] of the tile's rows n = (m, uc), m < 4: s[m] is this
// thread's sum over its e-pair of every chunk; the 16 threads of one uc are
// consecutive lanes. The block owns its rows, so the store is exclusive.
template <bool RAG>
__device__ __forceinline__ void dw_write_db(float* __restrict__ db, const float (&s)[4],
                                            int mb, int cb, int mo, int miF, int tid) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float v = s[m];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
        if ((tid & 15) == 0 &&
            (!RAG || (mb * 4 + m < mo && cb * 32 + (tid >> 4) < miF)))
            db[(size_t)(mb * 4 + m) * miF + cb * 32 + (tid >> 4)] = v;
    }
}

// ---------------------------------------------------------------------------
// B2: dW[n,k] = sum_e dR[e,n] H[e,k];  db[n] = sum_e dR[e,n]
// block: n-tile 128 (4 mo x 32 urow) x 128 k, loops e in chunks of 32.
// Ht is H transposed: (128, E) bf16.
//
// dR^T build: thread (c = tid >> 4, e-pair = tid & 15) keeps its two u
// vectors u[c][e], u[c][e+1] in the T14 staging registers — u never goes
// through LDS, each vector is loaded once — and contracts them with the four
// g[m][e], g[m][e+1] pairs of the tile by v_dot2_f32_bf16: 8 dR entries per
// thread, stored as four 4-byte e-pairs into the [128 n][32 e] MFMA image
// (a wave's stores cover 4 whole 64 B rows: conflict-free). Only the
// 4 x 32 g vectors and the H^T tile are staged in LDS.
// With DB the thread also sums its f32 dR entries, before their bf16
// rounding, into db (dw_write_db); without it the kernel is what it was.
// mo and miF are the true sizes of dW and db; G and U have the padded rows.
// RAG: mo % 4 or miF % 32 is nonzero and the stores are guarded.
// ---------------------------------------------------------------------------
template <int O, bool DB, bool RAG>
__global__ void __launch_bounds__(NT)
pairconv_bwd_dw_kernel(const __bf16* __restrict__ Gt,  // (mo, E, OP)
                       const __bf16* __restrict__ Ut,  // (miF, E, OP)
                       const __bf16* __restrict__ Ht,  // (128, E)
                       float* __restrict__ dW,         // (mo*miF, 128) f32
                       float* __restrict__ db,         // (mo*miF,) f32, DB only
                       int E, int mo, int miF) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int OP = opad_of(O);
    typedef typename OVec<OP>::type ovec;
    __bf16* dr_lds = reinterpret_cast<__bf16*>(smem);                  // [128n][32e] 8 KiB
    __bf16* h_lds = reinterpret_cast<__bf16*>(smem + 8192);            // [128k][32e] 8 KiB
    __bf16* g_lds = reinterpret_cast<__bf16*>(smem + 16384);           // [4][32][OP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l15 = lane & 15;
    const int l4 = lane >> 4;
    const int wn = wid >> 1;          // 0..3: n-group of 32
    const int wk = wid & 1;           // 0..1: k-group of 64
    const int ncb = RAG ? (miF + 31) / 32 : miF / 32;
    const int mb = blockIdx.x / ncb;            // mo-block (4 mo each)
    const int cb = blockIdx.x % ncb;            // urow chunk
    const int uc = tid >> 4;          // 0..31: this thread's urow in the chunk
    const int ue = (tid & 15) * 2;    // its e-pair in the 32-edge chunk

    f32x4 acc[2][4];                  // wave: 32 n x 64 k
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    // T14 register-staged pipeline: chunk ec+1's global loads are issued
    // right after chunk ec's LDS image is written, so HBM/L2 latency hides
    // under the dR + MFMA phase instead of serializing each chunk.
    ovec u_reg[2], g_reg;
    bf16x8 h_reg;
    const int nec = (E + 31) / 32;

    auto load_chunk = [&](int ec) {
        const int e0 = ec * 32;
        u_reg[0] = load_ovec<OP>(Ut, (size_t)(cb * 32 + uc), e0 + ue, E);
        u_reg[1] = load_ovec<OP>(Ut, (size_t)(cb * 32 + uc), e0 + ue + 1, E);
        if (tid < 4 * 32)
            g_reg = load_ovec<OP>(Gt, (size_t)(mb * 4 + (tid >> 5)), e0 + (tid & 31), E);
        h_reg = dw_load_h(Ht, E, e0, tid);
    };

    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    load_chunk(0);
    for (int ec = 0; ec < nec; ++ec) {
        __syncthreads();   // previous MFMA done reading the LDS images
        const ovec u0 = u_reg[0], u1 = u_reg[1];
        if (tid < 4 * 32)
            *reinterpret_cast<ovec*>(g_lds + (size_t)tid * OP) = g_reg;
        {
            int k = tid >> 2, eu = (tid & 3) * 8;
            *reinterpret_cast<bf16x8*>(h_lds + (size_t)k * 32 + eu) = h_reg;
        }
        if (ec + 1 < nec) load_chunk(ec + 1);   // issue next loads early
        __syncthreads();
        // dR^T tile [128n][32e]: this thread's (c, e-pair) against 4 mo
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            ovec g0 = *reinterpret_cast<const ovec*>(g_lds + (size_t)(m * 32 + ue) * OP);
            ovec g1 = *reinterpret_cast<const ovec*>(g_lds + (size_t)(m * 32 + ue + 1) * OP);
            const float d0 = dot_ovec<OP>(g0, u0), d1 = dot_ovec<OP>(g1, u1);
            if constexpr (DB) dbs[m] += d0 + d1;
            *reinterpret_cast<bf16x2*>(dr_lds + (size_t)(m * 32 + uc) * 32 + ue) =
                bf16x2{(__bf16)d0, (__bf16)d1};
        }
        __syncthreads();
        dw_mfma_chunk(acc, dr_lds, h_lds, wn, wk, l15, l4);
    }
    __syncthreads();
    dw_write_tile<RAG>(dW, acc, mb, cb, mo, miF, wn, wk, l15, l4);
    if constexpr (DB) dw_write_db<RAG>(db, dbs, mb, cb, mo, miF, tid);
}

// ---------------------------------------------------------------------------
// B2 at O=1: G and U are plain [row][E] (the padded layout with OP=1), there
// is no o to contract, and a dR entry is one product. The tile, the staging
// pipeline and the MFMA step are those of the kernel above; dR^T is built
// from LDS images of the g and u rows, as e-pairs: pass j of a thread is
// row (m = j, c = tid >> 4), the same (uc, e-pair) ownership, so db sums alike.
// ---------------------------------------------------------------------------
template <bool DB, bool RAG>
__global__ void __launch_bounds__(NT)
pairconv_bwd_dw_o1_kernel(const __bf16* __restrict__ Gt,  // (mo, E)
                          const __bf16* __restrict__ Ut,  // (miF, E)
                          const __bf16* __restrict__ Ht,  // (128, E)
                          float* __restrict__ dW,         // (mo*miF, 128) f32
                          float* __restrict__ db,         // (mo*miF,) f32, DB only
                          int E, int mo, int miF) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* dr_lds = reinterpret_cast<__bf16*>(smem);                  // [128n][32e] 8 KiB
    __bf16* h_lds = reinterpret_cast<__bf16*>(smem + 8192);            // [128k][32e] 8 KiB
    __bf16* u_lds = reinterpret_cast<__bf16*>(smem + 16384);           // [32][32]
    __bf16* g_lds = reinterpret_cast<__bf16*>(smem + 16384 + 32 * 32 * 2); // [4][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l15 = lane & 15;
    const int l4 = lane >> 4;
    const int wn = wid >> 1;          // 0..3: n-group of 32
    const int wk = wid & 1;           // 0..1: k-group of 64
    const int ncb = RAG ? (miF + 31) / 32 : miF / 32;
    const int mb = blockIdx.x / ncb;            // mo-block (4 mo each)
    const int cb = blockIdx.x % ncb;            // urow chunk

    f32x4 acc[2][4];                  // wave: 32 n x 64 k
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    // one 8-edge unit of a row: threads 0..127 own the u chunk, 0..15 the g tile
    auto load_row8 = [&](const __bf16* __restrict__ T, int row0, int e0) {
        bf16x8 v(0);
        int ro = tid >> 2, eu = (tid & 3) * 8;
        const __bf16* src = T + (size_t)(row0 + ro) * E + e0 + eu;
        if (e0 + eu + 8 <= E) v = *reinterpret_cast<const bf16x8*>(src);
        else { for (int j = 0; j < 8; ++j) v[j] = (e0 + eu + j < E) ? src[j] : (__bf16)0.f; }
        return v;
    };
    bf16x8 u_reg(0), g_reg(0), h_reg;
    const int nec = (E + 31) / 32;
    auto load_chunk = [&](int ec) {
        const int e0 = ec * 32;
        if (tid < 128) u_reg = load_row8(Ut, cb * 32, e0);
        if (tid < 16) g_reg = load_row8(Gt, mb * 4, e0);
        h_reg = dw_load_h(Ht, E, e0, tid);
    };

    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    load_chunk(0);
    for (int ec = 0; ec < nec; ++ec) {
        __syncthreads();   // previous MFMA done reading the LDS images
        if (tid < 128) *reinterpret_cast<bf16x8*>(u_lds + (size_t)tid * 8) = u_reg;
        if (tid < 16) *reinterpret_cast<bf16x8*>(g_lds + (size_t)tid * 8) = g_reg;
        {
            int k = tid >> 2, eu = (tid & 3) * 8;
            *reinterpret_cast<bf16x8*>(h_lds + (size_t)k * 32 + eu) = h_reg;
        }
        if (ec + 1 < nec) load_chunk(ec + 1);   // issue next loads early
        __syncthreads();
        // cooperative dR^T tile [128n][32e] (e-pairs, packed)
        static_assert((128 * 32) / 2 == 4 * NT, "db: pass j is mo j");
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int i = tid + j * NT;
            int e = (i & 15) * 2, n = i >> 4;
            int m = n >> 5, c = n & 31;
            f32x2 gv = b2f2(*reinterpret_cast<const bf16x2*>(g_lds + m * 32 + e));
            f32x2 uv = b2f2(*reinterpret_cast<const bf16x2*>(u_lds + c * 32 + e));
            const float d0 = fmaf(gv[0], uv[0], 0.f), d1 = fmaf(gv[1], uv[1], 0.f);
            if constexpr (DB) dbs[j] += d0 + d1;
            *reinterpret_cast<bf16x2*>(dr_lds + (size_t)n * 32 + e) =
                bf16x2{(__bf16)d0, (__bf16)d1};
        }
        __syncthreads();
        dw_mfma_chunk(acc, dr_lds, h_lds, wn, wk, l15, l4);
    }
    __syncthreads();
    dw_write_tile<RAG>(dW, acc, mb, cb, mo, miF, wn, wk, l15, l4);
    if constexpr (DB) dw_write_db<RAG>(db, dbs, mb, cb, mo, miF, tid);
}

// ---------------------------------------------------------------------------
// B3: du[c,e,o] = sum_mo R[e,(mo,c)] g[mo,e,o],  R = H @ W^T + bias
// G is read as (mo, E, OP) vectors and dU written as (miF, E, OP) vectors,
// f32 or bf16 (TD; the bf16 form rounds the f32 sums once, to nearest even).
// block: 64 e x 32 urow, loops mo in blocks of 8; the R tile is recomputed by
// the forward's MFMA loop (mfma_rtile), bounced through LDS, contracted vs g.
//
// A thread owns the cells (e = lane, c = 4 wid + k), k < 4, for the whole
// kernel and keeps their 4 x O sums in registers: LDS holds only h | R | g |
// bias, 68,608 B at OP = 8, so two workgroups are resident on a CU at every
// O and one block's W-fragment loads and MFMA phase overlap the other's
// bounce and contraction. With the f32 sums in LDS (41 KB at O = 5, 57 KB at
// O = 7) the launch asked for 96-115 KB and ran one workgroup per CU at
// O >= 5, every phase serialised by the barriers; that, not the layout, was
// the 4-10 % that du lost against the e-contiguous kernel
// (profiles/du_residency.md).
//
// The R bounce is [e][q][m][k] (n = (m, c = 4 q + k)), rows DU_RP apart: the
// four registers of an MFMA fragment are the four k of one (e, q, m), one
// 8-byte store, and the 32 values a thread contracts are 64 contiguous
// bytes of its row, four 16-byte reads. DU_RP = 264 elements = 132 dwords
// keeps those reads conflict-free (16 lanes x 4 banks tile the 64 banks).
// The g tile sits [m][e][OP] as in memory: per m a thread reads one vector,
// widens it once and uses it for its four cells. g and bias are double
// buffered, so a mo-block needs two barriers, not three.
// No W prefetch here: the contraction phase holds more live state than the
// forward's epilogue, and prefetching under the 2-blocks/CU cap spilled
// 116-240 B/lane (profiles/LADDER.md).
// ---------------------------------------------------------------------------
#define DU_RP 264   // R bounce row pitch, elements

// mfma_rtile for du, same MFMA order and so the same R bits, with the W
// fragments in a ring of two k-steps: step kit+2 loads when step kit's MFMAs
// are issued, and nothing crosses a step. Left to itself the compiler fills
// what the du sums leave of the 128 registers with W loads hoisted as far as
// they go and then spills at O = 7; this holds 32.
__device__ __forceinline__ void du_rtile(f32x4 (&acc)[4][2], const __bf16* h_lds,
                                         const __bf16* pbase, int we, int l15, int l4) {
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int ef = 0; ef < 2; ++ef) acc[mf][ef] = f32x4(0.f);
    bf16x8 a[2][4];
#pragma unroll
    for (int kit = 0; kit < 2; ++kit)
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) a[kit][mf] = load_wfrag(pbase, mf * 4 + kit);
#pragma unroll
    for (int kit = 0; kit < 4; ++kit) {
        const int k0 = kit * 32 + l4 * 8;
        bf16x8 b[2];
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
                acc[mf][ef] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[kit & 1][mf], b[ef], acc[mf][ef], 0, 0, 0);
        if (kit + 2 < 4) {
#pragma unroll
            for (int mf = 0; mf < 4; ++mf)
                a[kit & 1][mf] = load_wfrag(pbase, mf * 4 + kit + 2);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int O, typename TD>
__device__ __forceinline__ void du_store_cell(TD* __restrict__ dst, const float (&s)[O]) {
    constexpr int OP = opad_of(O);
    if constexpr (O == 1) {
        dst[0] = (TD)s[0];
    } else if constexpr (sizeof(TD) == 4) {
#pragma unroll
        for (int q = 0; q < OP / 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (q * 4 + j < O) ? s[q * 4 + j] : 0.f;
            *reinterpret_cast<f32x4*>(dst + q * 4) = v;
        }
    } else {
        typename OVec<OP>::type v;
#pragma unroll
        for (int j = 0; j < OP; ++j) v[j] = (j < O) ? (__bf16)s[j] : (__bf16)0.f;
        *reinterpret_cast<typename OVec<OP>::type*>(dst) = v;
    }
}

template <int O, typename TD>
__global__ void __launch_bounds__(NT, 4)   // cap VGPR<=128: 2 blocks/CU
pairconv_bwd_du_kernel(const __bf16* __restrict__ H,   // (E,128)
                       const __bf16* __restrict__ P,   // packed W as forward
                       const float* __restrict__ bias, // (mo*miF,)
                       const __bf16* __restrict__ Gt,  // (mo, E, OP)
                       TD* __restrict__ dU,            // (miF, E, OP), pads written 0
                       int E, int mo, int miF, int nmemb, int coh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int OP = opad_of(O);
    typedef typename OVec<OP>::type ovec;
    constexpr int GT = 8 * 64 * OP;                                    // g tile, elements
    __bf16* h_lds = reinterpret_cast<__bf16*>(smem);                   // [64][128] swizzled 16K
    constexpr int RB = 64 * DU_RP * 2;                                 // R bounce, bytes
    __bf16* r_lds = reinterpret_cast<__bf16*>(smem + 16384);           // [64e][DU_RP] 33K
    __bf16* g_lds = reinterpret_cast<__bf16*>(smem + 16384 + RB);      // [2][8][64][OP]
    float* bias_lds = reinterpret_cast<float*>(smem + 16384 + RB + 2 * GT * 2);  // [2][256]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // the wave index as a scalar: the W-fragment addresses are then a scalar
    // base plus one lane offset, not 64-bit vector pointers that the
    // accumulators would push into scratch
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15;
    const int l4 = lane >> 4;
    const int wm = wid >> 1;
    const int we = wid & 1;
    int eb, cb;                       // the cohort shares a urow chunk
    cohort_map(coh, nmemb, eb, cb);
    const int e0 = eb * 64;
    const int uc0 = cb * 32;          // urow chunk

    stage_h_tile(h_lds, H, e0, E, tid);

    float du[4][O];                   // cells (e = lane, c = 4 wid + k)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 0; o < O; ++o) du[k][o] = 0.f;

    // T14 register staging: the next mo-block's g tile + bias chunk load
    // while the current block's MFMA + contraction run (the g tile is one
    // (m, e) vector per thread; at O=1, 8 edges of one m for 64 threads).
    // The g load is a bare predicated load into a register zeroed once (a
    // thread's edge is in or out of range for the whole kernel).
    ovec g_reg(0);
    float bias_reg;
    const bool g_in = e0 + lane < E;
    auto load_gb = [&](int mb) {
        if constexpr (O == 1) {
            if (tid < 64) {   // spelled out on purpose: see dw_load_h
                int ro = tid >> 3, eu = (tid & 7) * 8;
                const __bf16* src = Gt + (size_t)(mb * 8 + ro) * E + e0 + eu;
                if (e0 + eu + 8 <= E) g_reg = *reinterpret_cast<const bf16x8*>(src);
                else {
                    bf16x8 v(0);
                    for (int j = 0; j < 8; ++j) if (e0 + eu + j < E) v[j] = src[j];
                    g_reg = v;
                }
            }
        } else {
            if (g_in)
                g_reg = *reinterpret_cast<const ovec*>(
                    Gt + ((size_t)(mb * 8 + (tid >> 6)) * E + e0 + lane) * OP);
        }
        if (tid < 256) {
            int m = tid >> 5, c = tid & 31;
            bias_reg = bias[(size_t)(mb * 8 + m) * miF + uc0 + c];
        }
    };
    load_gb(0);

    const int nmo = mo / 8;

    for (int mb = 0; mb < nmo; ++mb) {
        // commit the staged g tile [8][64][OP] + bias chunk [256] to the
        // buffer of this parity. Its last readers were block mb-2's, which
        // every thread left before it passed a barrier of block mb-1.
        __bf16* g_buf = g_lds + (mb & 1) * GT;
        float* b_buf = bias_lds + (mb & 1) * 256;
        if constexpr (O == 1) {
            if (tid < 64) *reinterpret_cast<bf16x8*>(g_buf + (size_t)tid * 8) = g_reg;
        } else {
            *reinterpret_cast<ovec*>(g_buf + (size_t)tid * OP) = g_reg;
        }
        if (tid < 256) b_buf[tid] = bias_reg;
        if (mb + 1 < nmo) load_gb(mb + 1);   // issue next block's loads early
        __syncthreads();   // g, bias (and h) visible; block mb-1's r_lds reads done
        // MFMA R tile (256n x 64e), A-fragments straight from the packed W
        f32x4 acc[4][2];
        const __bf16* pbase = P + ((((size_t)mb * (miF / 32) + cb) * 4 + wm) * 4) * 4 * 64 * 8
                              + (size_t)lane * 8;
        du_rtile(acc, h_lds, pbase, we, l15, l4);
        // bounce R (+bias) to LDS: fragment (mf, ef) holds rows
        // r = wm*64 + mf*16 + l4*4 + reg, that is m = 2 wm + (mf >> 1),
        // q = 4 (mf & 1) + l4, k = reg, of column e = we*32 + ef*16 + l15
        {
            __bf16* rb = r_lds + (size_t)(we * 32 + l15) * DU_RP + l4 * 32 + wm * 8;
            const float* bb = b_buf + wm * 64 + l4 * 4;
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(bb + mf * 16);
#pragma unroll
                for (int ef = 0; ef < 2; ++ef) {
                    bf16x4 v;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg)
                        v[reg] = (__bf16)(acc[mf][ef][reg] + b4[reg]);
                    *reinterpret_cast<bf16x4*>(
                        rb + ef * 16 * DU_RP + (mf & 1) * 128 + (mf >> 1) * 4) = v;
                }
            }
        }
        __syncthreads();
        // contraction: du[k][o] += sum_m R[(m, c_k)][e] * g[m][e][o], m
        // ascending, one fma per term (the order the sums always had)
        const __bf16* gp = g_buf + (size_t)lane * OP;
        bf16x8 rv[4];                 // R[e][q = wid][m][k]
#pragma unroll
        for (int j = 0; j < 4; ++j)
            rv[j] = *reinterpret_cast<const bf16x8*>(
                r_lds + (size_t)lane * DU_RP + wid * 32 + j * 8);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            float gf[O];
            if constexpr (O == 1) {
                gf[0] = b2f(gp[m * 64]);
            } else {
                ovec gv = *reinterpret_cast<const ovec*>(gp + (size_t)m * 64 * OP);
#pragma unroll
                for (int o = 0; o < O; ++o) gf[o] = b2f(gv[o]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float r = b2f(rv[m >> 1][(m & 1) * 4 + k]);
#pragma unroll
                for (int o = 0; o < O; ++o) du[k][o] = fmaf(r, gf[o], du[k][o]);
            }
        }
    }
    // each cell's (c, e) vector of OP values straight from registers, pads
    // zero; rows e >= E are not written. In bf16 a wave's store covers 64
    // consecutive vectors.
    if (g_in) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            du_store_cell<O, TD>(
                dU + ((size_t)(uc0 + wid * 4 + k) * E + e0 + lane) * OP, du[k]);
    }
}

// ---------------------------------------------------------------------------
// launchers. G is (mo, E, OP), U (miF, E, OP), dU (miF, E, OP), OP = opad_of(O)
// ---------------------------------------------------------------------------
static void check_opad(const torch::Tensor& T, const char* name, int64_t rows,
                       int E, int O, c10::ScalarType dt) {
    TORCH_CHECK(O == 1 || O == 3 || O == 5 || O == 7, "unsupported O ", O);
    TORCH_CHECK(T.is_cuda() && T.is_contiguous() && T.dtype() == dt && T.dim() == 3 &&
                T.size(0) == rows && T.size(1) == E && T.size(2) == opad_of(O),
                name, " must be (rows, E, OP(O)) contiguous");
}

void pairconv_bwd_dh(torch::Tensor Gt, torch::Tensor Ut, torch::Tensor Wt,
                     torch::Tensor dH, int64_t mo_, int64_t O_) {
    int E = dH.size(0), mo = (int)mo_, miF = Ut.size(0), O = (int)O_;
    check_opad(Gt, "G", mo, E, O, torch::kBFloat16);
    check_opad(Ut, "U", miF, E, O, torch::kBFloat16);
    TORCH_CHECK(Wt.is_contiguous() && dH.is_contiguous() && dH.dtype() == torch::kFloat32);
    TORCH_CHECK(Wt.numel() == (int64_t)mo * miF * KDIM, "expect packed W (P1)");
    TORCH_CHECK(mo % 8 == 0 && miF % 32 == 0 && dH.size(1) == KDIM);
    auto stream = at::cuda::getCurrentHIPStream();
    int eblk = (E + 63) / 64;
    int nmo = mo / 8;
    int nsplit = (nmo % 16 == 0) ? 16 : ((nmo % 8 == 0) ? 8 : 1);
    while (eblk * nsplit * 2 <= 1024 && nsplit * 2 <= nmo && nmo % (nsplit * 2) == 0)
        nsplit *= 2;
    const int PS = 4, PE = 128;
    int panels = ((eblk + PE - 1) / PE) * ((nsplit + PS - 1) / PS);
    dim3 grid((long)panels * PS * PE);
    DISPATCH_ORDER(O, kO, "O", {
        constexpr int LP = (kO == 1) ? 8 : opad_of(kO);
        // dr | g[8][64][LP], and at O=1 | u[32][64][LP]
        size_t lds = 32768 + (size_t)(kO == 1 ? 8 + 32 : 8) * 64 * LP * 2;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(pairconv_bwd_dh_kernel<kO>), grid, dim3(NT), lds, stream,
                           tptr<const __bf16>(Gt), tptr<const __bf16>(Ut),
                           tptr<const __bf16>(Wt),
                           dH.data_ptr<float>(), E, mo, miF, nsplit, eblk);
    });
    check_launch("bwd_dh: ");
}

template <int O, bool DB, bool RAG>
static void launch_dw(dim3 grid, hipStream_t stream, const __bf16* Gt,
                      const __bf16* Ut, const __bf16* Ht, float* dW, float* db,
                      int E, int mo, int miF) {
    if constexpr (O == 1) {
        size_t lds = 16384 + (size_t)32 * 32 * 2 + (size_t)4 * 32 * 2;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(pairconv_bwd_dw_o1_kernel<DB, RAG>), grid,
                           dim3(NT), lds, stream, Gt, Ut, Ht, dW, db, E, mo, miF);
    } else {
        size_t lds = 16384 + (size_t)4 * 32 * opad_of(O) * 2;   // dr | h | g[4][32][OP]
        hipLaunchKernelGGL(HIP_KERNEL_NAME(pairconv_bwd_dw_kernel<O, DB, RAG>), grid,
                           dim3(NT), lds, stream, Gt, Ut, Ht, dW, db, E, mo, miF);
    }
}

// db (mo*miF,) f32 is filled too; an empty db means "not wanted". G has mo_
// rows and U miF_p rows (multiples of 4 and 32). A 2-D dW (mo_*miF_p, 128) has
// those sizes; a 3-D dW (mo, miF, 128) names the true ones, mo <= mo_ and
// miF <= miF_p with miF_p = ceil32(miF), and db is then (mo*miF,).
void pairconv_bwd_dw(torch::Tensor Gt, torch::Tensor Ut, torch::Tensor Ht,
                     torch::Tensor dW, torch::Tensor db, int64_t mo_, int64_t O_) {
    int E = Ht.size(1), mo_p = (int)mo_, miF_p = Ut.size(0), O = (int)O_;
    check_opad(Gt, "G", mo_p, E, O, torch::kBFloat16);
    check_opad(Ut, "U", miF_p, E, O, torch::kBFloat16);
    TORCH_CHECK(Ht.is_contiguous() && Ht.dtype() == torch::kBFloat16 && Ht.size(0) == KDIM);
    TORCH_CHECK(mo_p >= 4 && mo_p % 4 == 0 && miF_p >= 32 && miF_p % 32 == 0);
    int mo = mo_p, miF = miF_p;
    if (dW.dim() == 3) {
        mo = dW.size(0);
        miF = dW.size(1);
        TORCH_CHECK(mo >= 1 && mo <= mo_p && miF >= 1 && ceil_mif(miF) == miF_p &&
                    dW.size(2) == KDIM, "expect dW as (mo, miF, 128) inside (mo_, ceil32(miF))");
    }
    TORCH_CHECK(dW.is_cuda() && dW.is_contiguous() && dW.dtype() == torch::kFloat32 &&
                dW.numel() == (int64_t)mo * miF * KDIM);
    auto stream = at::cuda::getCurrentHIPStream();
    const bool want_db = db.numel() > 0;
    if (want_db)
        TORCH_CHECK(db.is_cuda() && db.is_contiguous() && db.dtype() == torch::kFloat32 &&
                    db.numel() == (int64_t)mo * miF, "db must be (mo*miF,) f32 or empty");
    const bool rag = mo % 4 != 0 || miF % 32 != 0;
    dim3 grid(((mo + 3) / 4) * (miF_p / 32));   // mo-blocks that hold a true row
    float* dbp = want_db ? db.data_ptr<float>() : nullptr;
#define DW_LAUNCH(DB, RAG)                                                          \
    launch_dw<kO, DB, RAG>(grid, stream, tptr<const __bf16>(Gt), tptr<const __bf16>(Ut), \
                           tptr<const __bf16>(Ht), dW.data_ptr<float>(), dbp, E, mo, miF)
    DISPATCH_ORDER(O, kO, "O", {
        if (want_db) { if (rag) DW_LAUNCH(true, true); else DW_LAUNCH(true, false); }
        else { if (rag) DW_LAUNCH(false, true); else DW_LAUNCH(false, false); }
    });
#undef DW_LAUNCH
    check_launch("bwd_dw: ");
}

void pairconv_bwd_du(torch::Tensor H, torch::Tensor W, torch::Tensor bias,
                     torch::Tensor Gt, torch::Tensor dU, int64_t mo_, int64_t O_) {
    int E = H.size(0), mo = (int)mo_, miF = dU.size(0), O = (int)O_;
    check_opad(Gt, "G", mo, E, O, torch::kBFloat16);
    check_opad(dU, "dU", miF, E, O, dU.scalar_type());
    TORCH_CHECK(H.is_contiguous() && W.is_contiguous() && bias.is_contiguous());
    TORCH_CHECK(H.dtype() == torch::kBFloat16 && H.size(1) == KDIM);
    TORCH_CHECK(W.numel() == (int64_t)mo * miF * KDIM, "expect packed W (P)");
    TORCH_CHECK(bias.dtype() == torch::kFloat32 && bias.numel() == (int64_t)mo * miF);
    TORCH_CHECK(mo % 8 == 0 && miF % 32 == 0);
    auto stream = at::cuda::getCurrentHIPStream();
    int nmemb = (E + 63) / 64;
    int ncb = miF / 32;
    int coh = (ncb % 8 == 0) ? 1 : 0;
    dim3 grid(nmemb * ncb);
    DISPATCH_F32_BF16(dU, __bf16, DISPATCH_ORDER(O, kO, "O", {
        // h | R | g [2][8][64][OP] | bias [2][256]: 68,608 B at OP = 8
        size_t lds = 16384 + (size_t)64 * DU_RP * 2 +
                     (size_t)2 * 8 * 64 * opad_of(kO) * 2 + 2 * 256 * 4;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(pairconv_bwd_du_kernel<kO, T>),
                           grid, dim3(NT), lds, stream,
                           tptr<const __bf16>(H), tptr<const __bf16>(W),
                           bias.data_ptr<float>(), tptr<const __bf16>(Gt),
                           tptr<T>(dU), E, mo, miF, nmemb, coh);
    }));
    check_launch("bwd_du: ");
}
