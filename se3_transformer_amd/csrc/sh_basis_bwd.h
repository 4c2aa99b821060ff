// Per-edge backward of the fused spherical-harmonics + basis pass
// (sh_basis.hip). Plain C++ with no torch/HIP dependency so the same code
// compiles for the device kernel and for a host-side check.
//
//   dK (TOT)  --Q_J-->  dY ((L+1)^2)  --recurrence tangents-->
//   (g_ct, g_st, g_cp, g_sp)  --closed-form chain-->  d rel (3)
//
// Parity target: autograd of ops/sh.py::sh_packed_from_cartesian, which
// treats (ct, st) and (cp, sp) as independent inputs of the Legendre and
// Chebyshev recurrences. The chain back to (x, y, z) is applied in its
// cancellation-free closed form instead of op-by-op.
#pragma once

#include <math.h>

#ifdef __HIPCC__
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD inline
#endif

// dy: per-edge scratch of (L+1)^2 floats, element s at dy[s * stride]
// (an LDS column on the device, a plain array on the host).
// meta: npairs x (d_in, d_out, off_out, off_q) as in the forward.
SH_HD void sh_basis_bwd_edge(float rx, float ry, float rz,
                             const float* __restrict__ qcat,
                             const float* __restrict__ normtab,
                             const int* __restrict__ meta, int npairs,
                             const float* __restrict__ dk,
                             float* dy, int stride, int L,
                             float* gx_std, float* gy_std, float* gz_std) {
    const float eps2 = 1e-24f;
    // SH-frame permutation, as in the forward
    const float x = rz, y = rx, z = ry;
    const float rho2 = x * x + y * y;
    const float r2 = rho2 + z * z;
    *gx_std = 0.f; *gy_std = 0.f; *gz_std = 0.f;
    // Degenerate branches. r ~ 0: every angle is a constant. rho ~ 0 (on the
    // SH polar axis): cp/sp are constants and rho is clamped, so ct = -z/|z|
    // is locally constant and st = eps/|z| moves by O(eps) only — autograd
    // yields 0 up to that O(1e-12) residue, which fp32 absorbs.
    if (rho2 <= eps2 || r2 <= eps2) return;

    const int S = (L + 1) * (L + 1);
    for (int s = 0; s < S; ++s) dy[s * stride] = 0.f;

    // 1. dY[J^2 + mj] += dK[off + oi*F + f] * q[mj*OI + oi]
    for (int p = 0; p < npairs; ++p) {
        const int di = meta[4 * p], dout = meta[4 * p + 1];
        const int O = 2 * dout + 1, I = 2 * di + 1, OI = O * I;
        const int Jlo = di > dout ? di - dout : dout - di, Jhi = di + dout;
        const int F = Jhi - Jlo + 1;
        const float* q = qcat + meta[4 * p + 3];
        const float* g = dk + meta[4 * p + 2];
        for (int J = Jlo; J <= Jhi; ++J) {
            const int f = J - Jlo, nm = 2 * J + 1;
            float* dyj = dy + (J * J) * stride;
            for (int oi = 0; oi < OI; ++oi) {
                const float gv = g[oi * F + f];
                for (int mj = 0; mj < nm; ++mj)
                    dyj[mj * stride] += gv * q[mj * OI + oi];
            }
            q += nm * OI;
        }
    }

    const float rho = sqrtf(rho2), r = sqrtf(r2);
    const float ct = -z / r, st = rho / r, cp = x / rho, sp = y / rho;

    // 2+3. forward recurrences with tangents, folded against dY
    float g_ct = 0.f, g_st = 0.f, g_cp = 0.f, g_sp = 0.f;
    float pmm = 1.f, pmm_s = 0.f;                 // P_m^m and d/dst
    float cm = 1.f, sm = 0.f;                     // cos/sin(m phi)
    float cm_c = 0.f, cm_s = 0.f, sm_c = 0.f, sm_s = 0.f;  // d/dcp, d/dsp
    for (int m = 0; m <= L; ++m) {
        if (m > 0) {
            const float k = (float)(-(2 * m - 1));
            pmm_s = (pmm_s * st + pmm) * k;
            pmm = pmm * st * k;
            const float ncm = cm * cp - sm * sp;
            const float ncm_c = cm_c * cp + cm - sm_c * sp;
            const float ncm_s = cm_s * cp - sm_s * sp - sm;
            const float nsm = sm * cp + cm * sp;
            const float nsm_c = sm_c * cp + sm + cm_c * sp;
            const float nsm_s = sm_s * cp + cm_s * sp + cm;
            cm = ncm; cm_c = ncm_c; cm_s = ncm_s;
            sm = nsm; sm_c = nsm_c; sm_s = nsm_s;
        }
        float p1 = 0.f, p1_c = 0.f, p1_s = 0.f;   // P_{l-1}^m, d/dct, d/dst
        float p2 = 0.f, p2_c = 0.f, p2_s = 0.f;   // P_{l-2}^m
        for (int l = m; l <= L; ++l) {
            float p, p_c, p_s;
            if (l == m) {
                p = pmm; p_c = 0.f; p_s = pmm_s;
            } else if (l == m + 1) {
                const float a = (float)(2 * m + 1);
                p = a * ct * pmm; p_c = a * pmm; p_s = a * ct * pmm_s;
            } else {
                const float a = (float)(2 * l - 1), b = (float)(l + m - 1);
                const float inv = 1.f / (float)(l - m);
                p = (a * ct * p1 - b * p2) * inv;
                p_c = (a * (p1 + ct * p1_c) - b * p2_c) * inv;
                p_s = (a * ct * p1_s - b * p2_s) * inv;
            }
            p2 = p1; p2_c = p1_c; p2_s = p1_s;
            p1 = p; p1_c = p_c; p1_s = p_s;
            const float n = normtab[l * (l + 1) / 2 + m];
            if (m == 0) {
                const float a = n * dy[(l * l + l) * stride];
                g_ct += a * p_c;
                g_st += a * p_s;
            } else {
                const float ac = n * dy[(l * l + l + m) * stride];
                const float as = n * dy[(l * l + l - m) * stride];
                const float w = ac * cm + as * sm;
                g_ct += w * p_c;
                g_st += w * p_s;
                g_cp += p * (ac * cm_c + as * sm_c);
                g_sp += p * (ac * cm_s + as * sm_s);
            }
        }
    }

    // 4. closed-form chain:
    //   d ct = (z x, z y, -rho^2) / r^3     d st = (x z^2, y z^2, -rho^2 z) / (rho r^3)
    //   d cp = (y^2, -x y, 0) / rho^3       d sp = (-x y, x^2, 0) / rho^3
    const float ir3 = 1.f / (r2 * r), irho = 1.f / rho;
    const float irho3 = irho / rho2;
    const float a = (g_ct * z + g_st * z * z * irho) * ir3;
    const float t = (g_cp * y - g_sp * x) * irho3;
    const float gx = a * x + t * y;
    const float gy = a * y - t * x;
    const float gz = -(g_ct * rho2 + g_st * rho * z) * ir3;
    // back to standard order: x_sh = rel[2], y_sh = rel[0], z_sh = rel[1]
    *gx_std = gy; *gy_std = gz; *gz_std = gx;
}
