// The seven-point fundamental-matrix solver of csrc/fundamental.hip, as one function that compiles for the host and for the device: the
// kernel calls it from one lane, tools/f7_host_check.cpp calls it on the CPU (the arithmetic can be read against pose.seven_point_ge
// without a GPU).  fp64, plain C++; the contract is next to gim_fundamental_step in include/gim_hip.h.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GIM_F7_FN __host__ __device__ inline
#else
#define GIM_F7_FN inline
#endif

constexpr double GIM_F7_SCALE_EPS = 1e-12;   // smallest mean distance of a side's seven points from their centre
constexpr double GIM_F7_RANK_EPS = 1e-12;    // smallest seventh pivot, relative to the first
constexpr double GIM_F7_CUBIC_EPS = 1e-12;   // smallest max |c| of the cubic: below it every matrix of the pencil is singular
constexpr double GIM_F7_LEAD_EPS = 1e-14;    // smallest |c3| relative to max |c| (pose.seven_point's rule)

// zero mean, mean distance sqrt(2): q = (p - c) * s.  false when the seven points coincide (or are not finite).
GIM_F7_FN bool gim_f7_normalise(const double* p /* [7][2] */, double* q /* [7][2] */, double* c /* [2] */, double* s) {
    c[0] = ((((((p[0] + p[2]) + p[4]) + p[6]) + p[8]) + p[10]) + p[12]) / 7.0;
    c[1] = ((((((p[1] + p[3]) + p[5]) + p[7]) + p[9]) + p[11]) + p[13]) / 7.0;
    double md = 0.0;
    for (int i = 0; i < 7; ++i) {
        q[2 * i] = p[2 * i] - c[0];
        q[2 * i + 1] = p[2 * i + 1] - c[1];
        md += sqrt(q[2 * i] * q[2 * i] + q[2 * i + 1] * q[2 * i + 1]);
    }
    md /= 7.0;
    if (!(md >= GIM_F7_SCALE_EPS) || !isfinite(md)) return false;
    *s = sqrt(2.0) / md;
    for (int i = 0; i < 14; ++i) q[i] *= *s;
    return true;
}

GIM_F7_FN double gim_f7_det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// two Newton steps on the monic cubic a^3 + b2 a^2 + b1 a + b0
GIM_F7_FN double gim_f7_polish(double a, double b2, double b1, double b0) {
    for (int it = 0; it < 2; ++it) {
        const double f = ((a + b2) * a + b1) * a + b0;
        const double g = (3.0 * a + 2.0 * b2) * a + b1;
        const double d = f / g;
        if (isfinite(d)) a -= d;
    }
    return a;
}

// p0, p1 [7][2] -> up to three F [3][9] row-major with p1^T F p0 = 0, unit Frobenius norm, ordered by the root a ascending; ok[j] = false
// and a zero matrix for an unused or rejected slot.  A: 7 x 9 doubles of work memory (LDS on the device: it is indexed at run time).
GIM_F7_FN void gim_f7_solve(const double p0[14], const double p1[14], double* A /* [7][9] */, double F[27], bool ok[3]) {
    for (int i = 0; i < 27; ++i) F[i] = 0.0;
    ok[0] = ok[1] = ok[2] = false;
    double q0[14], q1[14], c0[2], c1[2], s0, s1;
    if (!gim_f7_normalise(p0, q0, c0, &s0) || !gim_f7_normalise(p1, q1, c1, &s1)) return;
    for (int i = 0; i < 7; ++i) {
        const double x = q0[2 * i], y = q0[2 * i + 1], u = q1[2 * i], v = q1[2 * i + 1];
        double* r = A + 9 * i;
        r[0] = u * x, r[1] = u * y, r[2] = u, r[3] = v * x, r[4] = v * y, r[5] = v, r[6] = x, r[7] = y, r[8] = 1.0;
    }
    // Gauss-Jordan with full pivoting: the largest |a| over the rows k.. and all columns (a column that already holds a pivot is
    // exactly zero in those rows); the lowest row, then the lowest column, wins a tie.  rowof: four bits per column, the row whose
    // pivot sits in it, 15 for a free column.
    uint64_t rowof = 0xFFFFFFFFFull;
    double first = 0.0;
    for (int k = 0; k < 7; ++k) {
        int pr = k, pc = 0;
        double best = 0.0;
        for (int r = k; r < 7; ++r)
            for (int c = 0; c < 9; ++c) {
                const double a = fabs(A[r * 9 + c]);
                if (a > best) best = a, pr = r, pc = c;
            }
        if (k == 0) first = best;
        if (!(best > 0.0) || !isfinite(best)) return;
        if (k == 6 && !(best >= GIM_F7_RANK_EPS * first)) return;                               // rank-deficient sample
        if (pr != k)
            for (int c = 0; c < 9; ++c) {
                const double t = A[k * 9 + c];
                A[k * 9 + c] = A[pr * 9 + c];
                A[pr * 9 + c] = t;
            }
        const double d = A[k * 9 + pc];
        for (int c = 0; c < 9; ++c) A[k * 9 + c] = A[k * 9 + c] / d;
        for (int r = 0; r < 7; ++r) {
            if (r == k) continue;
            const double f = A[r * 9 + pc];
            for (int c = 0; c < 9; ++c) A[r * 9 + c] -= f * A[k * 9 + c];
        }
        rowof = (rowof & ~(0xFull << (4 * pc))) | ((uint64_t)k << (4 * pc));
    }
    int f1 = -1, f2 = -1;                                                                       // the two free columns, ascending
    for (int c = 0; c < 9; ++c)
        if (((rowof >> (4 * c)) & 15) == 15) {
            if (f1 < 0) f1 = c;
            else f2 = c;
        }
    double F1[9], F2[9];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 9; ++c) {
        const int r = (int)((rowof >> (4 * c)) & 15);
        F1[c] = c == f1 ? 1.0 : (c == f2 ? 0.0 : -A[(r % 7) * 9 + f1]);
        F2[c] = c == f2 ? 1.0 : (c == f1 ? 0.0 : -A[(r % 7) * 9 + f2]);
    }
    // det(a F1 + (1 - a) F2) = c0 + c1 a + c2 a^2 + c3 a^3 through a = 0, 1, -1, 2
    double Mm[9], Mp[9];
    for (int i = 0; i < 9; ++i) Mm[i] = 2.0 * F2[i] - F1[i], Mp[i] = 2.0 * F1[i] - F2[i];
    const double d0 = gim_f7_det3(F2), d1 = gim_f7_det3(F1), dm = gim_f7_det3(Mm), d2 = gim_f7_det3(Mp);
    const double k0 = d0;
    const double k2 = (d1 + dm) * 0.5 - k0;
    const double sum13 = (d1 - dm) * 0.5;                                                       // c1 + c3
    const double sum143 = ((d2 - k0) - 4.0 * k2) * 0.5;                                         // c1 + 4 c3
    const double k3 = (sum143 - sum13) / 3.0;
    const double k1 = sum13 - k3;
    const double cmax = fmax(fmax(fabs(k0), fabs(k1)), fmax(fabs(k2), fabs(k3)));
    if (!(cmax >= GIM_F7_CUBIC_EPS)) return;                                                    // the cubic is rounding noise
    if (!(fabs(k3) > GIM_F7_LEAD_EPS * (cmax + 1e-300))) return;
    const double b2 = k2 / k3, b1 = k1 / k3, b0 = k0 / k3;
    // a = t - b2 / 3 with t^3 + p t + q = 0; D = (q/2)^2 + (p/3)^3 > 0: one real root (Cardano), else three (trigonometric form)
    const double sh = b2 / 3.0;
    const double p = b1 - b2 * sh;
    const double q = (2.0 * sh * sh - b1) * sh + b0;
    const double hq = 0.5 * q, tp = p / 3.0;
    const double D = hq * hq + tp * tp * tp;
    double a[3];
    int nr;
    if (D > 0.0) {
        const double sD = sqrt(D);
        const double u = hq >= 0.0 ? -cbrt(hq + sD) : cbrt(sD - hq);                            // no cancellation under the cube root
        const double v = u != 0.0 ? -tp / u : 0.0;
        a[0] = (u + v) - sh;
        a[1] = a[2] = 0.0;
        nr = 1;
    } else if (D <= 0.0) {
        const double m = sqrt(-tp);                                                             // tp <= 0 here
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        if (m > 0.0) {
            double w = -hq / (m * m * m);
            w = w > 1.0 ? 1.0 : (w < -1.0 ? -1.0 : w);
            const double th = acos(w) / 3.0;
            const double tw = 2.0943951023931954923;                                            // 2 pi / 3
            t0 = 2.0 * m * cos(th), t1 = 2.0 * m * cos(th - tw), t2 = 2.0 * m * cos(th - 2.0 * tw);
        }
        a[0] = t0 - sh, a[1] = t1 - sh, a[2] = t2 - sh;
        nr = 3;
    } else {
        return;                                                                                 // NaN
    }
    a[0] = gim_f7_polish(a[0], b2, b1, b0);
    if (nr == 3) {
        a[1] = gim_f7_polish(a[1], b2, b1, b0);
        a[2] = gim_f7_polish(a[2], b2, b1, b0);
        double t;
        if (a[1] < a[0]) t = a[0], a[0] = a[1], a[1] = t;
        if (a[2] < a[1]) t = a[1], a[1] = a[2], a[2] = t;
        if (a[1] < a[0]) t = a[0], a[0] = a[1], a[1] = t;
    }
    // F = T1^T (a F1 + (1 - a) F2) T0 with T = [s 0 -s c.x; 0 s -s c.y; 0 0 1], then unit Frobenius norm
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 3; ++j) {
        if (j >= nr) continue;
        double N[9], G[9], P[9];
        for (int i = 0; i < 9; ++i) N[i] = a[j] * F1[i] + (1.0 - a[j]) * F2[i];
        for (int r = 0; r < 3; ++r) {
            G[3 * r] = N[3 * r] * s0;
            G[3 * r + 1] = N[3 * r + 1] * s0;
            G[3 * r + 2] = N[3 * r + 2] - s0 * (N[3 * r] * c0[0] + N[3 * r + 1] * c0[1]);
        }
        double n2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            P[c] = s1 * G[c];
            P[3 + c] = s1 * G[3 + c];
            P[6 + c] = G[6 + c] - s1 * (c1[0] * G[c] + c1[1] * G[3 + c]);
        }
        for (int i = 0; i < 9; ++i) n2 += P[i] * P[i];
        const double nrm = sqrt(n2);
        if (!(nrm > 0.0) || !isfinite(nrm)) continue;
        for (int i = 0; i < 9; ++i) F[9 * j + i] = P[i] / nrm;
        ok[j] = true;
    }
}
