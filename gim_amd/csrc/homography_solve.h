// The four-point homography solver of csrc/homography.hip, as one function that compiles for the host and for the device: the kernel
// calls it from one lane, tools/homography_host_check.cpp calls it on the CPU (the arithmetic can be read against pose.homography_4pt
// without a GPU).  fp64, plain C++; the contract is next to gim_homography_step in include/gim_hip.h.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GIM_H4_FN __host__ __device__ inline
#else
#define GIM_H4_FN inline
#endif

constexpr double GIM_H4_PIVOT_EPS = 1e-12;   // smallest pivot of the normalised 8 x 8 system
constexpr double GIM_H4_AREA_EPS = 1e-9;     // smallest doubled triangle area, normalised coordinates

// the triples of HomographyEstimatorCallback::checkSubset (fundam.cpp)
constexpr int GIM_H4_TRI[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};

// zero mean, mean distance sqrt(2): q = (p - c) * s.  false when the four points coincide.
GIM_H4_FN bool gim_h4_normalise(const double* p /* [4][2] */, double* q /* [4][2] */, double* c /* [2] */, double* s) {
    c[0] = (((p[0] + p[2]) + p[4]) + p[6]) * 0.25;
    c[1] = (((p[1] + p[3]) + p[5]) + p[7]) * 0.25;
    double md = 0.0;
    for (int i = 0; i < 4; ++i) {
        q[2 * i] = p[2 * i] - c[0];
        q[2 * i + 1] = p[2 * i + 1] - c[1];
        md += sqrt(q[2 * i] * q[2 * i] + q[2 * i + 1] * q[2 * i + 1]);
    }
    md *= 0.25;
    if (!(md > 0.0) || !isfinite(md)) return false;
    *s = sqrt(2.0) / md;
    for (int i = 0; i < 8; ++i) q[i] *= *s;
    return true;
}

// doubled signed area of the triangle (i, j, k) of q [4][2]
GIM_H4_FN double gim_h4_area2(const double* q, int i, int j, int k) {
    return (q[2 * j] - q[2 * i]) * (q[2 * k + 1] - q[2 * i + 1]) - (q[2 * j + 1] - q[2 * i + 1]) * (q[2 * k] - q[2 * i]);
}

// src, dst [4][2] -> H [9] row-major with H[8] = 1, dst ~ H src.  A: 8 x 9 doubles of work memory (LDS on the device: it is indexed
// at run time).  Returns false, and leaves H undefined, for a sample the contract rejects.
GIM_H4_FN bool gim_h4_solve(const double* src, const double* dst, double* A /* [8][9] */, double* H) {
    double qs[8], qd[8], cs[2], cd[2], ss, sd;
    if (!gim_h4_normalise(src, qs, cs, &ss) || !gim_h4_normalise(dst, qd, cd, &sd)) return false;
    int negative = 0;
    for (int t = 0; t < 4; ++t) {
        const double as = gim_h4_area2(qs, GIM_H4_TRI[t][0], GIM_H4_TRI[t][1], GIM_H4_TRI[t][2]);
        const double ad = gim_h4_area2(qd, GIM_H4_TRI[t][0], GIM_H4_TRI[t][1], GIM_H4_TRI[t][2]);
        if (!(fabs(as) >= GIM_H4_AREA_EPS) || !(fabs(ad) >= GIM_H4_AREA_EPS)) return false;     // collinear (or NaN)
        negative += (as < 0.0) != (ad < 0.0);
    }
    if (negative != 0 && negative != 4) return false;                                           // checkSubset's orientation test
    for (int i = 0; i < 4; ++i) {
        const double x = qs[2 * i], y = qs[2 * i + 1], u = qd[2 * i], v = qd[2 * i + 1];
        double* r0 = A + (2 * i) * 9;
        double* r1 = r0 + 9;
        r0[0] = x, r0[1] = y, r0[2] = 1.0, r0[3] = 0.0, r0[4] = 0.0, r0[5] = 0.0, r0[6] = -u * x, r0[7] = -u * y, r0[8] = u;
        r1[0] = 0.0, r1[1] = 0.0, r1[2] = 0.0, r1[3] = x, r1[4] = y, r1[5] = 1.0, r1[6] = -v * x, r1[7] = -v * y, r1[8] = v;
    }
    // Gaussian elimination with partial pivoting (the first row of the largest magnitude wins a tie)
    for (int k = 0; k < 8; ++k) {
        int piv = k;
        double best = fabs(A[k * 9 + k]);
        for (int r = k + 1; r < 8; ++r) {
            const double a = fabs(A[r * 9 + k]);
            if (a > best) best = a, piv = r;
        }
        if (!(best >= GIM_H4_PIVOT_EPS)) return false;
        if (piv != k)
            for (int c = k; c < 9; ++c) {
                const double t = A[k * 9 + c];
                A[k * 9 + c] = A[piv * 9 + c];
                A[piv * 9 + c] = t;
            }
        const double d = A[k * 9 + k];
        for (int r = k + 1; r < 8; ++r) {
            const double f = A[r * 9 + k] / d;
            for (int c = k + 1; c < 9; ++c) A[r * 9 + c] -= f * A[k * 9 + c];
        }
    }
    double h[9];
    for (int k = 7; k >= 0; --k) {
        double acc = A[k * 9 + 8];
        for (int c = k + 1; c < 8; ++c) acc -= A[k * 9 + c] * A[c * 9 + 8];
        A[k * 9 + 8] = acc / A[k * 9 + k];
    }
    for (int k = 0; k < 8; ++k) h[k] = A[k * 9 + 8];
    h[8] = 1.0;
    // H = Td^-1 Hn Ts with Ts = [ss 0 -ss cs.x; 0 ss -ss cs.y; 0 0 1], Td^-1 = [1/sd 0 cd.x; 0 1/sd cd.y; 0 0 1]
    double g[9];
    for (int r = 0; r < 3; ++r) {
        g[3 * r] = h[3 * r] * ss;
        g[3 * r + 1] = h[3 * r + 1] * ss;
        g[3 * r + 2] = h[3 * r + 2] - ss * (h[3 * r] * cs[0] + h[3 * r + 1] * cs[1]);
    }
    const double isd = 1.0 / sd;
    for (int c = 0; c < 3; ++c) {
        H[c] = g[c] * isd + cd[0] * g[6 + c];
        H[3 + c] = g[3 + c] * isd + cd[1] * g[6 + c];
        H[6 + c] = g[6 + c];
    }
    const double w = H[8];
    bool ok = true;
    for (int i = 0; i < 9; ++i) {
        H[i] /= w;
        ok = ok && isfinite(H[i]);
    }
    H[8] = 1.0;
    return ok;
}
