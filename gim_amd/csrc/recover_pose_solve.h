// cv::recoverPose's arithmetic for csrc/recover_pose.hip, as functions that compile for the host and for the device: the kernel runs
// gim_rp_decompose on one lane per pair and gim_rp_point on every (point, candidate), tools/rp_host_check.cpp runs gim_rp_recover on
// the CPU (the arithmetic can be read against pose.recover_pose_ge without a GPU).  fp64, plain C++, real arithmetic only, every loop
// bounded; the contract is next to gim_recover_pose in include/gim_hip.h.
//
// Nothing here is indexed at run time: the 3 x 3 and 4 x 4 matrices are arrays whose every index is a template argument or the
// counter of a fully unrolled loop, so on the device they live in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GIM_RP_FN __host__ __device__ inline
#else
#define GIM_RP_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GIM_RP_UNROLL _Pragma("unroll")
#else
#define GIM_RP_UNROLL
#endif

constexpr int GIM_RP_SWEEPS3 = 8;        // cyclic Jacobi sweeps over E^T E (three rotations each)
constexpr int GIM_RP_SWEEPS4 = 8;        // cyclic Jacobi sweeps over A^T A of a point (six rotations each)
constexpr double GIM_RP_W_TINY = 1e-300; // recover_pose's clamp of the homogeneous coordinate
constexpr int GIM_RP_CAND = 12;          // doubles per candidate: R row-major, then t

// One Jacobi rotation in the plane (P, Q), P < Q, of the symmetric N x N matrix a (only its upper triangle is read and written),
// accumulated into v (columns: the eigenvectors so far).  Rutishauser's formulas: t the smaller root, tau = s / (1 + c).
template <int N, int P, int Q>
GIM_RP_FN void gim_rp_rotate(double (&a)[N][N], double (&v)[N][N]) {
    const double apq = a[P][Q];
    if (!(apq != 0.0)) return;           // nothing to annihilate (a NaN goes on as it is)
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // theta^2 = inf: t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = 0.0;
    GIM_RP_UNROLL
    for (int r = 0; r < N; ++r) {
        if (r == P || r == Q) continue;
        double& arp = r < P ? a[r][P] : a[P][r];
        double& arq = r < Q ? a[r][Q] : a[Q][r];
        const double g = arp, h = arq;
        arp = g - s * (h + tau * g);
        arq = h + s * (g - tau * h);
    }
    GIM_RP_UNROLL
    for (int r = 0; r < N; ++r) {
        const double g = v[r][P], h = v[r][Q];
        v[r][P] = g - s * (h + tau * g);
        v[r][Q] = h + s * (g - tau * h);
    }
}

GIM_RP_FN void gim_rp_jacobi3(double (&a)[3][3], double (&v)[3][3]) {
    for (int sweep = 0; sweep < GIM_RP_SWEEPS3; ++sweep) {
        gim_rp_rotate<3, 0, 1>(a, v);
        gim_rp_rotate<3, 0, 2>(a, v);
        gim_rp_rotate<3, 1, 2>(a, v);
    }
}

GIM_RP_FN void gim_rp_jacobi4(double (&a)[4][4], double (&v)[4][4]) {
    for (int sweep = 0; sweep < GIM_RP_SWEEPS4; ++sweep) {
        gim_rp_rotate<4, 0, 1>(a, v);
        gim_rp_rotate<4, 0, 2>(a, v);
        gim_rp_rotate<4, 0, 3>(a, v);
        gim_rp_rotate<4, 1, 2>(a, v);
        gim_rp_rotate<4, 1, 3>(a, v);
        gim_rp_rotate<4, 2, 3>(a, v);
    }
}

// exchanges the eigenpairs I and J when the later one is the larger: three of these sort a 3 x 3 spectrum, largest first
template <int I, int J>
GIM_RP_FN void gim_rp_order(double (&d)[3], double (&v)[3][3]) {
    if (d[J] > d[I]) {
        const double x = d[I];
        d[I] = d[J], d[J] = x;
        GIM_RP_UNROLL
        for (int r = 0; r < 3; ++r) {
            const double y = v[r][I];
            v[r][I] = v[r][J], v[r][J] = y;
        }
    }
}

// cv::decomposeEssentialMat with a fixed-sweep SVD: cand [4][GIM_RP_CAND] = (R1, t), (R2, t), (R1, -t), (R2, -t), the order of
// pose.recover_pose.  E is scaled by its largest |entry|; V: the eigenvectors of E^T E by cyclic Jacobi, largest eigenvalue first, v0
// normalised, v1 orthogonalised against v0, v2 = v0 x v1 (det V = +1); U: u0 = E v0 / |E v0|, u1 = E v1 orthogonalised against u0
// and normalised (a perpendicular of u0 when E v1 vanishes: a rank-one E), u2 = u0 x u1 (det U = +1); R1 = U W V^T, R2 = U W^T V^T,
// t = u2.  false (and cand zero): an entry of E that is not finite, or E = 0.
GIM_RP_FN bool gim_rp_decompose(const double* E, double* cand) {
    double e[3][3], big = 0.0;
    bool finite = true;
    GIM_RP_UNROLL
    for (int i = 0; i < 9; ++i) {
        const double x = E[i];
        finite = finite && fabs(x) <= 1.7976931348623157e308;
        big = fabs(x) > big ? fabs(x) : big;
    }
    if (!finite || !(big > 0.0)) {
        GIM_RP_UNROLL
        for (int i = 0; i < 4 * GIM_RP_CAND; ++i) cand[i] = 0.0;
        return false;
    }
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) {
        GIM_RP_UNROLL
        for (int j = 0; j < 3; ++j) e[i][j] = E[3 * i + j] / big;
    }
    double a[3][3], v[3][3];
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) {
        GIM_RP_UNROLL
        for (int j = 0; j < 3; ++j) {
            a[i][j] = (e[0][i] * e[0][j] + e[1][i] * e[1][j]) + e[2][i] * e[2][j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    gim_rp_jacobi3(a, v);
    double d[3] = {a[0][0], a[1][1], a[2][2]};
    gim_rp_order<0, 1>(d, v);
    gim_rp_order<0, 2>(d, v);
    gim_rp_order<1, 2>(d, v);
    double v0[3] = {v[0][0], v[1][0], v[2][0]}, v1[3] = {v[0][1], v[1][1], v[2][1]}, v2[3];
    double n = sqrt((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2]);
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) v0[i] /= n;
    double dot = (v0[0] * v1[0] + v0[1] * v1[1]) + v0[2] * v1[2];
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) v1[i] -= dot * v0[i];
    n = sqrt((v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2]);
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) v1[i] /= n;
    v2[0] = v0[1] * v1[2] - v0[2] * v1[1], v2[1] = v0[2] * v1[0] - v0[0] * v1[2], v2[2] = v0[0] * v1[1] - v0[1] * v1[0];
    double u0[3], u1[3], u2[3];
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) {
        u0[i] = (e[i][0] * v0[0] + e[i][1] * v0[1]) + e[i][2] * v0[2];
        u1[i] = (e[i][0] * v1[0] + e[i][1] * v1[1]) + e[i][2] * v1[2];
    }
    n = sqrt((u0[0] * u0[0] + u0[1] * u0[1]) + u0[2] * u0[2]);   // the largest singular value of e: at least 1 / 3
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) u0[i] /= n;
    dot = (u0[0] * u1[0] + u0[1] * u1[1]) + u0[2] * u1[2];
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) u1[i] -= dot * u0[i];
    n = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    if (!(n > 1e-150)) {                 // rank one: any unit vector perpendicular to u0 -- u0 x (the axis of its smallest |entry|)
        const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
        const bool kx = ax <= ay && ax <= az, ky = !kx && ay <= az;
        const double w0 = kx ? 1.0 : 0.0, w1 = ky ? 1.0 : 0.0, w2 = (!kx && !ky) ? 1.0 : 0.0;
        u1[0] = u0[1] * w2 - u0[2] * w1, u1[1] = u0[2] * w0 - u0[0] * w2, u1[2] = u0[0] * w1 - u0[1] * w0;
        n = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    }
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) u1[i] /= n;
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1], u2[1] = u0[2] * u1[0] - u0[0] * u1[2], u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    // U W = (-u1, u0, u2) and U W^T = (u1, -u0, u2) as columns; the rows of V^T are v0, v1, v2
    GIM_RP_UNROLL
    for (int i = 0; i < 3; ++i) {
        GIM_RP_UNROLL
        for (int j = 0; j < 3; ++j) {
            const double r1 = (u0[i] * v1[j] - u1[i] * v0[j]) + u2[i] * v2[j];
            const double r2 = (u1[i] * v0[j] - u0[i] * v1[j]) + u2[i] * v2[j];
            cand[3 * i + j] = r1, cand[2 * GIM_RP_CAND + 3 * i + j] = r1;
            cand[GIM_RP_CAND + 3 * i + j] = r2, cand[3 * GIM_RP_CAND + 3 * i + j] = r2;
        }
        cand[9 + i] = u2[i], cand[GIM_RP_CAND + 9 + i] = u2[i];
        cand[2 * GIM_RP_CAND + 9 + i] = -u2[i], cand[3 * GIM_RP_CAND + 9 + i] = -u2[i];
    }
    return true;
}

// One match under one candidate c = (R row-major, t): the DLT matrix of pose._triangulate with P0 = [I | 0], P1 = [R | t]; its null
// vector as the eigenvector of the smallest eigenvalue of A^T A (cyclic Jacobi, the first smallest diagonal entry); then
// recover_pose's test: w clamped away from zero, X = Q[:3] / w, z0 = X[2], z1 = (R X + t)[2]; good iff both lie in (0, dthr).
GIM_RP_FN bool gim_rp_point(const double* c, double x, double y, double u, double w1, double dthr) {
    double A[4][4] = {{-1.0, 0.0, x, 0.0},
                      {0.0, -1.0, y, 0.0},
                      {u * c[6] - c[0], u * c[7] - c[1], u * c[8] - c[2], u * c[11] - c[9]},
                      {w1 * c[6] - c[3], w1 * c[7] - c[4], w1 * c[8] - c[5], w1 * c[11] - c[10]}};
    double a[4][4], v[4][4];
    GIM_RP_UNROLL
    for (int i = 0; i < 4; ++i) {
        GIM_RP_UNROLL
        for (int j = 0; j < 4; ++j) {
            a[i][j] = j >= i ? ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j] : 0.0;
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    gim_rp_jacobi4(a, v);
    double dmin = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
    GIM_RP_UNROLL
    for (int k = 1; k < 4; ++k) {
        const bool less = a[k][k] < dmin;
        dmin = less ? a[k][k] : dmin;
        q0 = less ? v[0][k] : q0, q1 = less ? v[1][k] : q1, q2 = less ? v[2][k] : q2, q3 = less ? v[3][k] : q3;
    }
    const double w = fabs(q3) > GIM_RP_W_TINY ? q3 : GIM_RP_W_TINY;
    const double X = q0 / w, Y = q1 / w, Z = q2 / w;
    const double z1 = ((X * c[6] + Y * c[7]) + Z * c[8]) + c[11];
    return Z > 0.0 && Z < dthr && z1 > 0.0 && z1 < dthr;
}

// the winner of four counts: the first maximum in candidate order (pose.recover_pose)
GIM_RP_FN int gim_rp_best(int n0, int n1, int n2, int n3) {
    return (n0 >= n1 && n0 >= n2 && n0 >= n3) ? 0 : (n1 >= n2 && n1 >= n3) ? 1 : n2 >= n3 ? 2 : 3;
}

// The whole of gim_recover_pose for one pair, serially (the host check): x0, x1 [P][2], mask_in [P] or NULL -> R [9], t [3], n_good
// [4], mask_out [P]; returns best, -1 for an invalid E (then everything is zero).
GIM_RP_FN int gim_rp_recover(const double* E, const double* x0, const double* x1, int P, const uint8_t* mask_in, double dthr, double* R,
                             double* t, int32_t* n_good, uint8_t* mask_out) {
    double cand[4 * GIM_RP_CAND];
    const bool ok = gim_rp_decompose(E, cand);
    for (int j = 0; j < 4; ++j) n_good[j] = 0;
    if (!ok) {
        for (int i = 0; i < 9; ++i) R[i] = 0.0;
        for (int i = 0; i < 3; ++i) t[i] = 0.0;
        for (int p = 0; p < P; ++p) mask_out[p] = 0;
        return -1;
    }
    for (int p = 0; p < P; ++p) {
        int bits = 0;
        if (!mask_in || mask_in[p])
            for (int j = 0; j < 4; ++j)
                bits |= (gim_rp_point(cand + GIM_RP_CAND * j, x0[2 * p], x0[2 * p + 1], x1[2 * p], x1[2 * p + 1], dthr) ? 1 : 0) << j;
        mask_out[p] = (uint8_t)bits;
        for (int j = 0; j < 4; ++j) n_good[j] += (bits >> j) & 1;
    }
    const int best = gim_rp_best(n_good[0], n_good[1], n_good[2], n_good[3]);
    for (int i = 0; i < 9; ++i) R[i] = cand[GIM_RP_CAND * best + i];
    for (int i = 0; i < 3; ++i) t[i] = cand[GIM_RP_CAND * best + 9 + i];
    for (int p = 0; p < P; ++p) mask_out[p] = (uint8_t)((mask_out[p] >> best) & 1);
    return best;
}
