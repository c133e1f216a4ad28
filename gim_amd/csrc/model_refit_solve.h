// The least-squares refit of a homography or a fundamental matrix on its inliers, for csrc/model_refit.hip, as functions that compile
// for the host and for the device: the kernel runs the per-point functions on every lane and gim_mr_solve on one lane per pair,
// tools/refit_host_check.cpp runs gim_mr_refit on the CPU (the arithmetic can be read against pose.refit_ge without a GPU).  fp64,
// plain C++, real arithmetic only, every loop bounded; the contract is next to gim_model_refit in include/gim_hip.h.
//
// kind 0: b ~ H a, the normalised DLT of pose.homography_dlt (two rows per inlier).  kind 1: b^T F a = 0, the normalised eight-point
// algorithm (one row of pose._epipolar_rows per inlier, then rank 2).  Both as OpenCV's HomographyEstimatorCallback::runKernel and
// run8Point do it: accumulate the 9 x 9 normal matrix A^T A and take the eigenvector of its smallest eigenvalue.
//
// GIM_MR_SWEEPS9 = 8 cyclic Jacobi sweeps (36 rotations each) over the 9 x 9 matrix.  Evidence, from the numpy restatement
// (pose._mr_solve with its sweep count varied) on the noisy scenes of tests/model_refit_cases.py, both kinds: the largest
// off-diagonal |entry| over the largest diagonal |entry| is at most 2.2e-24 after 6 sweeps, 3.1e-54 after 7 and 2.2e-141 after 8
// (the iteration converges quadratically; rounding is 1.1e-16), and the model has the same bits from sweep 6 on.  Eight leaves two
// sweeps of margin; tests/test_model_refit_cpu.py asserts the mass of every solve of every scene and round.
#pragma once
#include <math.h>
#include <stdint.h>

#include "two_view_residual.h"     // gim_tv_inlier: the error and the comparison of the step, score and mask kernels
#include "recover_pose_solve.h"    // gim_rp_jacobi3, gim_rp_order: the 3 x 3 eigen-decomposition of the rank-2 step

#if defined(__HIPCC__)
#define GIM_MR_FN __host__ __device__ inline
#else
#define GIM_MR_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GIM_MR_UNROLL _Pragma("unroll")
#else
#define GIM_MR_UNROLL
#endif

constexpr int GIM_MR_SWEEPS9 = 8;        // cyclic Jacobi sweeps over A^T A (36 rotations each)
constexpr int GIM_MR_LANES = 256;        // the lanes whose partial sums fix the summation order
constexpr int GIM_MR_TRI = 45;           // upper-triangle entries of a symmetric 9 x 9 matrix, row by row
constexpr int GIM_MR_MAX_ROUNDS = 8;
constexpr double GIM_MR_SQRT2 = 1.4142135623730951;
constexpr double GIM_MR_DBL_MAX = 1.7976931348623157e308;

GIM_MR_FN int gim_mr_min_points(int kind) { return kind == 0 ? 4 : 8; }
GIM_MR_FN bool gim_mr_finite(double x) { return fabs(x) <= GIM_MR_DBL_MAX; }

// a model that can be refitted: every entry finite, not all of them zero
GIM_MR_FN bool gim_mr_model_ok(const double* M) {
    bool finite = true, any = false;
    for (int i = 0; i < 9; ++i) finite = finite && gim_mr_finite(M[i]), any = any || M[i] != 0.0;
    return finite && any;
}

// Hartley's normalisation of one pair: centres and scales of both sides, q = (p - c) * s
struct gim_mr_norm {
    double ca[2], cb[2], sa, sb;
};

// centre = sum / n, then scale = sqrt(2) / (dist / n); false for a mean distance that is zero or not finite
GIM_MR_FN void gim_mr_centres(const double* sum4, int n, gim_mr_norm* N) {
    N->ca[0] = sum4[0] / n, N->ca[1] = sum4[1] / n, N->cb[0] = sum4[2] / n, N->cb[1] = sum4[3] / n;
}
GIM_MR_FN void gim_mr_dist(const gim_mr_norm& N, double ax, double ay, double bx, double by, double* d2) {
    const double px = ax - N.ca[0], py = ay - N.ca[1], qx = bx - N.cb[0], qy = by - N.cb[1];
    d2[0] = sqrt(px * px + py * py), d2[1] = sqrt(qx * qx + qy * qy);
}
GIM_MR_FN bool gim_mr_scales(const double* dist2, int n, gim_mr_norm* N) {
    const double ma = dist2[0] / n, mb = dist2[1] / n;
    if (!(ma > 0.0) || !(mb > 0.0) || !gim_mr_finite(ma) || !gim_mr_finite(mb)) return false;
    N->sa = GIM_MR_SQRT2 / ma, N->sb = GIM_MR_SQRT2 / mb;
    return true;
}

// adds one inlier's rows to the 45 upper-triangle sums: kind 0 the two rows of pose.homography_dlt, kind 1 the row of
// pose._epipolar_rows, both on the normalised point
template <int KIND>
GIM_MR_FN void gim_mr_accumulate(const gim_mr_norm& N, double ax, double ay, double bx, double by, double (&acc)[GIM_MR_TRI]) {
    const double x = (ax - N.ca[0]) * N.sa, y = (ay - N.ca[1]) * N.sa, u = (bx - N.cb[0]) * N.sb, v = (by - N.cb[1]) * N.sb;
    if (KIND == 0) {
        const double r1[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u};
        const double r2[9] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v};
        int k = 0;
        GIM_MR_UNROLL
        for (int i = 0; i < 9; ++i) {
            GIM_MR_UNROLL
            for (int j = i; j < 9; ++j, ++k) acc[k] += r1[i] * r1[j] + r2[i] * r2[j];
        }
    } else {
        const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int k = 0;
        GIM_MR_UNROLL
        for (int i = 0; i < 9; ++i) {
            GIM_MR_UNROLL
            for (int j = i; j < 9; ++j, ++k) acc[k] += r[i] * r[j];
        }
    }
}

// Cyclic Jacobi on the symmetric 9 x 9 matrix a (row-major [81], only its upper triangle is read and written), the eigenvectors as
// the columns of v [81]: the rotation of gim_rp_rotate (recover_pose_solve.h) with indices known at run time -- a and v live in
// LDS on the device, where such indexing costs no scratch.
GIM_MR_FN void gim_mr_jacobi9(double* a, double* v) {
    for (int i = 0; i < 81; ++i) v[i] = (i / 9 == i % 9) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < GIM_MR_SWEEPS9; ++sweep) {
        for (int p = 0; p < 8; ++p) {
            for (int q = p + 1; q < 9; ++q) {
                const double apq = a[9 * p + q];
                if (!(apq != 0.0)) continue;
                const double theta = (a[9 * q + q] - a[9 * p + p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
                a[9 * p + p] -= t * apq;
                a[9 * q + q] += t * apq;
                a[9 * p + q] = 0.0;
                for (int r = 0; r < 9; ++r) {
                    if (r == p || r == q) continue;
                    const int ip = r < p ? 9 * r + p : 9 * p + r, iq = r < q ? 9 * r + q : 9 * q + r;
                    const double g = a[ip], h = a[iq];
                    a[ip] = g - s * (h + tau * g);
                    a[iq] = h + s * (g - tau * h);
                }
                for (int r = 0; r < 9; ++r) {
                    const double g = v[9 * r + p], h = v[9 * r + q];
                    v[9 * r + p] = g - s * (h + tau * g);
                    v[9 * r + q] = h + s * (g - tau * h);
                }
            }
        }
    }
}

// kind 1: the nearest rank-2 matrix.  V from the eigenvectors of f^T f (gim_rp_jacobi3, largest eigenvalue first); with v2 the unit
// eigenvector of the smallest, f - (f v2) v2^T is f with its smallest singular value set to zero.
GIM_MR_FN void gim_mr_rank2(double* f) {
    double a[3][3], v[3][3];
    GIM_MR_UNROLL
    for (int i = 0; i < 3; ++i) {
        GIM_MR_UNROLL
        for (int j = 0; j < 3; ++j) {
            a[i][j] = (f[i] * f[j] + f[3 + i] * f[3 + j]) + f[6 + i] * f[6 + j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    gim_rp_jacobi3(a, v);
    double d[3] = {a[0][0], a[1][1], a[2][2]};
    gim_rp_order<0, 1>(d, v);
    gim_rp_order<0, 2>(d, v);
    gim_rp_order<1, 2>(d, v);
    double v2[3] = {v[0][2], v[1][2], v[2][2]};
    const double n = sqrt((v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2]);
    GIM_MR_UNROLL
    for (int i = 0; i < 3; ++i) v2[i] /= n;
    GIM_MR_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double w = (f[3 * i] * v2[0] + f[3 * i + 1] * v2[1]) + f[3 * i + 2] * v2[2];
        GIM_MR_UNROLL
        for (int j = 0; j < 3; ++j) f[3 * i + j] -= w * v2[j];
    }
}

// Steps 4 to 6 for one pair: tri [45] the summed upper triangle; a, v [81] work space (LDS on the device).  The eigenvector of the
// first smallest diagonal entry after the sweeps, rank 2 for kind 1, de-normalised with Ta, Tb (T = [s, 0, -s cx; 0, s, -s cy; 0, 0,
// 1]): kind 0 Tb^-1 h Ta scaled to h33 = 1, kind 1 Tb^T f Ta scaled to unit Frobenius norm.  false: a result that is not finite, a
// zero norm or h33 == 0.
GIM_MR_FN bool gim_mr_solve(int kind, const double* tri, const gim_mr_norm& N, double* a, double* v, double* out) {
    for (int i = 0, k = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) a[9 * i + j] = j >= i ? tri[k++] : 0.0;
    gim_mr_jacobi9(a, v);
    int kmin = 0;
    for (int k = 1; k < 9; ++k) kmin = a[10 * k] < a[10 * kmin] ? k : kmin;
    double f[9], m[9];
    GIM_MR_UNROLL
    for (int i = 0; i < 9; ++i) f[i] = v[9 * i + kmin];
    if (kind == 1) gim_mr_rank2(f);
    // m = f Ta
    GIM_MR_UNROLL
    for (int i = 0; i < 3; ++i) {
        m[3 * i] = f[3 * i] * N.sa, m[3 * i + 1] = f[3 * i + 1] * N.sa;
        m[3 * i + 2] = f[3 * i + 2] - N.sa * (f[3 * i] * N.ca[0] + f[3 * i + 1] * N.ca[1]);
    }
    double scale;
    if (kind == 0) {
        GIM_MR_UNROLL
        for (int j = 0; j < 3; ++j) {
            out[j] = m[j] / N.sb + N.cb[0] * m[6 + j];
            out[3 + j] = m[3 + j] / N.sb + N.cb[1] * m[6 + j];
            out[6 + j] = m[6 + j];
        }
        scale = out[8];
    } else {
        GIM_MR_UNROLL
        for (int j = 0; j < 3; ++j) {
            out[j] = N.sb * m[j];
            out[3 + j] = N.sb * m[3 + j];
            out[6 + j] = m[6 + j] - N.sb * (N.cb[0] * m[j] + N.cb[1] * m[3 + j]);
        }
        double ss = 0.0;
        GIM_MR_UNROLL
        for (int i = 0; i < 9; ++i) ss += out[i] * out[i];
        scale = sqrt(ss);
    }
    if (!(scale != 0.0) || !gim_mr_finite(scale)) return false;
    bool finite = true;
    GIM_MR_UNROLL
    for (int i = 0; i < 9; ++i) out[i] /= scale, finite = finite && gim_mr_finite(out[i]);
    return finite;
}

// The kernel's fixed summation order on the host: lane l adds its points l, l + 256, ... in ascending order, the 64 lanes of a wave
// are combined by the shuffle tree x[l] += x[l + o], o = 32 .. 1, and the four wave totals are added in wave order.
template <int K, typename F>
inline void gim_mr_block_sum(int P, const uint8_t* mask, double* total, F&& term) {
    static double lane[GIM_MR_LANES][K];    // the host check is single-threaded
    for (int l = 0; l < GIM_MR_LANES; ++l) {
        double acc[K];
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
        for (int p = l; p < P; p += GIM_MR_LANES)
            if (mask[p]) term(p, acc);
        for (int k = 0; k < K; ++k) lane[l][k] = acc[k];
    }
    for (int k = 0; k < K; ++k) {
        double w[4];
        for (int wave = 0; wave < 4; ++wave) {
            double x[64];
            for (int l = 0; l < 64; ++l) x[l] = lane[64 * wave + l][k];
            for (int o = 32; o > 0; o >>= 1)
                for (int l = 0; l < o; ++l) x[l] += x[l + o];
            w[wave] = x[0];
        }
        total[k] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}

// Steps 2 to 6 on the n points of a, b [P][2] whose mask byte is set (all of them finite), serially: pose.homography_dlt_ge /
// pose.eight_point_ge on the host.  false: no model (the stops of steps 2 and 6).
template <int KIND>
inline bool gim_mr_fit(const double* pa, const double* pb, int P, const uint8_t* mask, int n, double* model) {
    static double a[81], v[81];
    gim_mr_norm N;
    double s4[4], d2[2], tri[GIM_MR_TRI];
    gim_mr_block_sum<4>(P, mask, s4, [&](int p, double* acc) { acc[0] += pa[2 * p], acc[1] += pa[2 * p + 1], acc[2] += pb[2 * p], acc[3] += pb[2 * p + 1]; });
    gim_mr_centres(s4, n, &N);
    gim_mr_block_sum<2>(P, mask, d2, [&](int p, double* acc) {
        double d[2];
        gim_mr_dist(N, pa[2 * p], pa[2 * p + 1], pb[2 * p], pb[2 * p + 1], d);
        acc[0] += d[0], acc[1] += d[1];
    });
    if (!gim_mr_scales(d2, n, &N)) return false;
    gim_mr_block_sum<GIM_MR_TRI>(P, mask, tri, [&](int p, double* acc) {
        gim_mr_accumulate<KIND>(N, pa[2 * p], pa[2 * p + 1], pb[2 * p], pb[2 * p + 1], *reinterpret_cast<double(*)[GIM_MR_TRI]>(acc));
    });
    return gim_mr_solve(KIND, tri, N, a, v, model);
}

// The whole of gim_model_refit for one pair, serially (the host check): a, b [P][2], mask_in [P] or NULL -> model_out [9], mask_out
// [P], counts [2]; returns the rounds accepted, -1 for a skipped pair (then everything is zero).
template <int KIND>
inline int gim_mr_refit_kind(const double* pa, const double* pb, int P, const double* model_in, const uint8_t* mask_in, double thr2, int rounds,
                             double* model_out, uint8_t* mask_out, int32_t* counts) {
    counts[0] = counts[1] = 0;
    if (!gim_mr_model_ok(model_in)) {
        for (int i = 0; i < 9; ++i) model_out[i] = 0.0;
        for (int p = 0; p < P; ++p) mask_out[p] = 0;
        return -1;
    }
    double cur[9];
    for (int i = 0; i < 9; ++i) cur[i] = model_in[i];
    int n = 0;
    for (int p = 0; p < P; ++p) {
        mask_out[p] = mask_in ? (mask_in[p] != 0) : gim_tv_inlier(KIND, cur, pa[2 * p], pa[2 * p + 1], pb[2 * p], pb[2 * p + 1], thr2);
        n += mask_out[p];
    }
    counts[0] = n;
    int accepted = 0;
    for (int r = 0; r < rounds; ++r) {
        if (n < gim_mr_min_points(KIND)) break;
        bool finite = true;
        for (int p = 0; p < P; ++p)
            if (mask_out[p]) finite = finite && gim_mr_finite(pa[2 * p]) && gim_mr_finite(pa[2 * p + 1]) && gim_mr_finite(pb[2 * p]) && gim_mr_finite(pb[2 * p + 1]);
        if (!finite) break;
        double cand[9];
        if (!gim_mr_fit<KIND>(pa, pb, P, mask_out, n, cand)) break;
        int nc = 0, ndiff = 0;
        for (int p = 0; p < P; ++p) {
            const int in = gim_tv_inlier(KIND, cand, pa[2 * p], pa[2 * p + 1], pb[2 * p], pb[2 * p + 1], thr2) ? 1 : 0;
            nc += in, ndiff += in != mask_out[p];
            mask_out[p] |= (uint8_t)(in << 1);
        }
        const bool take = nc >= n;
        for (int p = 0; p < P; ++p) mask_out[p] = take ? (mask_out[p] >> 1) : (mask_out[p] & 1);
        if (!take) break;
        for (int i = 0; i < 9; ++i) cur[i] = cand[i];
        n = nc, ++accepted;
        if (ndiff == 0) break;
    }
    for (int i = 0; i < 9; ++i) model_out[i] = cur[i];
    counts[1] = n;
    return accepted;
}

inline int gim_mr_refit(int kind, const double* pa, const double* pb, int P, const double* model_in, const uint8_t* mask_in, double thr2, int rounds,
                        double* model_out, uint8_t* mask_out, int32_t* counts) {
    return kind == 0 ? gim_mr_refit_kind<0>(pa, pb, P, model_in, mask_in, thr2, rounds, model_out, mask_out, counts)
                     : gim_mr_refit_kind<1>(pa, pb, P, model_in, mask_in, thr2, rounds, model_out, mask_out, counts);
}
