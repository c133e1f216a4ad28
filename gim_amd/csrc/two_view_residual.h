// The two residuals of the pose half and their inlier rule, written once for the device and the host: every kernel that counts, masks,
// scores or refits (ransac_score.hip, homography.hip, fundamental.hip, essential.hip, model_refit.hip) and every host check under
// tools/ calls these, so a step's count, the scorer's count, a mask's sum, the MAGSAC count and the refit's starting count are the
// same number for the same model by construction.  A new residual is added here and nowhere else.  fp64, plain C++; the divisions
// are IEEE, and the compiler may contract a*b+c into an FMA where numpy rounds twice.
//
// kind 1 (GIM_TV_EPIPOLAR), a fundamental or essential matrix M: the Sampson error (x1^T M x0)^2 / max(|M x0|_xy^2 + |M^T x1|_xy^2,
// 1e-300) of pose.sampson_error (EMEstimatorCallback / FMEstimatorCallback::computeError of OpenCV).  A NaN anywhere fails the
// comparison; an all-zero model gives 0 / 1e-300 = 0 and counts every point, as numpy does.
// kind 0 (GIM_TV_HOMOGRAPHY), b ~ M a: the forward transfer error |b - proj(M a)|^2 of pose.transfer_error
// (HomographyEstimatorCallback::computeError, in fp64); NaN when w == 0, and an error that is not finite is an outlier.
// The numbering is the `kind` of gim_magsac_score and gim_model_refit (include/gim_hip.h).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GIM_TV_FN __host__ __device__ inline
#else
#define GIM_TV_FN inline
#endif

constexpr int GIM_TV_HOMOGRAPHY = 0;
constexpr int GIM_TV_EPIPOLAR = 1;

GIM_TV_FN double gim_tv_sampson(const double* m, double ax, double ay, double bx, double by) {
    const double r0 = m[0] * ax + m[1] * ay + m[2];          // M x0
    const double r1 = m[3] * ax + m[4] * ay + m[5];
    const double r2 = m[6] * ax + m[7] * ay + m[8];
    const double c0 = m[0] * bx + m[3] * by + m[6];          // M^T x1, first two rows
    const double c1 = m[1] * bx + m[4] * by + m[7];
    const double e = r0 * bx + r1 * by + r2;                 // x1^T M x0
    const double den = r0 * r0 + r1 * r1 + c0 * c0 + c1 * c1;
    return (e * e) / (den < 1e-300 ? 1e-300 : den);          // np.maximum(den, 1e-300): a NaN den stays NaN
}

GIM_TV_FN double gim_tv_transfer(const double* H, double sx, double sy, double dx, double dy) {
    const double w = H[6] * sx + H[7] * sy + H[8];
    if (w == 0.0) return NAN;                                // no projection, no residual
    const double ex = dx - (H[0] * sx + H[1] * sy + H[2]) / w;
    const double ey = dy - (H[3] * sx + H[4] * sy + H[5]) / w;
    return ex * ex + ey * ey;
}

GIM_TV_FN double gim_tv_error(int kind, const double* M, double ax, double ay, double bx, double by) {
    return kind == GIM_TV_HOMOGRAPHY ? gim_tv_transfer(M, ax, ay, bx, by) : gim_tv_sampson(M, ax, ay, bx, by);
}

// err <= thr2.  kind 0: w != 0 && isfinite(e) && e <= thr2 (the NaN of w == 0 is not finite); kind 1: the bare comparison, which
// a NaN fails.
GIM_TV_FN bool gim_tv_within(int kind, double err, double thr2) {
    return kind == GIM_TV_HOMOGRAPHY ? isfinite(err) && err <= thr2 : err <= thr2;
}

GIM_TV_FN bool gim_tv_inlier(int kind, const double* M, double ax, double ay, double bx, double by, double thr2) {
    return gim_tv_within(kind, gim_tv_error(kind, M, ax, ay, bx, by), thr2);
}
