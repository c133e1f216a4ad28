// Fundamental-matrix RANSAC step for the demo's match filter and for pair-list verification (gfx950): the seven-point minimal solve AND
// the inlier counts of its up to three models in one launch.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py draws the samples; a step uploads only its sample indices [B][K][7] and reads back models, flags and counts.  The
// points stay on the device, as for csrc/ransac_score.hip and csrc/homography.hip; the final mask is gim_ransac_mask.  The five-point
// solver (a 10 x 10 non-symmetric eigenproblem) is csrc/essential.hip.
//
// Replaces (reference file:line): the minimal solve and the scoring inside cv2.findFundamentalMat(mkpts0, mkpts1, ...) of demo.py:514-517
// (FMEstimatorCallback::runKernel / run7Point and ::computeError of OpenCV's modules/calib3d/src/fundam.cpp, the inlier count of
// RANSACPointSetRegistrator::run); pose.seven_point_ge / pose.sampson_error of this project are the same arithmetic in batched numpy.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/fundamental_solve.h): per sample both sides are shifted to zero mean and scaled
// to mean distance sqrt(2); the 7 x 9 epipolar rows are reduced by Gauss-Jordan elimination with full pivoting; the cubic
// det(a F1 + (1 - a) F2) is interpolated at a = 0, 1, -1, 2 (a cubic that vanishes identically is refused) and solved in closed form
// with two Newton steps per root; each root's F is de-normalised and scaled to unit Frobenius norm.  The counts are
// two_view_residual.h's (kind 1).  The divisions are IEEE; the compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "fundamental_solve.h"
#include "ransac_body.h"

namespace {

// Lane 0 gathers the seven correspondences, checks and solves the sample in LDS (63 doubles, indexed at run time by the pivoting) and
// leaves its three models there; after one barrier rb_count_models counts all three over the pair's points (ransac_body.h).
__global__ void __launch_bounds__(RB_THREADS) fundamental_step_kernel(const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                      const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                      int K, double thr2, double* __restrict__ models,
                                                                      uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
    __shared__ double sA[63];
    __shared__ double sF[27];
    __shared__ int sOk[3];
    __shared__ int sCnt[RB_WAVES][3];
    const int b = blockIdx.y, k = blockIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    const int64_t mk = (int64_t)b * K + k;
    if (threadIdx.x == 0) {
        double p0[14], p1[14], F[27];
        bool ok[3] = {false, false, false};
        if (rb_gather_sample<7>(x0, x1, idx, mk, base, n, p0, p1)) gim_f7_solve(p0, p1, sA, F, ok);
#pragma unroll
        for (int j = 0; j < 3; ++j) rb_publish_model(ok[j], F + 9 * j, sF + 9 * j, sOk + j, models + (mk * 3 + j) * 9, valid + mk * 3 + j);
    }
    __syncthreads();
    rb_count_models<GIM_TV_EPIPOLAR, 3>(x0, x1, base, n, sF, sOk, sCnt, thr2, counts + mk * 3);
}

}  // namespace

extern "C" int gim_fundamental_step(const double* x0, const double* x1, const int32_t* offsets, int B, const int32_t* idx, int K,
                                    double thr2, double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_fundamental_step: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    if (int e = rb_check_launch("gim_fundamental_step", (int64_t)B * K, 27, "samples", x0 && x1 && offsets && idx && models && valid && counts,
                                x0, x1, "x0", "x1", rb_aligned8(models) && rb_aligned4(offsets, idx, counts),
                                "models, offsets, idx or counts"))
        return e;
    hipLaunchKernelGGL(fundamental_step_kernel, dim3((unsigned)K, (unsigned)B), dim3(RB_THREADS), 0, (hipStream_t)stream,
                       (const f64x2_t*)x0, (const f64x2_t*)x1, offsets, idx, K, thr2, models, valid, counts);
    return gim_check_launch("fundamental_step_kernel");
}
