// Homography RANSAC step for the demo's geometry (gfx950): the four-point minimal solve AND the inlier count of every hypothesis in one
// launch.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py draws the samples; the four-point homography is one 8 x 8 linear solve, so a step uploads only its sample indices
// [B][K][4] and reads back models, flags and counts.  The points stay on the device, as for csrc/ransac_score.hip; the final mask is
// gim_homography_mask there.
//
// Replaces (reference file:line): cv2.findHomography(mkpts1, mkpts0, ...) inside compute_geom, demo.py:180-227, i.e. the minimal solve
// (HomographyEstimatorCallback::runKernel), the sample check (::checkSubset) and the scoring (::computeError + the inlier count of
// RANSACPointSetRegistrator::run) of OpenCV's modules/calib3d/src/fundam.cpp and ptsetreg.cpp; pose.homography_4pt / pose.transfer_error
// of this project are the same arithmetic in batched numpy.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/homography_solve.h): per sample both sides are shifted to zero mean and scaled to
// mean distance sqrt(2); the 8 x 9 augmented system of dst ~ H src with h33 = 1 is reduced by Gaussian elimination with partial
// pivoting; H is de-normalised and scaled to h33 = 1.  The count is two_view_residual.h's (kind 0).  The divisions are IEEE; the
// compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "homography_solve.h"
#include "ransac_body.h"

namespace {

// Lane 0 gathers the four correspondences, checks and solves the sample in LDS (72 doubles, indexed at run time by the pivoting) and
// leaves H there; after one barrier rb_count_models counts over the pair's points (ransac_body.h).
__global__ void __launch_bounds__(RB_THREADS) homography_step_kernel(const f64x2_t* __restrict__ src, const f64x2_t* __restrict__ dst,
                                                                     const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                     int K, double thr2, double* __restrict__ models,
                                                                     uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
    __shared__ double sA[72];
    __shared__ double sH[9];
    __shared__ int sOk[1];
    __shared__ int sCnt[RB_WAVES][1];
    const int b = blockIdx.y, k = blockIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    const int64_t mk = (int64_t)b * K + k;
    if (threadIdx.x == 0) {
        double ps[8], pd[8], H[9];
        bool ok = rb_gather_sample<4>(src, dst, idx, mk, base, n, ps, pd);
        if (ok) ok = gim_h4_solve(ps, pd, sA, H);
        rb_publish_model(ok, H, sH, sOk, models + mk * 9, valid + mk);
    }
    __syncthreads();
    rb_count_models<GIM_TV_HOMOGRAPHY, 1>(src, dst, base, n, sH, sOk, sCnt, thr2, counts + mk);
}

}  // namespace

extern "C" int gim_homography_step(const double* src, const double* dst, const int32_t* offsets, int B, const int32_t* idx, int K,
                                   double thr2, double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_homography_step: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    if (int e = rb_check_launch("gim_homography_step", (int64_t)B * K, 9, "hypotheses", src && dst && offsets && idx && models && valid && counts,
                                src, dst, "src", "dst", rb_aligned8(models) && rb_aligned4(offsets, idx, counts),
                                "models, offsets, idx or counts"))
        return e;
    hipLaunchKernelGGL(homography_step_kernel, dim3((unsigned)K, (unsigned)B), dim3(RB_THREADS), 0, (hipStream_t)stream,
                       (const f64x2_t*)src, (const f64x2_t*)dst, offsets, idx, K, thr2, models, valid, counts);
    return gim_check_launch("homography_step_kernel");
}
