// Essential-matrix RANSAC step for the pose half of the ZEB metric (gfx950): the five-point minimal solve AND the inlier counts of its
// up to ten models in one launch.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py draws the samples; a step uploads only its sample indices [B][K][5] and reads back models, flags and counts.  The
// points stay on the device, as for csrc/ransac_score.hip, csrc/homography.hip and csrc/fundamental.hip; the final mask is
// gim_ransac_mask.  recoverPose is csrc/recover_pose.hip, on the same points.
//
// Replaces (reference file:line): the minimal solve and the scoring inside cv2.findEssentialMat(kpts0, kpts1, np.eye(3), threshold,
// prob, method=cv2.RANSAC) of tools/metrics.py:88-89 (EMEstimatorCallback::runKernel and ::computeError of OpenCV's
// modules/calib3d/src/five-point.cpp, the inlier count of RANSACPointSetRegistrator::run); pose.five_point_ge / pose.sampson_error
// of this project are the same arithmetic in numpy.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/essential_solve.h): the 5 x 9 epipolar rows are reduced by Gauss-Jordan
// elimination with full pivoting, the four free columns give the basis X, Y, Z, W; the ten cubic constraints on E = x X + y Y + z Z + W
// are accumulated over the 20 monomials and reduced to [I | B]; the eigenvalues of the 10 x 10 action matrix of multiplication by x
// come from a Householder reduction to Hessenberg form and the real double-shift QR iteration; each real eigenvalue's null vector
// (elimination with full pivoting) gives (x, y, z) and its E, scaled to unit Frobenius norm.  The counts are two_view_residual.h's
// (kind 1).  The divisions are IEEE; the compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "essential_solve.h"
#include "ransac_body.h"

namespace {

// Lane 0 gathers the five correspondences, checks them and runs the serial phases (null space, constraints, reduction, eigenvalues)
// in LDS: everything indexed at run time lives there (GIM_E5_WORK doubles, 10 976 bytes).  After a barrier the lanes 0 .. 9 take one
// real root each (its own 10 x 10 system in LDS) and leave its model in LDS and in the output; after a second barrier
// rb_count_models counts all ten over the pair's points (ransac_body.h).
__global__ void __launch_bounds__(RB_THREADS) essential_step_kernel(const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                    const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                    int K, double thr2, double* __restrict__ models,
                                                                    uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
    __shared__ double sW[GIM_E5_WORK];
    __shared__ double sE[90];
    __shared__ int sN;
    __shared__ int sOk[10];
    __shared__ int sCnt[RB_WAVES][10];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    const int64_t mk = (int64_t)b * K + k;
    if (tid == 0) {
        double p0[10], p1[10];
        sN = rb_gather_sample<5>(x0, x1, idx, mk, base, n, p0, p1) ? gim_e5_roots(p0, p1, sW) : 0;
    }
    __syncthreads();
    if (tid < 10) {
        double E[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = 0.0;
        const bool ok = tid < sN && gim_e5_model(sW, sW[GIM_E5_ROOTS + tid], sW + GIM_E5_SYS + 100 * tid, E);
        rb_publish_model(ok, E, sE + 9 * tid, sOk + tid, models + (mk * 10 + tid) * 9, valid + mk * 10 + tid);
    }
    __syncthreads();
    rb_count_models<GIM_TV_EPIPOLAR, 10>(x0, x1, base, n, sE, sOk, sCnt, thr2, counts + mk * 10);
}

}  // namespace

extern "C" int gim_essential_step(const double* x0, const double* x1, const int32_t* offsets, int B, const int32_t* idx, int K,
                                  double thr2, double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_essential_step: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    if (int e = rb_check_launch("gim_essential_step", (int64_t)B * K, 90, "samples", x0 && x1 && offsets && idx && models && valid && counts,
                                x0, x1, "x0", "x1", rb_aligned8(models) && rb_aligned4(offsets, idx, counts),
                                "models, offsets, idx or counts"))
        return e;
    hipLaunchKernelGGL(essential_step_kernel, dim3((unsigned)K, (unsigned)B), dim3(RB_THREADS), 0, (hipStream_t)stream,
                       (const f64x2_t*)x0, (const f64x2_t*)x1, offsets, idx, K, thr2, models, valid, counts);
    return gim_check_launch("essential_step_kernel");
}
