// recoverPose for the pose half of the ZEB metric (gfx950): the decomposition of E into its four (R, t) candidates, the DLT
// triangulation of every match under each of them, the cheirality test, the four counts, the winner and its mask in one launch for a
// batch of pairs.  fp64 throughout, no fast-math flag on this file.
//
// The points are those the RANSAC step kernels already hold on the device (csrc/essential.hip), the input mask is the output of
// gim_ransac_mask: after the RANSAC a pair's pose costs this launch and one copy of R, t and the counts.
//
// Replaces (reference file:line): cv2.recoverPose(E, kpts0, kpts1, np.eye(3), 1e9, mask=mask) of tools/metrics.py:96-101
// (cv::decomposeEssentialMat, cv::triangulatePoints and the depth tests of cv::recoverPose in OpenCV's
// modules/calib3d/src/five-point.cpp); pose.recover_pose is the host's restatement with LAPACK's SVDs, pose.recover_pose_ge the
// arithmetic of this file in numpy.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/recover_pose_solve.h): both SVDs are cyclic Jacobi iterations with a fixed
// number of sweeps on the symmetric products E^T E (3 x 3) and A^T A (4 x 4); the null vector of a point's DLT matrix is the
// eigenvector of the smallest eigenvalue.  The divisions and square roots are IEEE; the compiler may contract a*b+c into an FMA where
// numpy rounds twice.
#include "gim_common.h"
#include "recover_pose_solve.h"

namespace {

constexpr int RP_THREADS = 256;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load

// grid = pairs: one workgroup owns one pair.  Lane 0 decomposes E[b] and leaves the four candidates in LDS (48 doubles).  After a
// barrier every lane walks the pair's points, 256 per pass, coalesced 16-byte loads; per point the four candidates in turn (a
// broadcast read from LDS each), the 4 x 4 matrices in registers; the point's four bits go to its own byte of mask_out.  The four
// partial counts are summed by wave shuffles and one LDS word per wave and candidate: integer sums, no atomics, so the result does
// not depend on the launch shape.  Every lane then knows the winner and turns the bytes it wrote itself into the winner's 0 / 1.
__global__ void __launch_bounds__(RP_THREADS) recover_pose_kernel(const double* __restrict__ E, const f64x2_t* __restrict__ x0,
                                                                  const f64x2_t* __restrict__ x1, const int32_t* __restrict__ offsets,
                                                                  const uint8_t* __restrict__ mask_in, double dthr, double* __restrict__ R,
                                                                  double* __restrict__ t, int32_t* __restrict__ n_good,
                                                                  int32_t* __restrict__ best, uint8_t* mask_out) {
    __shared__ double sC[4 * GIM_RP_CAND];
    __shared__ int sOk;
    __shared__ int sCnt[RP_THREADS / 64][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    if (tid == 0) {
        double e[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) e[i] = E[(int64_t)b * 9 + i];
        sOk = gim_rp_decompose(e, sC) ? 1 : 0;                 // the candidates go straight to LDS
    }
    __syncthreads();
    if (sOk == 0) {                                           // workgroup-uniform
        for (int p = tid; p < n; p += RP_THREADS) mask_out[(int64_t)base + p] = 0;
        if (tid < 9) R[(int64_t)b * 9 + tid] = 0.0;
        if (tid < 3) t[(int64_t)b * 3 + tid] = 0.0;
        if (tid < 4) n_good[(int64_t)b * 4 + tid] = 0;
        if (tid == 0) best[b] = -1;
        return;
    }
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int p = tid; p < n; p += RP_THREADS) {
        int bits = 0;
        if (mask_in == nullptr || mask_in[(int64_t)base + p] != 0) {
            const f64x2_t a = x0[(int64_t)base + p], d = x1[(int64_t)base + p];
#pragma unroll 1
            for (int j = 0; j < 4; ++j) bits |= (gim_rp_point(sC + GIM_RP_CAND * j, a.x, a.y, d.x, d.y, dthr) ? 1 : 0) << j;
        }
        mask_out[(int64_t)base + p] = (uint8_t)bits;
        c0 += bits & 1, c1 += (bits >> 1) & 1, c2 += (bits >> 2) & 1, c3 += (bits >> 3) & 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c0 += __shfl_down(c0, o, 64), c1 += __shfl_down(c1, o, 64);
        c2 += __shfl_down(c2, o, 64), c3 += __shfl_down(c3, o, 64);
    }
    if ((tid & 63) == 0) sCnt[tid >> 6][0] = c0, sCnt[tid >> 6][1] = c1, sCnt[tid >> 6][2] = c2, sCnt[tid >> 6][3] = c3;
    __syncthreads();
    int g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = (sCnt[0][j] + sCnt[1][j]) + (sCnt[2][j] + sCnt[3][j]);
    const int k = gim_rp_best(g[0], g[1], g[2], g[3]);        // workgroup-uniform
    if (tid < 9) R[(int64_t)b * 9 + tid] = sC[GIM_RP_CAND * k + tid];
    if (tid < 3) t[(int64_t)b * 3 + tid] = sC[GIM_RP_CAND * k + 9 + tid];
    if (tid < 4) n_good[(int64_t)b * 4 + tid] = tid == 0 ? g[0] : tid == 1 ? g[1] : tid == 2 ? g[2] : g[3];
    if (tid == 0) best[b] = k;
    for (int p = tid; p < n; p += RP_THREADS) {               // the bytes this lane wrote above
        const int64_t i = (int64_t)base + p;
        mask_out[i] = (uint8_t)((mask_out[i] >> k) & 1);
    }
}

}  // namespace

extern "C" int gim_recover_pose(const double* E, const double* x0, const double* x1, const int32_t* offsets, int B,
                                const uint8_t* mask_in, double distance_thresh, double* R, double* t, int32_t* n_good, int32_t* best,
                                uint8_t* mask_out, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && B <= 65535, "gim_recover_pose: B=%d (0 <= B <= 65535)", B);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(E && x0 && x1 && offsets && R && t && n_good && best && mask_out, "gim_recover_pose: NULL pointer");
    GIM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1) & 15) == 0, "gim_recover_pose: x0 and x1 must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)E | (uintptr_t)R | (uintptr_t)t) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)n_good | (uintptr_t)best) & 3) == 0,
                "gim_recover_pose: misaligned E, R, t, offsets, n_good or best");
    hipLaunchKernelGGL(recover_pose_kernel, dim3((unsigned)B), dim3(RP_THREADS), 0, (hipStream_t)stream, E, (const f64x2_t*)x0,
                       (const f64x2_t*)x1, offsets, mask_in, distance_thresh, R, t, n_good, best, mask_out);
    return gim_check_launch("recover_pose_kernel");
}
