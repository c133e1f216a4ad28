// Essential-matrix RANSAC step for the pose half of the ZEB metric (gfx950): the five-point minimal solve AND the inlier counts of its
// up to ten models in one launch.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py draws the samples; a step uploads only its sample indices [B][K][5] and reads back models, flags and counts.  The
// points stay on the device, as for csrc/ransac_score.hip, csrc/homography.hip and csrc/fundamental.hip; the final mask is
// gim_ransac_mask (the same Sampson error).  recoverPose is csrc/recover_pose.hip, on the same points.
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
// (elimination with full pivoting) gives (x, y, z) and its E, scaled to unit Frobenius norm.  The divisions are IEEE; the compiler may
// contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "essential_solve.h"
#include "fundamental_solve.h"   // gim_f7_inlier: the Sampson rule of gim_ransac_score

namespace {

constexpr int EM_THREADS = 256;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load

// grid = (samples, pairs): one workgroup owns one sample.  Lane 0 gathers the five correspondences, checks them and runs the serial
// phases (null space, constraints, reduction, eigenvalues) in LDS: everything indexed at run time lives there (GIM_E5_WORK doubles,
// 10 976 bytes).  After a barrier the lanes 0 .. 9 take one real root each (its own 10 x 10 system in LDS) and leave its model in LDS
// and in the output; after a second barrier every lane walks the pair's points once, 256 per pass, coalesced 16-byte loads, every
// valid model (a broadcast read from LDS) against each loaded point.  The ten partial counts are summed by wave shuffles and one
// LDS word per wave and model: integer sums, one plain store per output, no atomics and no memset.
__global__ void __launch_bounds__(EM_THREADS) essential_step_kernel(const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                    const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                    int K, double thr2, double* __restrict__ models,
                                                                    uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
    __shared__ double sW[GIM_E5_WORK];
    __shared__ double sE[90];
    __shared__ int sN;
    __shared__ int sOk[10];
    __shared__ int sCnt[EM_THREADS / 64][10];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    const int64_t mk = (int64_t)b * K + k;
    if (tid == 0) {
        int id[5];
        bool in = true;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            id[i] = idx[mk * 5 + i];
            in = in && id[i] >= 0 && id[i] < n;                // an index outside the pair never becomes an address
        }
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = i + 1; j < 5; ++j) in = in && id[i] != id[j];
        int nr = 0;
        if (in) {
            double p0[10], p1[10];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const f64x2_t a = x0[(int64_t)base + id[i]], d = x1[(int64_t)base + id[i]];
                p0[2 * i] = a.x, p0[2 * i + 1] = a.y, p1[2 * i] = d.x, p1[2 * i + 1] = d.y;
            }
            nr = gim_e5_roots(p0, p1, sW);
        }
        sN = nr;
    }
    __syncthreads();
    if (tid < 10) {
        double E[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = 0.0;
        const bool ok = tid < sN && gim_e5_model(sW, sW[GIM_E5_ROOTS + tid], sW + GIM_E5_SYS + 100 * tid, E);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double v = ok ? E[i] : 0.0;
            sE[9 * tid + i] = v;
            models[mk * 90 + 9 * tid + i] = v;
        }
        valid[mk * 10 + tid] = (uint8_t)(ok ? 1 : 0);
        sOk[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    int okmask = 0;                                           // workgroup-uniform
#pragma unroll
    for (int j = 0; j < 10; ++j) okmask |= (sOk[j] != 0 ? 1 : 0) << j;
    if (okmask == 0) {
        if (tid < 10) counts[mk * 10 + tid] = 0;
        return;
    }
    int c[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) c[j] = 0;
    for (int p = tid; p < n; p += EM_THREADS) {
        const f64x2_t a = x0[(int64_t)base + p], d = x1[(int64_t)base + p];
#pragma unroll
        for (int j = 0; j < 10; ++j)
            if ((okmask >> j) & 1) c[j] += gim_f7_inlier(sE + 9 * j, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[j] += __shfl_down(c[j], o, 64);
        if ((tid & 63) == 0) sCnt[tid >> 6][j] = c[j];
    }
    __syncthreads();
    if (tid < 10) counts[mk * 10 + tid] = sCnt[0][tid] + sCnt[1][tid] + sCnt[2][tid] + sCnt[3][tid];
}

}  // namespace

extern "C" int gim_essential_step(const double* x0, const double* x1, const int32_t* offsets, int B, const int32_t* idx, int K,
                                  double thr2, double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_essential_step: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K <= 0x7fffffffLL / 90, "gim_essential_step: B*K=%lld samples", (long long)B * K);
    GIM_REQUIRE(x0 && x1 && offsets && idx && models && valid && counts, "gim_essential_step: NULL pointer");
    GIM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1) & 15) == 0, "gim_essential_step: x0 and x1 must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)idx | (uintptr_t)counts) & 3) == 0,
                "gim_essential_step: misaligned models, offsets, idx or counts");
    hipLaunchKernelGGL(essential_step_kernel, dim3((unsigned)K, (unsigned)B), dim3(EM_THREADS), 0, (hipStream_t)stream,
                       (const f64x2_t*)x0, (const f64x2_t*)x1, offsets, idx, K, thr2, models, valid, counts);
    return gim_check_launch("essential_step_kernel");
}
