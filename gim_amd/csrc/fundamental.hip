// Fundamental-matrix RANSAC step for the demo's match filter and for pair-list verification (gfx950): the seven-point minimal solve AND
// the inlier counts of its up to three models in one launch.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py draws the samples; a step uploads only its sample indices [B][K][7] and reads back models, flags and counts.  The
// points stay on the device, as for csrc/ransac_score.hip and csrc/homography.hip; the final mask is gim_ransac_mask (the same Sampson
// error).  The five-point solver (a 10 x 10 non-symmetric eigenproblem) is csrc/essential.hip.
//
// Replaces (reference file:line): the minimal solve and the scoring inside cv2.findFundamentalMat(mkpts0, mkpts1, ...) of demo.py:514-517
// (FMEstimatorCallback::runKernel / run7Point and ::computeError of OpenCV's modules/calib3d/src/fundam.cpp, the inlier count of
// RANSACPointSetRegistrator::run); pose.seven_point_ge / pose.sampson_error of this project are the same arithmetic in batched numpy.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/fundamental_solve.h): per sample both sides are shifted to zero mean and scaled
// to mean distance sqrt(2); the 7 x 9 epipolar rows are reduced by Gauss-Jordan elimination with full pivoting; the cubic
// det(a F1 + (1 - a) F2) is interpolated at a = 0, 1, -1, 2 (a cubic that vanishes identically is refused) and solved in closed form
// with two Newton steps per root; each root's F is de-normalised and scaled to unit Frobenius norm.  The divisions are IEEE; the
// compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "fundamental_solve.h"

namespace {

constexpr int FM_THREADS = 256;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load

// grid = (samples, pairs): one workgroup owns one sample.  Lane 0 gathers the seven correspondences, checks and solves the sample in
// LDS (63 doubles, indexed at run time by the pivoting) and leaves its three models there; after one barrier every lane reads them
// (a broadcast read) and walks the pair's points once, 256 per pass, coalesced 16-byte loads, every valid model against each loaded
// point.  The three partial counts are summed by wave shuffles and one LDS word per wave and model: integer sums, one plain store
// per output, no atomics and no memset.
__global__ void __launch_bounds__(FM_THREADS) fundamental_step_kernel(const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                      const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                      int K, double thr2, double* __restrict__ models,
                                                                      uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
    __shared__ double sA[63];
    __shared__ double sF[27];
    __shared__ int sOk[3];
    __shared__ int sCnt[FM_THREADS / 64][3];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    const int64_t mk = (int64_t)b * K + k;
    if (tid == 0) {
        int id[7];
        bool in = true;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            id[i] = idx[mk * 7 + i];
            in = in && id[i] >= 0 && id[i] < n;                // an index outside the pair never becomes an address
        }
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = i + 1; j < 7; ++j) in = in && id[i] != id[j];
        double F[27];
        bool ok[3] = {false, false, false};
        if (in) {
            double p0[14], p1[14];
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const f64x2_t a = x0[(int64_t)base + id[i]], d = x1[(int64_t)base + id[i]];
                p0[2 * i] = a.x, p0[2 * i + 1] = a.y, p1[2 * i] = d.x, p1[2 * i + 1] = d.y;
            }
            gim_f7_solve(p0, p1, sA, F, ok);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double v = in && ok[j] ? F[9 * j + i] : 0.0;
                sF[9 * j + i] = v;
                models[mk * 27 + 9 * j + i] = v;
            }
            const int o = in && ok[j] ? 1 : 0;
            valid[mk * 3 + j] = (uint8_t)o;
            sOk[j] = o;
        }
    }
    __syncthreads();
    const bool ok0 = sOk[0] != 0, ok1 = sOk[1] != 0, ok2 = sOk[2] != 0;   // workgroup-uniform
    if (!(ok0 || ok1 || ok2)) {
        if (tid < 3) counts[mk * 3 + tid] = 0;
        return;
    }
    double F0[9], F1[9], F2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F0[i] = sF[i], F1[i] = sF[9 + i], F2[i] = sF[18 + i];
    int c0 = 0, c1 = 0, c2 = 0;
    for (int p = tid; p < n; p += FM_THREADS) {
        const f64x2_t a = x0[(int64_t)base + p], d = x1[(int64_t)base + p];
        if (ok0) c0 += gim_f7_inlier(F0, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
        if (ok1) c1 += gim_f7_inlier(F1, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
        if (ok2) c2 += gim_f7_inlier(F2, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c0 += __shfl_down(c0, o, 64);
        c1 += __shfl_down(c1, o, 64);
        c2 += __shfl_down(c2, o, 64);
    }
    if ((tid & 63) == 0) sCnt[tid >> 6][0] = c0, sCnt[tid >> 6][1] = c1, sCnt[tid >> 6][2] = c2;
    __syncthreads();
    if (tid < 3) counts[mk * 3 + tid] = sCnt[0][tid] + sCnt[1][tid] + sCnt[2][tid] + sCnt[3][tid];
}

}  // namespace

extern "C" int gim_fundamental_step(const double* x0, const double* x1, const int32_t* offsets, int B, const int32_t* idx, int K,
                                    double thr2, double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_fundamental_step: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K <= 0x7fffffffLL / 27, "gim_fundamental_step: B*K=%lld samples", (long long)B * K);
    GIM_REQUIRE(x0 && x1 && offsets && idx && models && valid && counts, "gim_fundamental_step: NULL pointer");
    GIM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1) & 15) == 0, "gim_fundamental_step: x0 and x1 must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)idx | (uintptr_t)counts) & 3) == 0,
                "gim_fundamental_step: misaligned models, offsets, idx or counts");
    hipLaunchKernelGGL(fundamental_step_kernel, dim3((unsigned)K, (unsigned)B), dim3(FM_THREADS), 0, (hipStream_t)stream,
                       (const f64x2_t*)x0, (const f64x2_t*)x1, offsets, idx, K, thr2, models, valid, counts);
    return gim_check_launch("fundamental_step_kernel");
}
