// RANSAC hypothesis scoring for the pose half of the ZEB loop (gfx950): inlier counts of many 3x3 models over the matched points of
// one or several pairs, and the inlier mask of one model per pair.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py solves 250 minimal samples (2 500 candidate essential matrices) per RANSAC step on the host and then needs, for
// every candidate, the number of points whose Sampson error is below the threshold: 2 500 x 2 000 evaluations, about 90 % of the
// host step.  This file is that reduction; sampling, the minimal solvers, the iteration bound and recoverPose stay on the host.
//
// Replaces (reference file:line): the scoring inside cv2.findEssentialMat / cv2.findFundamentalMat as called from
// tools/metrics.py:77-103 and demo.py:514-517 (EMEstimatorCallback::computeError + the inlier count of
// RANSACPointSetRegistrator::run), i.e. pose.sampson_error / pose._count_inliers of this project.
//
// Arithmetic (the contract of include/gim_hip.h): err = (x1^T M x0)^2 / max(|M x0|_xy^2 + |M^T x1|_xy^2, 1e-300), inlier when
// err <= thr2.  A NaN anywhere makes the comparison false; an all-zero model gives 0 / 1e-300 = 0 and counts every point, as numpy does.
// The division is IEEE (no reciprocal approximation); the compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"

namespace {

constexpr int RS_THREADS = 256;   // one model per lane
constexpr int RS_TP = 64;         // points staged per LDS tile: 64 x (x0.x, x0.y, x1.x, x1.y) fp64 = 2 KiB
constexpr int RS_MAX_SPLITS = 64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load, global or LDS

__device__ __forceinline__ bool sampson_inlier(const double (&m)[9], double ax, double ay, double bx, double by, double thr2) {
    const double r0 = m[0] * ax + m[1] * ay + m[2];          // M x0
    const double r1 = m[3] * ax + m[4] * ay + m[5];
    const double r2 = m[6] * ax + m[7] * ay + m[8];
    const double c0 = m[0] * bx + m[3] * by + m[6];          // M^T x1, first two rows
    const double c1 = m[1] * bx + m[4] * by + m[7];
    const double e = r0 * bx + r1 * by + r2;                 // x1^T M x0
    const double den = r0 * r0 + r1 * r1 + c0 * c0 + c1 * c1;
    return (e * e) / (den < 1e-300 ? 1e-300 : den) <= thr2;  // np.maximum(den, 1e-300): a NaN den stays NaN and fails the comparison
}

// grid = (model tiles of 256, point splits, pairs).  A lane keeps its model's nine coefficients in registers; the workgroup stages 64
// points in LDS and every lane reads the same point (a broadcast read: no bank conflict).  A workgroup walks the point tiles
// blockIdx.y, blockIdx.y + gridDim.y, ... of its pair, so the launch needs no point count on the host; its partial count goes to
// counts[] with one integer atomic per model (counts[] is zeroed by the entry point: integer sums, any order, same result).
__global__ void __launch_bounds__(RS_THREADS) ransac_score_kernel(const double* __restrict__ models, const uint8_t* __restrict__ valid,
                                                                  const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                  const int32_t* __restrict__ offsets, int K, double thr2,
                                                                  int32_t* __restrict__ counts) {
    __shared__ f64x2_t pts[2][RS_TP];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int k = blockIdx.x * RS_THREADS + tid;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform: the loop below and its barriers are too
    const int64_t mk = (int64_t)b * K + k;
    const bool live = k < K && (valid == nullptr || valid[mk] != 0);
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = live ? models[mk * 9 + i] : 0.0;
    if (__syncthreads_count(live) == 0) return;              // a tile of padding or of a finished pair (workgroup-uniform)
    int cnt = 0;
    for (int c = blockIdx.y * RS_TP; c < n; c += gridDim.y * RS_TP) {
        __syncthreads();                                      // the previous tile has been read by every lane
        if (tid < 2 * RS_TP) {
            const int side = tid / RS_TP, q = tid % RS_TP;
            f64x2_t v = {0.0, 0.0};
            if (c + q < n) v = (side ? x1 : x0)[(int64_t)base + c + q];
            pts[side][q] = v;
        }
        __syncthreads();
        const int np = min(RS_TP, n - c);
#pragma unroll 4
        for (int q = 0; q < np; ++q) {
            const f64x2_t a = pts[0][q], d = pts[1][q];
            cnt += sampson_inlier(m, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
        }
    }
    if (live && cnt) atomicAdd(&counts[mk], cnt);
}

// grid = (point blocks, pairs): one point per lane, the pair's model in registers (uniform over the workgroup), grid-stride over the
// pair's points.  Every point of [offsets[0], offsets[B]) is written exactly once.
__global__ void __launch_bounds__(RS_THREADS) ransac_mask_kernel(const double* __restrict__ models, const f64x2_t* __restrict__ x0,
                                                                 const f64x2_t* __restrict__ x1, const int32_t* __restrict__ offsets,
                                                                 double thr2, uint8_t* __restrict__ mask) {
    const int b = blockIdx.y;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = models[(int64_t)b * 9 + i];
    for (int p = blockIdx.x * RS_THREADS + threadIdx.x; p < n; p += gridDim.x * RS_THREADS) {
        const f64x2_t a = x0[(int64_t)base + p], d = x1[(int64_t)base + p];
        mask[(int64_t)base + p] = sampson_inlier(m, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
}

}  // namespace

extern "C" int gim_ransac_score(const double* models, const uint8_t* valid, const double* x0, const double* x1, const int32_t* offsets,
                                int B, int K, double thr2, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_ransac_score: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K <= 0x7fffffffLL / 9, "gim_ransac_score: B*K=%lld models", (long long)B * K);
    GIM_REQUIRE(models && x0 && x1 && offsets && counts, "gim_ransac_score: NULL pointer");
    GIM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1) & 15) == 0, "gim_ransac_score: x0 and x1 must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)counts) & 3) == 0, "gim_ransac_score: misaligned models, offsets or counts");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * K * sizeof(int32_t), st) != hipSuccess) {
        gim_set_error("gim_ransac_score: hipMemsetAsync(counts)");
        return GIM_ERR_LAUNCH;
    }
    // 2 500 models are 10 tiles: the point splits are what fills 256 CUs.  The point counts live on the device, so the split count
    // comes from B and K alone (about 2 048 workgroups, at most 64 splits); a split beyond a pair's last tile leaves at once.
    const int tiles = (K + RS_THREADS - 1) / RS_THREADS;
    int64_t splits = (2048 + (int64_t)tiles * B - 1) / ((int64_t)tiles * B);
    splits = splits < 1 ? 1 : (splits > RS_MAX_SPLITS ? RS_MAX_SPLITS : splits);
    hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)tiles, (unsigned)splits, (unsigned)B), dim3(RS_THREADS), 0, st, models, valid,
                       (const f64x2_t*)x0, (const f64x2_t*)x1, offsets, K, thr2, counts);
    return gim_check_launch("ransac_score_kernel");
}

extern "C" int gim_ransac_mask(const double* models, const double* x0, const double* x1, const int32_t* offsets, int B, double thr2,
                               uint8_t* mask, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && B <= 65535, "gim_ransac_mask: B=%d (0 <= B <= 65535)", B);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(models && x0 && x1 && offsets && mask, "gim_ransac_mask: NULL pointer");
    GIM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1) & 15) == 0, "gim_ransac_mask: x0 and x1 must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models) & 7) == 0 && (((uintptr_t)offsets) & 3) == 0, "gim_ransac_mask: misaligned models or offsets");
    const int blocks = B >= 32 ? 4 : 32;                      // 8 192 points per pass of a pair; more are strided
    hipLaunchKernelGGL(ransac_mask_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(RS_THREADS), 0, (hipStream_t)stream, models,
                       (const f64x2_t*)x0, (const f64x2_t*)x1, offsets, thr2, mask);
    return gim_check_launch("ransac_mask_kernel");
}
