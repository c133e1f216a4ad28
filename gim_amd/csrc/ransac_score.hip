// RANSAC hypothesis scoring for the pose half of the ZEB loop and the demo's geometry (gfx950): inlier counts of many 3x3 models
// over the matched points of one or several pairs, their MAGSAC++ qualities, and the inlier mask of one model per pair under either
// residual.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py solves 250 minimal samples (2 500 candidate essential matrices) per RANSAC step on the host and then needs, for
// every candidate, the number of points whose Sampson error is below the threshold: 2 500 x 2 000 evaluations, about 90 % of the
// host step.  gim_ransac_score is that reduction; sampling, the minimal solvers, the iteration bound and recoverPose stay on the host.
// gim_magsac_score adds, in the same walk, the int64 quality: the sum of the quantised marginalised gains of magsac_loss.h.
//
// Replaces (reference file:line): the scoring inside cv2.findEssentialMat / cv2.findFundamentalMat as called from
// tools/metrics.py:77-103 and demo.py:514-517 (EMEstimatorCallback::computeError + the inlier count of
// RANSACPointSetRegistrator::run), i.e. pose.sampson_error / pose._count_inliers of this project; the scoring inside
// cv2.findFundamentalMat(USAC_MAGSAC) / cv2.findHomography(USAC_MAGSAC) as called from demo.py:514-517, demo.py:197-217,
// video_preprocessor.py:578 and datasets/walk/walk.py:295 -- the published loss (Barath et al., CVPR 2020), not OpenCV's bytes;
// pose.magsac_quality is the numpy restatement.
//
// Arithmetic (the contract of include/gim_hip.h): the residuals and the inlier rule of two_view_residual.h.  Only integer sums cross
// lanes and workgroups, so a count or a quality does not depend on the launch shape, the point split, the batch or the pair's
// place in it.
#include "gim_common.h"
#include "magsac_loss.h"
#include "ransac_body.h"

namespace {

// what a lane of rb_score_walk sums per point (ransac_body.h)
struct count_acc {       // the inlier count: one 32-bit integer atomic per model and workgroup
    static constexpr bool FINITE_MODELS = false;   // a NaN model fails every comparison by itself
    static constexpr int UNROLL = 4;
    double thr2;
    int32_t* counts;
    int cnt = 0;
    __device__ __forceinline__ void add(double err) { cnt += gim_tv_within(GIM_TV_EPIPOLAR, err, thr2) ? 1 : 0; }
    __device__ __forceinline__ void commit(int64_t mk) {
        if (cnt) atomicAdd(&counts[mk], cnt);
    }
};

template <int KIND>
struct magsac_acc {      // the count and the quality in a 64-bit register: one 64-bit atomic beside the 32-bit one
    static constexpr bool FINITE_MODELS = true;    // a model with an entry that is not finite: quality 0, count 0
    static constexpr int UNROLL = 1;
    double thr2, scale;
    unsigned long long* quality;
    int32_t* counts;
    unsigned long long q = 0;
    int cnt = 0;
    __device__ __forceinline__ void add(double err) {
        cnt += gim_tv_within(KIND, err, thr2) ? 1 : 0;
        q += (unsigned long long)gim_ms_units(err, scale);
    }
    __device__ __forceinline__ void commit(int64_t mk) {
        if (q) atomicAdd(&quality[mk], q);
        if (cnt) atomicAdd(&counts[mk], cnt);
    }
};

__global__ void __launch_bounds__(RB_THREADS) ransac_score_kernel(const double* __restrict__ models, const uint8_t* __restrict__ valid,
                                                                  const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                  const int32_t* __restrict__ offsets, int K, double thr2,
                                                                  int32_t* __restrict__ counts) {
    __shared__ f64x2_t pts[2][RB_TP];
    rb_score_walk<GIM_TV_EPIPOLAR>(models, valid, x0, x1, offsets, K, pts, count_acc{thr2, counts});
}

template <int KIND>
__global__ void __launch_bounds__(RB_THREADS) magsac_score_kernel(const double* __restrict__ models, const uint8_t* __restrict__ valid,
                                                                  const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                  const int32_t* __restrict__ offsets, int K, double thr2, double scale,
                                                                  unsigned long long* __restrict__ quality, int32_t* __restrict__ counts) {
    __shared__ f64x2_t pts[2][RB_TP];
    rb_score_walk<KIND>(models, valid, x0, x1, offsets, K, pts, magsac_acc<KIND>{thr2, scale, quality, counts});
}

__global__ void __launch_bounds__(RB_THREADS) ransac_mask_kernel(const double* __restrict__ models, const f64x2_t* __restrict__ x0,
                                                                 const f64x2_t* __restrict__ x1, const int32_t* __restrict__ offsets,
                                                                 double thr2, uint8_t* __restrict__ mask) {
    rb_mask<GIM_TV_EPIPOLAR>(models, x0, x1, offsets, thr2, mask);
}

__global__ void __launch_bounds__(RB_THREADS) homography_mask_kernel(const double* __restrict__ models, const f64x2_t* __restrict__ src,
                                                                     const f64x2_t* __restrict__ dst, const int32_t* __restrict__ offsets,
                                                                     double thr2, uint8_t* __restrict__ mask) {
    rb_mask<GIM_TV_HOMOGRAPHY>(models, src, dst, offsets, thr2, mask);
}

}  // namespace

extern "C" int gim_ransac_score(const double* models, const uint8_t* valid, const double* x0, const double* x1, const int32_t* offsets,
                                int B, int K, double thr2, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_ransac_score: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    if (int e = rb_check_launch("gim_ransac_score", (int64_t)B * K, 9, "models", models && x0 && x1 && offsets && counts, x0, x1, "x0", "x1",
                                rb_aligned8(models) && rb_aligned4(offsets, counts), "models, offsets or counts"))
        return e;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * K * sizeof(int32_t), st) != hipSuccess) {
        gim_set_error("gim_ransac_score: hipMemsetAsync(counts)");
        return GIM_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(ransac_score_kernel, rb_score_grid(B, K), dim3(RB_THREADS), 0, st, models, valid, (const f64x2_t*)x0,
                       (const f64x2_t*)x1, offsets, K, thr2, counts);
    return gim_check_launch("ransac_score_kernel");
}

extern "C" int gim_magsac_score(int kind, const double* models, const uint8_t* valid, const double* a, const double* b,
                                const int32_t* offsets, int B, int K, double thr2, double max_thr2, int64_t* quality, int32_t* counts,
                                gim_stream_t stream) {
    GIM_REQUIRE(kind == 0 || kind == 1, "gim_magsac_score: kind=%d (0: homography, 1: fundamental matrix)", kind);
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_magsac_score: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    GIM_REQUIRE(isfinite(max_thr2) && max_thr2 > 0.0, "gim_magsac_score: max_thr2=%g must be finite and positive", max_thr2);
    if (B == 0 || K == 0) return GIM_OK;
    if (int e = rb_check_launch("gim_magsac_score", (int64_t)B * K, 9, "models", models && a && b && offsets && quality && counts, a, b, "a",
                                "b", rb_aligned8(models, quality) && rb_aligned4(offsets, counts), "models, quality, offsets or counts"))
        return e;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(quality, 0, (size_t)B * K * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)B * K * sizeof(int32_t), st) != hipSuccess) {
        gim_set_error("gim_magsac_score: hipMemsetAsync(quality, counts)");
        return GIM_ERR_LAUNCH;
    }
    const dim3 grid = rb_score_grid(B, K), block(RB_THREADS);
    const double scale = gim_ms_scale(max_thr2);
    if (kind) hipLaunchKernelGGL(magsac_score_kernel<1>, grid, block, 0, st, models, valid, (const f64x2_t*)a, (const f64x2_t*)b, offsets, K,
                                 thr2, scale, (unsigned long long*)quality, counts);
    else hipLaunchKernelGGL(magsac_score_kernel<0>, grid, block, 0, st, models, valid, (const f64x2_t*)a, (const f64x2_t*)b, offsets, K,
                            thr2, scale, (unsigned long long*)quality, counts);
    return gim_check_launch("magsac_score_kernel");
}

// the one body of the two mask entry points: `fn`, `an` and `bn` name the entry point and its point arrays in a refusal
template <class KERNEL>
static int mask_launch(const char* fn, const char* an, const char* bn, KERNEL kernel, const char* kernel_name, const double* models,
                       const double* x0, const double* x1, const int32_t* offsets, int B, double thr2, uint8_t* mask, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d (0 <= B <= 65535)", fn, B);
    if (B == 0) return GIM_OK;
    if (int e = rb_check_launch(fn, B, 0, "", models && x0 && x1 && offsets && mask, x0, x1, an, bn,
                                rb_aligned8(models) && rb_aligned4(offsets), "models or offsets"))
        return e;
    const int blocks = B >= 32 ? 4 : 32;                      // 8 192 points per pass of a pair; more are strided
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)B), dim3(RB_THREADS), 0, (hipStream_t)stream, models, (const f64x2_t*)x0,
                       (const f64x2_t*)x1, offsets, thr2, mask);
    return gim_check_launch(kernel_name);
}

extern "C" int gim_ransac_mask(const double* models, const double* x0, const double* x1, const int32_t* offsets, int B, double thr2,
                               uint8_t* mask, gim_stream_t stream) {
    return mask_launch("gim_ransac_mask", "x0", "x1", ransac_mask_kernel, "ransac_mask_kernel", models, x0, x1, offsets, B, thr2, mask, stream);
}

extern "C" int gim_homography_mask(const double* models, const double* src, const double* dst, const int32_t* offsets, int B, double thr2,
                                   uint8_t* mask, gim_stream_t stream) {
    return mask_launch("gim_homography_mask", "src", "dst", homography_mask_kernel, "homography_mask_kernel", models, src, dst, offsets, B,
                       thr2, mask, stream);
}
