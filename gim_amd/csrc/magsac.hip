// MAGSAC++ scoring of RANSAC hypotheses (gfx950): for many 3x3 models per pair, the int64 quality (the sum of the quantised
// marginalised gains of magsac_loss.h over the pair's points) and the plain inlier count, in one launch.  fp64 throughout, no
// fast-math flag on this file.
//
// Replaces (reference file:line): the scoring inside cv2.findFundamentalMat(USAC_MAGSAC) / cv2.findHomography(USAC_MAGSAC) as
// called from demo.py:514-517, demo.py:197-217, video_preprocessor.py:578 and datasets/walk/walk.py:295 -- the published loss
// (Barath et al., CVPR 2020), not OpenCV's bytes.  pose.magsac_quality is the numpy restatement.
//
// The residual is the Sampson error of ransac_score.hip (kind 1) or the forward transfer error of homography_solve.h (kind 0), the
// same expressions in the same order, and the count is theirs: err <= thr2.  Only integer sums cross lanes and workgroups, so a
// quality does not depend on the launch shape, the point split, the batch or the pair's place in it.
#include "gim_common.h"
#include "magsac_loss.h"

namespace {

constexpr int MS_THREADS = 256;   // one model per lane
constexpr int MS_TP = 64;         // points staged per LDS tile: 64 x (a.x, a.y, b.x, b.y) fp64 = 2 KiB
constexpr int MS_MAX_SPLITS = 64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));

// the squared residual of a point and whether it is an inlier under thr2: sampson_inlier of ransac_score.hip
__device__ __forceinline__ double sampson_r2(const double (&m)[9], double ax, double ay, double bx, double by, double thr2, bool& in) {
    const double r0 = m[0] * ax + m[1] * ay + m[2];
    const double r1 = m[3] * ax + m[4] * ay + m[5];
    const double r2 = m[6] * ax + m[7] * ay + m[8];
    const double c0 = m[0] * bx + m[3] * by + m[6];
    const double c1 = m[1] * bx + m[4] * by + m[7];
    const double e = r0 * bx + r1 * by + r2;
    const double den = r0 * r0 + r1 * r1 + c0 * c0 + c1 * c1;
    const double err = (e * e) / (den < 1e-300 ? 1e-300 : den);
    in = err <= thr2;
    return err;
}

// ... gim_h4_inlier of homography_solve.h; w == 0: no residual (NaN: gain 0, no inlier)
__device__ __forceinline__ double transfer_r2(const double (&H)[9], double sx, double sy, double dx, double dy, double thr2, bool& in) {
    const double w = H[6] * sx + H[7] * sy + H[8];
    const double ex = dx - (H[0] * sx + H[1] * sy + H[2]) / w;
    const double ey = dy - (H[3] * sx + H[4] * sy + H[5]) / w;
    const double e = ex * ex + ey * ey;
    in = w != 0.0 && isfinite(e) && e <= thr2;
    return w != 0.0 ? e : NAN;
}

// grid = (model tiles of 256, point splits, pairs): the launch shape of ransac_score_kernel.  A lane keeps its model's nine
// coefficients in registers, the workgroup stages 64 points in LDS and every lane reads the same point (a broadcast read).  A lane
// sums its q in a 64-bit register and its count in a 32-bit one; one 64-bit and one 32-bit integer atomic per model and workgroup.
template <int KIND>
__global__ void __launch_bounds__(MS_THREADS) magsac_score_kernel(const double* __restrict__ models, const uint8_t* __restrict__ valid,
                                                                  const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                                  const int32_t* __restrict__ offsets, int K, double thr2, double scale,
                                                                  unsigned long long* __restrict__ quality, int32_t* __restrict__ counts) {
    __shared__ f64x2_t pts[2][MS_TP];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int k = blockIdx.x * MS_THREADS + tid;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform: the loop below and its barriers are too
    const int64_t mk = (int64_t)b * K + k;
    bool live = k < K && (valid == nullptr || valid[mk] != 0);
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        m[i] = live ? models[mk * 9 + i] : 0.0;
        live = live && isfinite(m[i]);                        // a model with an entry that is not finite: quality 0, count 0
    }
    if (__syncthreads_count(live) == 0) return;              // a tile of padding or of a finished pair (workgroup-uniform)
    unsigned long long q = 0;
    int cnt = 0;
    for (int c = blockIdx.y * MS_TP; c < n; c += gridDim.y * MS_TP) {
        __syncthreads();                                      // the previous tile has been read by every lane
        if (tid < 2 * MS_TP) {
            const int side = tid / MS_TP, p = tid % MS_TP;
            f64x2_t v = {0.0, 0.0};
            if (c + p < n) v = (side ? x1 : x0)[(int64_t)base + c + p];
            pts[side][p] = v;
        }
        __syncthreads();
        const int np = min(MS_TP, n - c);
        for (int p = 0; p < np; ++p) {
            const f64x2_t a = pts[0][p], d = pts[1][p];
            bool in;
            const double r2 = KIND ? sampson_r2(m, a.x, a.y, d.x, d.y, thr2, in) : transfer_r2(m, a.x, a.y, d.x, d.y, thr2, in);
            cnt += in ? 1 : 0;
            q += (unsigned long long)gim_ms_units(r2, scale);
        }
    }
    if (live && q) atomicAdd(&quality[mk], q);
    if (live && cnt) atomicAdd(&counts[mk], cnt);
}

}  // namespace

extern "C" int gim_magsac_score(int kind, const double* models, const uint8_t* valid, const double* a, const double* b,
                                const int32_t* offsets, int B, int K, double thr2, double max_thr2, int64_t* quality, int32_t* counts,
                                gim_stream_t stream) {
    GIM_REQUIRE(kind == 0 || kind == 1, "gim_magsac_score: kind=%d (0: homography, 1: fundamental matrix)", kind);
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_magsac_score: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    GIM_REQUIRE(isfinite(max_thr2) && max_thr2 > 0.0, "gim_magsac_score: max_thr2=%g must be finite and positive", max_thr2);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K <= 0x7fffffffLL / 9, "gim_magsac_score: B*K=%lld models", (long long)B * K);
    GIM_REQUIRE(models && a && b && offsets && quality && counts, "gim_magsac_score: NULL pointer");
    GIM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "gim_magsac_score: a and b must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models | (uintptr_t)quality) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)counts) & 3) == 0,
                "gim_magsac_score: misaligned models, quality, offsets or counts");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(quality, 0, (size_t)B * K * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)B * K * sizeof(int32_t), st) != hipSuccess) {
        gim_set_error("gim_magsac_score: hipMemsetAsync(quality, counts)");
        return GIM_ERR_LAUNCH;
    }
    // the split rule of gim_ransac_score: about 2 048 workgroups from B and K alone, at most 64 splits
    const int tiles = (K + MS_THREADS - 1) / MS_THREADS;
    int64_t splits = (2048 + (int64_t)tiles * B - 1) / ((int64_t)tiles * B);
    splits = splits < 1 ? 1 : (splits > MS_MAX_SPLITS ? MS_MAX_SPLITS : splits);
    const dim3 grid((unsigned)tiles, (unsigned)splits, (unsigned)B), block(MS_THREADS);
    const double scale = gim_ms_scale(max_thr2);
    if (kind) hipLaunchKernelGGL(magsac_score_kernel<1>, grid, block, 0, st, models, valid, (const f64x2_t*)a, (const f64x2_t*)b, offsets, K,
                                 thr2, scale, (unsigned long long*)quality, counts);
    else hipLaunchKernelGGL(magsac_score_kernel<0>, grid, block, 0, st, models, valid, (const f64x2_t*)a, (const f64x2_t*)b, offsets, K,
                            thr2, scale, (unsigned long long*)quality, counts);
    return gim_check_launch("magsac_score_kernel");
}
