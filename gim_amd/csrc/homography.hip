// Homography RANSAC step for the demo's geometry (gfx950): the four-point minimal solve AND the inlier count of every hypothesis in one
// launch, and the inlier mask of one model per pair.  fp64 throughout, no fast-math flag on this file.
//
// gim_amd/pose.py draws the samples; unlike the five- and seven-point solvers (null spaces, eigenvalues: they stay on the host) the
// four-point homography is one 8 x 8 linear solve, so a step uploads only its sample indices [B][K][4] and reads back models, flags and
// counts.  The points stay on the device, as for csrc/ransac_score.hip.
//
// Replaces (reference file:line): cv2.findHomography(mkpts1, mkpts0, ...) inside compute_geom, demo.py:180-227, i.e. the minimal solve
// (HomographyEstimatorCallback::runKernel), the sample check (::checkSubset) and the scoring (::computeError + the inlier count of
// RANSACPointSetRegistrator::run) of OpenCV's modules/calib3d/src/fundam.cpp and ptsetreg.cpp; pose.homography_4pt / pose.transfer_error
// of this project are the same arithmetic in batched numpy.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/homography_solve.h): per sample both sides are shifted to zero mean and scaled to
// mean distance sqrt(2); the 8 x 9 augmented system of dst ~ H src with h33 = 1 is reduced by Gaussian elimination with partial
// pivoting; H is de-normalised and scaled to h33 = 1.  err = |dst - proj(H src)|^2, inlier when err <= thr2; w == 0 or a projection that
// is not finite is an outlier.  The divisions are IEEE; the compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "homography_solve.h"

namespace {

constexpr int HG_THREADS = 256;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load

// grid = (hypotheses, pairs): one workgroup owns one hypothesis.  Lane 0 gathers the four correspondences, checks and solves the
// sample in LDS (72 doubles, indexed at run time by the pivoting) and leaves H there; after one barrier every lane reads H (a broadcast
// read) and counts over the pair's points, 256 per pass, coalesced 16-byte loads.  The partial counts are summed by wave shuffles and
// one LDS word per wave: integer sums, one plain store per output, no atomics and no memset.
__global__ void __launch_bounds__(HG_THREADS) homography_step_kernel(const f64x2_t* __restrict__ src, const f64x2_t* __restrict__ dst,
                                                                     const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                     int K, double thr2, double* __restrict__ models,
                                                                     uint8_t* __restrict__ valid, int32_t* __restrict__ counts) {
    __shared__ double sA[72];
    __shared__ double sH[9];
    __shared__ int sOk;
    __shared__ int sCnt[HG_THREADS / 64];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform
    const int64_t mk = (int64_t)b * K + k;
    if (tid == 0) {
        int id[4];
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            id[i] = idx[mk * 4 + i];
            ok = ok && id[i] >= 0 && id[i] < n;                // an index outside the pair never becomes an address
        }
        ok = ok && id[0] != id[1] && id[0] != id[2] && id[0] != id[3] && id[1] != id[2] && id[1] != id[3] && id[2] != id[3];
        double H[9];
        if (ok) {
            double ps[8], pd[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f64x2_t a = src[(int64_t)base + id[i]], d = dst[(int64_t)base + id[i]];
                ps[2 * i] = a.x, ps[2 * i + 1] = a.y, pd[2 * i] = d.x, pd[2 * i + 1] = d.y;
            }
            ok = gim_h4_solve(ps, pd, sA, H);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double v = ok ? H[i] : 0.0;
            sH[i] = v;
            models[mk * 9 + i] = v;
        }
        valid[mk] = ok ? 1 : 0;
        sOk = ok ? 1 : 0;
    }
    __syncthreads();
    if (!sOk) {                                               // workgroup-uniform
        if (tid == 0) counts[mk] = 0;
        return;
    }
    double H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = sH[i];
    int cnt = 0;
    for (int p = tid; p < n; p += HG_THREADS) {
        const f64x2_t a = src[(int64_t)base + p], d = dst[(int64_t)base + p];
        cnt += gim_h4_inlier(H, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((tid & 63) == 0) sCnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) counts[mk] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
}

// grid = (point blocks, pairs): one point per lane, the pair's model in registers, grid-stride over the pair's points.  Every point of
// [offsets[0], offsets[B]) is written exactly once.
__global__ void __launch_bounds__(HG_THREADS) homography_mask_kernel(const double* __restrict__ models, const f64x2_t* __restrict__ src,
                                                                     const f64x2_t* __restrict__ dst, const int32_t* __restrict__ offsets,
                                                                     double thr2, uint8_t* __restrict__ mask) {
    const int b = blockIdx.y;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;
    double H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = models[(int64_t)b * 9 + i];
    for (int p = blockIdx.x * HG_THREADS + threadIdx.x; p < n; p += gridDim.x * HG_THREADS) {
        const f64x2_t a = src[(int64_t)base + p], d = dst[(int64_t)base + p];
        mask[(int64_t)base + p] = gim_h4_inlier(H, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
}

}  // namespace

extern "C" int gim_homography_step(const double* src, const double* dst, const int32_t* offsets, int B, const int32_t* idx, int K,
                                   double thr2, double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_homography_step: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K <= 0x7fffffffLL / 9, "gim_homography_step: B*K=%lld hypotheses", (long long)B * K);
    GIM_REQUIRE(src && dst && offsets && idx && models && valid && counts, "gim_homography_step: NULL pointer");
    GIM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "gim_homography_step: src and dst must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)idx | (uintptr_t)counts) & 3) == 0,
                "gim_homography_step: misaligned models, offsets, idx or counts");
    hipLaunchKernelGGL(homography_step_kernel, dim3((unsigned)K, (unsigned)B), dim3(HG_THREADS), 0, (hipStream_t)stream,
                       (const f64x2_t*)src, (const f64x2_t*)dst, offsets, idx, K, thr2, models, valid, counts);
    return gim_check_launch("homography_step_kernel");
}

extern "C" int gim_homography_mask(const double* models, const double* src, const double* dst, const int32_t* offsets, int B, double thr2,
                                   uint8_t* mask, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && B <= 65535, "gim_homography_mask: B=%d (0 <= B <= 65535)", B);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(models && src && dst && offsets && mask, "gim_homography_mask: NULL pointer");
    GIM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "gim_homography_mask: src and dst must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models) & 7) == 0 && (((uintptr_t)offsets) & 3) == 0, "gim_homography_mask: misaligned models or offsets");
    const int blocks = B >= 32 ? 4 : 32;                      // 8 192 points per pass of a pair; more are strided
    hipLaunchKernelGGL(homography_mask_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(HG_THREADS), 0, (hipStream_t)stream, models,
                       (const f64x2_t*)src, (const f64x2_t*)dst, offsets, thr2, mask);
    return gim_check_launch("homography_mask_kernel");
}
