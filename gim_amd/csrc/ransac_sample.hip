// RANSAC sampling on the device (gfx950): the sample indices of one step of every pair of a lockstep run, in one launch.  Integer
// arithmetic only; csrc/ransac_sample.h is the arithmetic (Philox4x32-10 words, Floyd's m distinct draws), pose.device_samples its
// numpy restatement.
//
// Replaces the host's per-step draw of gim_amd/pose.py (_ransac_steps: an argsort of nb x P random keys, uploaded as int32
// [B][K][m]); the reference draws inside OpenCV's RANSACPointSetRegistrator::getSubset (cv::RNG), on the host too.  A sample
// depends on (seed, its ordinal in the pair's run, P, m) alone -- not on the step size, the pair's place in the batch or the launch
// shape -- so a batch pair's samples are those of its single call.  The output feeds gim_homography_step / gim_fundamental_step /
// gim_essential_step, which treat -1 as padding.
#include "gim_common.h"
#include "ransac_sample.h"

namespace {

constexpr int RS_THREADS = 256;

// grid = (ceil(K / 256), pairs): one lane owns one sample slot s of pair b and writes its m words with plain per-lane stores (the
// whole [B][K][m] buffer is written: slots at or beyond count[b], and every slot of a pair with fewer than m points, hold -1).
template <int M>
__global__ void __launch_bounds__(RS_THREADS) ransac_sample_kernel(const int32_t* __restrict__ offsets, const int64_t* __restrict__ first,
                                                                   const int32_t* __restrict__ count, int K, uint64_t seed,
                                                                   int32_t* __restrict__ idx) {
    const int b = blockIdx.y;
    const int s = blockIdx.x * RS_THREADS + threadIdx.x;
    if (s >= K) return;
    const int32_t P = offsets[b + 1] - offsets[b];
    int32_t out[M];
    // P < M pads inside gim_rs_sample_m; an unused slot is a sample over no points
    gim_rs_sample_m<M>(seed, (uint64_t)first[b] + (uint64_t)s, s < count[b] ? P : 0, out);
    int32_t* dst = idx + ((int64_t)b * K + s) * M;
#pragma unroll
    for (int i = 0; i < M; ++i) dst[i] = out[i];
}

}  // namespace

extern "C" int gim_ransac_sample(const int32_t* offsets, int B, const int64_t* first, const int32_t* count, int K, int m, uint64_t seed,
                                 int32_t* idx, gim_stream_t stream) {
    GIM_REQUIRE(gim_rs_supported(m), "gim_ransac_sample: m=%d (4, 5 or 7)", m);
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_ransac_sample: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K * m <= 0x7fffffffLL, "gim_ransac_sample: B*K*m=%lld indices", (long long)B * K * m);
    GIM_REQUIRE(offsets && first && count && idx, "gim_ransac_sample: NULL pointer");
    GIM_REQUIRE((((uintptr_t)first) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)count | (uintptr_t)idx) & 3) == 0,
                "gim_ransac_sample: misaligned first, offsets, count or idx");
    const dim3 grid((unsigned)((K + RS_THREADS - 1) / RS_THREADS), (unsigned)B), block(RS_THREADS);
    if (m == 4) hipLaunchKernelGGL(ransac_sample_kernel<4>, grid, block, 0, (hipStream_t)stream, offsets, first, count, K, seed, idx);
    else if (m == 5) hipLaunchKernelGGL(ransac_sample_kernel<5>, grid, block, 0, (hipStream_t)stream, offsets, first, count, K, seed, idx);
    else hipLaunchKernelGGL(ransac_sample_kernel<7>, grid, block, 0, (hipStream_t)stream, offsets, first, count, K, seed, idx);
    return gim_check_launch("ransac_sample_kernel");
}
