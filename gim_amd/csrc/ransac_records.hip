// The reduction of one RANSAC step on the device (gfx950): of the step's inlier counts, only the samples that set a new strict
// maximum -- the only ones the host's bookkeeping acts on (gim_amd/pose.py, _ransac_steps) -- in sample order.  Integer arithmetic
// only; pose.step_records is the numpy restatement.
//
// Replaces the bulk read-back of a step (every model, flag and count: 250 x 10 x 9 doubles for the five-point solver) and the
// Python walk over its counts; the reference keeps this loop inside OpenCV's RANSACPointSetRegistrator::run, on the host.  The
// input is the counts output of gim_homography_step (k = 1), gim_fundamental_step (k = 3) or gim_essential_step (k = 10).
#include "gim_common.h"

namespace {

constexpr int RR_THREADS = 256, RR_WAVES = RR_THREADS / 64;

// grid = pairs: one workgroup owns one pair and walks its K samples in chunks of 256, one lane per sample, with the running maximum
// and the number of records so far carried from chunk to chunk (both workgroup-uniform).  Per chunk: the lane's c_s (the largest of
// its k slots) and j_s (the lowest slot that reaches it); an exclusive prefix maximum (wave shuffles, then one LDS word per wave);
// record = c_s above it; the records' places by a ballot per wave and one LDS word per wave.  One plain store per output word, no
// atomics: the output does not depend on the launch shape.
template <int KS>
__global__ void __launch_bounds__(RR_THREADS) ransac_records_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ nb,
                                                                    const int32_t* __restrict__ floor_, int K, int32_t* __restrict__ rec) {
    __shared__ int sMax[RR_WAVES];
    __shared__ int sCnt[RR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(nb[b], 0), K);                         // workgroup-uniform
    const int32_t* cb = counts + (int64_t)b * K * KS;
    int32_t* out = rec + (int64_t)b * (1 + 3 * (int64_t)K);
    int run = floor_[b];                                         // max(floor, c_0 .. c_{chunk start - 1})
    int n_rec = 0;
    for (int s0 = 0; s0 < n; s0 += RR_THREADS) {
        const int s = s0 + tid;
        int c = INT32_MIN, j = 0;
        if (s < n) {
            c = cb[(int64_t)s * KS];
#pragma unroll
            for (int q = 1; q < KS; ++q) {
                const int v = cb[(int64_t)s * KS + q];
                if (v > c) c = v, j = q;
            }
        }
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl = max(incl, t);
        }
        int excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = INT32_MIN;
        if (lane == 63) sMax[wave] = incl;
        __syncthreads();
        int before = run, all = run;
#pragma unroll
        for (int w = 0; w < RR_WAVES; ++w) {
            if (w < wave) before = max(before, sMax[w]);
            all = max(all, sMax[w]);
        }
        const bool is_rec = s < n && c > max(excl, before);
        const unsigned long long bal = __ballot(is_rec);
        if (lane == 0) sCnt[wave] = __popcll(bal);
        __syncthreads();
        int base = n_rec, total = n_rec;
#pragma unroll
        for (int w = 0; w < RR_WAVES; ++w) {
            if (w < wave) base += sCnt[w];
            total += sCnt[w];
        }
        if (is_rec) {
            int32_t* t = out + 1 + 3 * (int64_t)(base + __popcll(bal & ((1ull << lane) - 1ull)));
            t[0] = s, t[1] = j, t[2] = c;
        }
        run = all, n_rec = total;
    }
    if (tid == 0) out[0] = n_rec;
}

}  // namespace

extern "C" int gim_ransac_records(const int32_t* counts, const int32_t* nb, const int32_t* floor_, int B, int K, int k, int32_t* rec,
                                  gim_stream_t stream) {
    GIM_REQUIRE(k == 1 || k == 3 || k == 10, "gim_ransac_records: k=%d (1, 3 or 10)", k);
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_ransac_records: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K * k <= 0x7fffffffLL && (int64_t)B * (1 + 3 * (int64_t)K) <= 0x7fffffffLL,
                "gim_ransac_records: B*K=%lld samples", (long long)B * K);
    GIM_REQUIRE((counts || K == 0) && nb && floor_ && rec, "gim_ransac_records: NULL pointer");
    GIM_REQUIRE((((uintptr_t)counts | (uintptr_t)nb | (uintptr_t)floor_ | (uintptr_t)rec) & 3) == 0,
                "gim_ransac_records: misaligned counts, nb, floor or rec");
    const dim3 grid((unsigned)B), block(RR_THREADS);
    if (k == 1) hipLaunchKernelGGL(ransac_records_kernel<1>, grid, block, 0, (hipStream_t)stream, counts, nb, floor_, K, rec);
    else if (k == 3) hipLaunchKernelGGL(ransac_records_kernel<3>, grid, block, 0, (hipStream_t)stream, counts, nb, floor_, K, rec);
    else hipLaunchKernelGGL(ransac_records_kernel<10>, grid, block, 0, (hipStream_t)stream, counts, nb, floor_, K, rec);
    return gim_check_launch("ransac_records_kernel");
}
