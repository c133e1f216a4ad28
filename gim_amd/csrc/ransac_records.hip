// The reduction of one RANSAC step on the device (gfx950): of the step's inlier counts, only the samples that set a new strict
// maximum -- the only ones the host's bookkeeping acts on (gim_amd/pose.py, _ransac_steps) -- in sample order.  Integer arithmetic
// only; pose.step_records is the numpy restatement.  gim_ransac_records64 is the same walk keyed on an int64 quality
// (csrc/ransac_score.hip) with the counts beside it; pose.step_records64 restates it.
//
// Replaces the bulk read-back of a step (every model, flag and count: 250 x 10 x 9 doubles for the five-point solver) and the
// Python walk over its counts; the reference keeps this loop inside OpenCV's RANSACPointSetRegistrator::run, on the host.  The
// input is the counts output of gim_homography_step (k = 1), gim_fundamental_step (k = 3) or gim_essential_step (k = 10).
#include <limits>

#include "gim_common.h"

namespace {

constexpr int RR_THREADS = 256, RR_WAVES = RR_THREADS / 64;

template <typename T>
__device__ __forceinline__ T rr_max(T a, T b) { return a > b ? a : b; }

// grid = pairs: one workgroup owns one pair and walks its K samples in chunks of 256, one lane per sample, with the running maximum
// and the number of records so far carried from chunk to chunk (both workgroup-uniform).  Per chunk: the lane's c_s (the largest of
// its k slots) and j_s (the lowest slot that reaches it); an exclusive prefix maximum (wave shuffles, then one LDS word per wave);
// record = c_s above it; the records' places by a ballot per wave and one LDS word per wave.  One plain store per output word, no
// atomics: the output does not depend on the launch shape.
// Key is the type the walk maximises: int32_t, the inlier counts themselves (gim_ransac_records: Out = int32_t, triples), or int64_t,
// a quality beside the counts (gim_ransac_records64: a slot whose count is below min_count has key 0; Out = int64_t, quadruples
// (s, j_s, the count of slot j_s, Q_s)).
template <int KS, typename Key, typename Out>
__device__ __forceinline__ void records_walk(const Key* __restrict__ keys, const int32_t* __restrict__ counts, const int32_t* __restrict__ nb,
                                             const Key* __restrict__ floor_, int min_count, int K, Out* __restrict__ rec) {
    constexpr bool Q = sizeof(Key) == 8;
    constexpr int W = Q ? 4 : 3;                                 // words per record
    constexpr Key LOWEST = std::numeric_limits<Key>::lowest();
    __shared__ Key sMax[RR_WAVES];
    __shared__ int sCnt[RR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(nb[b], 0), K);                         // workgroup-uniform
    const Key* kb = keys + (int64_t)b * K * KS;
    const int32_t* cb = counts + (int64_t)b * K * KS;
    Out* out = rec + (int64_t)b * (1 + W * (int64_t)K);
    Key run = floor_[b];                                         // max(floor, c_0 .. c_{chunk start - 1})
    int n_rec = 0;
    for (int s0 = 0; s0 < n; s0 += RR_THREADS) {
        const int s = s0 + tid;
        Key c = LOWEST;
        int j = 0;
        if (s < n) {
            c = Q ? (cb[(int64_t)s * KS] >= min_count ? kb[(int64_t)s * KS] : (Key)0) : kb[(int64_t)s * KS];
#pragma unroll
            for (int q = 1; q < KS; ++q) {
                const Key v = Q ? (cb[(int64_t)s * KS + q] >= min_count ? kb[(int64_t)s * KS + q] : (Key)0) : kb[(int64_t)s * KS + q];
                if (v > c) c = v, j = q;
            }
        }
        Key incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const Key t = __shfl_up(incl, o, 64);
            if (lane >= o) incl = rr_max(incl, t);
        }
        Key excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = LOWEST;
        if (lane == 63) sMax[wave] = incl;
        __syncthreads();
        Key before = run, all = run;
#pragma unroll
        for (int w = 0; w < RR_WAVES; ++w) {
            if (w < wave) before = rr_max(before, sMax[w]);
            all = rr_max(all, sMax[w]);
        }
        const bool is_rec = s < n && c > rr_max(excl, before);
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
            Out* t = out + 1 + W * (int64_t)(base + __popcll(bal & ((1ull << lane) - 1ull)));
            t[0] = s, t[1] = j;
            if (Q) t[2] = cb[(int64_t)s * KS + j], t[3] = (Out)c;
            else t[2] = (Out)c;
        }
        run = all, n_rec = total;
    }
    if (tid == 0) out[0] = n_rec;
}

template <int KS>
__global__ void __launch_bounds__(RR_THREADS) ransac_records_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ nb,
                                                                    const int32_t* __restrict__ floor_, int K, int32_t* __restrict__ rec) {
    records_walk<KS, int32_t, int32_t>(counts, counts, nb, floor_, 0, K, rec);
}

template <int KS>
__global__ void __launch_bounds__(RR_THREADS) ransac_records64_kernel(const int64_t* __restrict__ quality, const int32_t* __restrict__ counts,
                                                                      const int32_t* __restrict__ nb, const int64_t* __restrict__ floor_q,
                                                                      int min_count, int K, int64_t* __restrict__ rec) {
    records_walk<KS, int64_t, int64_t>(quality, counts, nb, floor_q, min_count, K, rec);
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

extern "C" int gim_ransac_records64(const int64_t* quality, const int32_t* counts, const int32_t* nb, const int64_t* floor_q, int min_count,
                                    int B, int K, int k, int64_t* rec, gim_stream_t stream) {
    GIM_REQUIRE(k == 1 || k == 3 || k == 10, "gim_ransac_records64: k=%d (1, 3 or 10)", k);
    GIM_REQUIRE(B >= 0 && K >= 0 && B <= 65535, "gim_ransac_records64: B=%d K=%d (0 <= B <= 65535, K >= 0)", B, K);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)B * K * k <= 0x7fffffffLL && (int64_t)B * (1 + 4 * (int64_t)K) <= 0x7fffffffLL,
                "gim_ransac_records64: B*K=%lld samples", (long long)B * K);
    GIM_REQUIRE(((quality && counts) || K == 0) && nb && floor_q && rec, "gim_ransac_records64: NULL pointer");
    GIM_REQUIRE((((uintptr_t)quality | (uintptr_t)floor_q | (uintptr_t)rec) & 7) == 0 && (((uintptr_t)counts | (uintptr_t)nb) & 3) == 0,
                "gim_ransac_records64: misaligned quality, floor_q, rec, counts or nb");
    const dim3 grid((unsigned)B), block(RR_THREADS);
    if (k == 1) hipLaunchKernelGGL(ransac_records64_kernel<1>, grid, block, 0, (hipStream_t)stream, quality, counts, nb, floor_q, min_count, K, rec);
    else if (k == 3) hipLaunchKernelGGL(ransac_records64_kernel<3>, grid, block, 0, (hipStream_t)stream, quality, counts, nb, floor_q, min_count, K, rec);
    else hipLaunchKernelGGL(ransac_records64_kernel<10>, grid, block, 0, (hipStream_t)stream, quality, counts, nb, floor_q, min_count, K, rec);
    return gim_check_launch("ransac_records64_kernel");
}
