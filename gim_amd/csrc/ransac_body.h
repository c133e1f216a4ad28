// The shared __device__ bodies of the RANSAC kernels (ransac_score.hip, homography.hip, fundamental.hip, essential.hip), in the
// manner of igemm_persistent_body.h: the __global__ kernels keep their names, arguments, launch bounds and grids, declare their LDS
// and call these.  A step kernel is rb_gather_sample, its own minimal solve, rb_publish_model per model, then rb_count_models; a new
// minimal solver adds only the solve.  The residual and the inlier rule are two_view_residual.h's.  Device code only, except
// rb_score_grid and rb_check_launch for the entry points.
#pragma once
#include "gim_common.h"
#include "two_view_residual.h"

namespace {

constexpr int RB_THREADS = 256;      // the workgroup of every kernel here
constexpr int RB_WAVES = RB_THREADS / 64;
constexpr int RB_TP = 64;            // points staged per LDS tile of a score walk: 64 x (a.x, a.y, b.x, b.y) fp64 = 2 KiB
constexpr int RB_MAX_SPLITS = 64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load, global or LDS

// ---- the step kernels: grid = (samples, pairs), one workgroup owns one sample ------------------------------------------------------
// Lane 0: the sample's M indices idx[mk * M ..], each inside [0, n) before it becomes an address and no two alike, then its
// correspondences p0, p1 [M][2].  false: a sample the contract rejects, p0 and p1 untouched.
template <int M>
__device__ __forceinline__ bool rb_gather_sample(const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                                 const int32_t* __restrict__ idx, int64_t mk, int base, int n, double (&p0)[2 * M],
                                                 double (&p1)[2 * M]) {
    int id[M];
    bool in = true;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        id[i] = idx[mk * M + i];
        in = in && id[i] >= 0 && id[i] < n;                    // an index outside the pair never becomes an address
    }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i + 1; j < M; ++j) in = in && id[i] != id[j];
    if (!in) return false;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const f64x2_t a = x0[(int64_t)base + id[i]], d = x1[(int64_t)base + id[i]];
        p0[2 * i] = a.x, p0[2 * i + 1] = a.y, p1[2 * i] = d.x, p1[2 * i + 1] = d.y;
    }
    return true;
}

// One lane leaves one model (zeros when it is not valid) in LDS for the count walk and in the outputs.
__device__ __forceinline__ void rb_publish_model(bool ok, const double* M, double* sM, int* sOk, double* __restrict__ model,
                                                 uint8_t* __restrict__ valid) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double v = ok ? M[i] : 0.0;
        sM[i] = v;
        model[i] = v;
    }
    *valid = (uint8_t)(ok ? 1 : 0);
    *sOk = ok ? 1 : 0;
}

// After the barrier behind rb_publish_model: every lane walks the pair's points once, 256 per pass, coalesced 16-byte loads, every
// valid model of sM [NM][9] (a broadcast read from LDS; up to three models are kept in registers) against each loaded point.  The NM
// partial counts are summed by wave shuffles and one LDS word per wave and model: integer sums, one plain store per output, no
// atomics and no memset.  A sample without a valid model writes its zero counts and leaves at once (workgroup-uniform).
template <int KIND, int NM>
__device__ __forceinline__ void rb_count_models(const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1, int base, int n,
                                                const double* sM, const int* sOk, int (&sCnt)[RB_WAVES][NM], double thr2,
                                                int32_t* __restrict__ counts /* [NM] of this sample */) {
    constexpr bool IN_REGS = NM <= 3;
    const int tid = threadIdx.x;
    int okmask = 0;                                           // workgroup-uniform
#pragma unroll
    for (int j = 0; j < NM; ++j) okmask |= (sOk[j] != 0 ? 1 : 0) << j;
    if (okmask == 0) {
        if (tid < NM) counts[tid] = 0;
        return;
    }
    double reg[IN_REGS ? 9 * NM : 1];
    if (IN_REGS) {
#pragma unroll
        for (int i = 0; i < 9 * NM; ++i) reg[i] = sM[i];
    }
    const double* m = IN_REGS ? reg : sM;
    int c[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) c[j] = 0;
    for (int p = tid; p < n; p += RB_THREADS) {
        const f64x2_t a = x0[(int64_t)base + p], d = x1[(int64_t)base + p];
#pragma unroll
        for (int j = 0; j < NM; ++j)
            if ((okmask >> j) & 1) c[j] += gim_tv_inlier(KIND, m + 9 * j, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[j] += __shfl_down(c[j], o, 64);
        if ((tid & 63) == 0) sCnt[tid >> 6][j] = c[j];
    }
    __syncthreads();
    if (tid < NM) counts[tid] = sCnt[0][tid] + sCnt[1][tid] + sCnt[2][tid] + sCnt[3][tid];
}

// ---- the mask kernels: grid = (point blocks, pairs) ------------------------------------------------------------------------------------
// One point per lane, the pair's model in registers (uniform over the workgroup), grid-stride over the pair's points.  Every point
// of [offsets[0], offsets[B]) is written exactly once.
template <int KIND>
__device__ __forceinline__ void rb_mask(const double* __restrict__ models, const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                        const int32_t* __restrict__ offsets, double thr2, uint8_t* __restrict__ mask) {
    const int b = blockIdx.y;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = models[(int64_t)b * 9 + i];
    for (int p = blockIdx.x * RB_THREADS + threadIdx.x; p < n; p += gridDim.x * RB_THREADS) {
        const f64x2_t a = x0[(int64_t)base + p], d = x1[(int64_t)base + p];
        mask[(int64_t)base + p] = gim_tv_inlier(KIND, m, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
    }
}

// ---- the score kernels: grid = (model tiles of 256, point splits, pairs) ---------------------------------------------------------------
// A lane keeps its model's nine coefficients in registers; the workgroup stages 64 points in LDS and every lane reads the same point
// (a broadcast read: no bank conflict).  A workgroup walks the point tiles blockIdx.y, blockIdx.y + gridDim.y, ... of its pair, so
// the launch needs no point count on the host.  What a lane sums per point and how its partial sums reach the outputs is ACC's:
//   ACC::FINITE_MODELS  a model with an entry that is not finite is dead (no sums)
//   ACC::UNROLL         the unroll count of the walk over a staged tile
//   acc.add(err)        one point's squared residual under the lane's model
//   acc.commit(mk)      the lane's sums to model mk's outputs: integer atomics (the outputs are zeroed by the entry point: integer
//                       sums, any order, same result)
template <int KIND, class ACC>
__device__ __forceinline__ void rb_score_walk(const double* __restrict__ models, const uint8_t* __restrict__ valid,
                                              const f64x2_t* __restrict__ x0, const f64x2_t* __restrict__ x1,
                                              const int32_t* __restrict__ offsets, int K, f64x2_t (&pts)[2][RB_TP], ACC acc) {
    const int b = blockIdx.z, tid = threadIdx.x;
    const int k = blockIdx.x * RB_THREADS + tid;
    const int base = offsets[b];
    const int n = offsets[b + 1] - base;                      // workgroup-uniform: the loop below and its barriers are too
    const int64_t mk = (int64_t)b * K + k;
    bool live = k < K && (valid == nullptr || valid[mk] != 0);
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        m[i] = live ? models[mk * 9 + i] : 0.0;
        if (ACC::FINITE_MODELS) live = live && isfinite(m[i]);
    }
    if (__syncthreads_count(live) == 0) return;              // a tile of padding or of a finished pair (workgroup-uniform)
    for (int c = blockIdx.y * RB_TP; c < n; c += gridDim.y * RB_TP) {
        __syncthreads();                                      // the previous tile has been read by every lane
        if (tid < 2 * RB_TP) {
            const int side = tid / RB_TP, q = tid % RB_TP;
            f64x2_t v = {0.0, 0.0};
            if (c + q < n) v = (side ? x1 : x0)[(int64_t)base + c + q];
            pts[side][q] = v;
        }
        __syncthreads();
        const int np = min(RB_TP, n - c);
#pragma unroll ACC::UNROLL
        for (int q = 0; q < np; ++q) {
            const f64x2_t a = pts[0][q], d = pts[1][q];
            acc.add(gim_tv_error(KIND, m, a.x, a.y, d.x, d.y));
        }
    }
    if (live) acc.commit(mk);
}

// 2 500 models are 10 tiles: the point splits are what fills 256 CUs.  The point counts live on the device, so the split count
// comes from B and K alone (about 2 048 workgroups, at most 64 splits); a split beyond a pair's last tile leaves at once.
inline dim3 rb_score_grid(int B, int K) {
    const int tiles = (K + RB_THREADS - 1) / RB_THREADS;
    int64_t splits = (2048 + (int64_t)tiles * B - 1) / ((int64_t)tiles * B);
    splits = splits < 1 ? 1 : (splits > RB_MAX_SPLITS ? RB_MAX_SPLITS : splits);
    return dim3((unsigned)tiles, (unsigned)splits, (unsigned)B);
}

// The refusals every entry point makes before its launch, under the entry point's name `fn`: models * per doubles within an int
// (`noun` names what B * K counts; per == 0: no such bound), no NULL among the pointers (`ptrs`), the two point arrays `an` / `bn`
// on 16 bytes, the arrays listed in `names` on their elements (`aligned`).
inline int rb_check_launch(const char* fn, int64_t models, int per, const char* noun, bool ptrs, const void* a, const void* b,
                           const char* an, const char* bn, bool aligned, const char* names) {
    GIM_REQUIRE(per == 0 || models <= 0x7fffffffLL / per, "%s: B*K=%lld %s", fn, (long long)models, noun);
    GIM_REQUIRE(ptrs, "%s: NULL pointer", fn);
    GIM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "%s: %s and %s must be 16-byte aligned", fn, an, bn);
    GIM_REQUIRE(aligned, "%s: misaligned %s", fn, names);
    return GIM_OK;
}
inline bool rb_aligned8(const void* a, const void* b = nullptr) { return (((uintptr_t)a | (uintptr_t)b) & 7) == 0; }
inline bool rb_aligned4(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0;
}

}  // namespace
