// Descriptor matcher of the root_sift baseline (gfx950): RootSIFT normalisation, similarity, mutual nearest neighbour and Lowe's
// ratio test in one sweep that never stores the similarity matrix.
//
// Replaces (reference file:line): trainer/lightning.py:215-226, 230 (root_sift_inference) = video_preprocessor.py:379-390:
//     desc = (desc / desc.sum(1, keepdim)).sqrt();  sim = desc0 @ desc1.T
//     mask = (sim == sim.max(1, keepdim)) & (sim == sim.max(0, keepdim));  valid, indices = mask.max(1)
//     r = (2 - 2 topk(sim, 2, dim=1)).sqrt();  valid &= r[:, 0] / r[:, 1] < 0.8;  mconf = sim.max(1)[valid]
// The reference materialises sim [n0, n1] fp32 (4.2 GB at the video labeller's 32400 keypoints per image) and reads it four more
// times.  Here a workgroup keeps 128 rows of desc0 in LDS, streams desc1 through a double-buffered LDS stage, forms 32 x 32 tiles
// of sim on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, no 16-bit operands, no split products) and
// reduces every tile in registers.  Memory beyond the inputs is O(n0 + n1).
//
//   nn_prep_kernel    rootsift = 1: sqrt(d / sum d) per row into the workspace copies; always: column maxima reset, count = 0
//   nn_sweep_kernel   pass A.  The tile is computed TRANSPOSED (MFMA A operand = desc1, B operand = desc0), so a desc0 row sits on a
//                     lane and its 16 accumulator registers are 16 columns: best / second best / lowest arg-max of a row are three
//                     registers per lane for the whole sweep, no cross-lane traffic.  The column maxima of a tile are folded over the
//                     32 lanes with a register-halving butterfly (16 cross-lane moves for 16 registers) and merged into colmax[n1]
//                     with vector integer atomic max on a monotone encoding of the float (max is order independent: the result
//                     is deterministic).  grid.y splits the column sweep when there are too few row blocks to fill the chip;
//                     every split writes its own per-row partial (best, second, arg).
//   nn_final_kernel   pass B, one thread per row: merge the splits, valid = best == colmax[arg] && sqrt(2 - 2 best) / sqrt(2 - 2 second)
//                     < ratio; match0, score0 and the count of valid rows.
//
// Differences from the reference, all on inputs the parity tests exclude or pin separately:
//   - Tie rule.  The reference's mask.max(dim=1) picks a column among those that tie the row maximum AND are mutual; this kernel
//     reports the LOWEST column index that attains the row maximum and then tests mutuality.  They differ only when one row has two
//     columns with bit-equal similarities of which one is mutual and the other is not.
//   - Not-a-number similarities (a row whose sum is 0 under rootsift: 0 / 0) are ignored by both maxima: such a row never matches and
//     is never the argument of a match.  In the reference one NaN row poisons max(dim=0) of every column and the pair has no matches.
//   - n1 == 1: there is no second best value (topk(2) raises in the reference); the ratio test rejects every row and the count is 0.
//     With the ratio test off (ratio <= 0) the result is the plain mutual nearest neighbour.  n0 == 0 or n1 == 0: nothing is
//     written except count = 0.
#include <math.h>
#include "gim_common.h"

namespace {

constexpr int NN_BM = 128;        // rows of desc0 per workgroup: 4 row groups of 32 (one MFMA tile side)
constexpr int NN_BN = 64;         // columns per sweep step: 2 column groups of 32
constexpr int NN_THREADS = 512;   // 8 waves = 4 row groups x 2 column groups: two waves per SIMD, one's tile epilogue under the other's MFMAs
constexpr int NN_PAD = 4;         // floats: row strides of 16 B x odd, so the 16 lanes of a ds_read_b128 group hit 16 distinct slots
constexpr int NN_MAX_SPLIT = 16;
constexpr int NN_ALIGN = 256;

__host__ __device__ inline int64_t nn_align(int64_t b) { return (b + NN_ALIGN - 1) / NN_ALIGN * NN_ALIGN; }

// order-preserving float -> int32 (for integer atomic max); -inf maps above INT_MIN, the reset value
__device__ __forceinline__ int nn_enc(float v) { const int e = __float_as_int(v); return e >= 0 ? e : e ^ 0x7fffffff; }
__device__ __forceinline__ float nn_dec(int e) { return __int_as_float(e >= 0 ? e : e ^ 0x7fffffff); }

struct NnRow { float best, second; int arg; };

// two partial row statistics over disjoint column sets -> the statistics of the union; the lower index wins a tie of the maxima and
// the tying value becomes the second best, as topk(2) counts it
__device__ __forceinline__ NnRow nn_merge(const NnRow a, const NnRow b) {
    const bool ta = a.best > b.best || (a.best == b.best && a.arg < b.arg);
    NnRow r;
    r.best = ta ? a.best : b.best;
    r.arg = ta ? a.arg : b.arg;
    r.second = ta ? fmaxf(a.second, b.best) : fmaxf(b.second, a.best);
    return r;
}

__global__ void __launch_bounds__(256) nn_prep_kernel(const float* __restrict__ d0, const float* __restrict__ d1, float* __restrict__ o0,
                                                      float* __restrict__ o1, int* __restrict__ colmax, int* __restrict__ count,
                                                      int n0, int n1, int D, int rootsift) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, gstep = (int64_t)gridDim.x * 256;
    for (int64_t j = gid; j < n1; j += gstep) colmax[j] = INT32_MIN;
    if (gid == 0 && count) *count = 0;
    if (!rootsift) return;
    // 16 lanes per row: a lane sums float4 pieces, the 16 partial sums meet in a xor butterfly inside the group
    const int sub = threadIdx.x & 15;
    const int64_t nrow = (int64_t)n0 + n1;
    for (int64_t r = gid >> 4; r < nrow; r += gstep >> 4) {
        const float* __restrict__ s = r < n0 ? d0 + r * D : d1 + (r - n0) * D;
        float* __restrict__ o = r < n0 ? o0 + r * D : o1 + (r - n0) * D;
        float sum = 0.f;
        for (int c = sub * 4; c < D; c += 64) {
            const float4 v = *(const float4*)(s + c);
            sum += (v.x + v.y) + (v.z + v.w);
        }
#pragma unroll
        for (int m = 8; m > 0; m >>= 1) sum += __shfl_xor(sum, m, 64);
        for (int c = sub * 4; c < D; c += 64) {
            const float4 v = *(const float4*)(s + c);
            *(float4*)(o + c) = make_float4(sqrtf(v.x / sum), sqrtf(v.y / sum), sqrtf(v.z / sum), sqrtf(v.w / sum));
        }
    }
}

// KC: k depth of one desc1 stage (32, or 16 when D is an odd multiple of 16)
template <int KC>
__global__ void __launch_bounds__(NN_THREADS) nn_sweep_kernel(const float* __restrict__ d0, const float* __restrict__ d1,
                                                               int* __restrict__ colmax, float* __restrict__ pbest,
                                                               float* __restrict__ psecond, int* __restrict__ parg,
                                                               int n0, int n1, int D, int tiles_per_split) {
    extern __shared__ float smem[];
    constexpr int LDB = KC + NN_PAD;
    const int lda = D + NN_PAD;
    float* const sA = smem;                          // [NN_BM][lda]
    float* const sB = smem + NN_BM * lda;            // [2][NN_BN][LDB]; after the sweep: the row statistics of column group 1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave & 3, cg = wave >> 2, l31 = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * NN_BM;
    const int ntile = (n1 + NN_BN - 1) / NN_BN;
    const int tile_lo = blockIdx.y * tiles_per_split;
    const int tile_hi = min(ntile, tile_lo + tiles_per_split);
    const int nkc = D / KC;
    const int nstep = (tile_hi - tile_lo) * nkc;

    // one 16-byte piece of a desc1 stage per thread: column tid / (KC / 4), piece tid % (KC / 4)
    constexpr int PPC = KC / 4;
    const bool loader = tid < NN_BN * PPC;
    const int lcol = tid / PPC, lpc = tid % PPC;
    auto load_b = [&](int step) -> float4 {
        const int col = (tile_lo + step / nkc) * NN_BN + lcol;
        if (!loader || col >= n1) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *(const float4*)(d1 + (size_t)col * D + (step % nkc) * KC + lpc * 4);
    };
    auto store_b = [&](int buf, const float4 v) {
        if (loader) *(float4*)(sB + (buf * NN_BN + lcol) * LDB + lpc * 4) = v;
    };

    float4 pre = nstep > 0 ? load_b(0) : make_float4(0.f, 0.f, 0.f, 0.f);
    // the row block of desc0 stays in LDS for the whole sweep; rows past n0 are zeros
    const int d4 = D / 4;
    for (int i = tid; i < NN_BM * d4; i += NN_THREADS) {
        const int r = i / d4, c = i - r * d4;
        const float4 v = row0 + r < n0 ? *(const float4*)(d0 + (size_t)(row0 + r) * D + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        *(float4*)(sA + r * lda + c * 4) = v;
    }
    store_b(0, pre);
    __syncthreads();

    const int row = row0 + rg * 32 + l31;            // the desc0 row of this lane
    const bool row_ok = row < n0;
    const float NINF = -INFINITY;
    NnRow st = {NINF, NINF, -1};
    f32x16_t acc = {};
    // lane (l31, h) takes k = 8 q + 4 h + c, c = 0..3, of both operands in the c-th MFMA of quad q: any k order is an exact fp32 chain
    const float* const pa = sA + (rg * 32 + l31) * lda + 4 * h;
    const float* const pb0 = sB + (cg * 32 + l31) * LDB + 4 * h;

    for (int step = 0; step < nstep; ++step) {
        const int kc = step % nkc;
        if (step + 1 < nstep) pre = load_b(step + 1);
        const float* const pb = pb0 + (step & 1) * NN_BN * LDB;
        const float* const pak = pa + kc * KC;
#pragma unroll
        for (int q = 0; q < KC / 8; ++q) {
            const float4 a = *(const float4*)(pak + 8 * q);
            const float4 b = *(const float4*)(pb + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, a.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, a.w, acc, 0, 0, 0);
        }
        if (kc == nkc - 1) {
            // acc[r] = sim[row][col0 + (r & 3) + 8 (r >> 2)], col0 = tile column + 4 h: ascending in r
            const int col0 = (tile_lo + step / nkc) * NN_BN + cg * 32 + 4 * h;
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = col0 + (r & 3) + 8 * (r >> 2);
                float x = acc[r];
                x = (j < n1 && x == x) ? x : NINF;            // columns past n1 and NaNs never win
                const bool gt = x > st.best;                  // strict: the lowest index keeps a tie
                st.second = gt ? st.best : fmaxf(st.second, x);
                st.arg = gt ? j : st.arg;
                st.best = gt ? x : st.best;
                v[r] = row_ok ? x : NINF;
            }
            // column maxima over the 32 rows of the tile: at every level a lane keeps one half of its registers and takes the
            // other lane's copy of that half, so 8 + 4 + 2 + 1 + 1 cross-lane moves reduce 16 registers over 32 lanes
#pragma unroll
            for (int half = 8; half >= 1; half >>= 1) {
                const bool up = (lane & (2 * half)) != 0;
#pragma unroll
                for (int r = 0; r < half; ++r) {
                    const float send = up ? v[r] : v[r + half];
                    const float keep = up ? v[r + half] : v[r];
                    v[r] = fmaxf(keep, __shfl_xor(send, 2 * half, 64));
                }
            }
            v[0] = fmaxf(v[0], __shfl_xor(v[0], 1, 64));
            // lane bits 4..1 are bits 3..0 of the register this lane ended up with
            const int r = (lane >> 1) & 15;
            const int j = col0 + (r & 3) + 8 * (r >> 2);
            if ((lane & 1) == 0 && j < n1) atomicMax(colmax + j, nn_enc(v[0]));
            acc = f32x16_t{};
        }
        if (step + 1 < nstep) store_b((step + 1) & 1, pre);
        __syncthreads();
    }

    // the two lane halves of a wave hold the same rows over interleaved columns; then column group 1 hands over through LDS
    {
        NnRow o;
        o.best = __shfl_xor(st.best, 32, 64);
        o.second = __shfl_xor(st.second, 32, 64);
        o.arg = __shfl_xor(st.arg, 32, 64);
        st = nn_merge(st, o);
    }
    float* const sx = sB;                            // [3][NN_BM]; every wave is past its last stage read (barrier above)
    if (cg == 1 && h == 0) {
        sx[rg * 32 + l31] = st.best;
        sx[NN_BM + rg * 32 + l31] = st.second;
        sx[2 * NN_BM + rg * 32 + l31] = __int_as_float(st.arg);
    }
    __syncthreads();
    if (cg == 0 && h == 0 && row_ok) {
        NnRow o;
        o.best = sx[rg * 32 + l31];
        o.second = sx[NN_BM + rg * 32 + l31];
        o.arg = __float_as_int(sx[2 * NN_BM + rg * 32 + l31]);
        st = nn_merge(st, o);
        const size_t p = (size_t)blockIdx.y * n0 + row;
        pbest[p] = st.best;
        psecond[p] = st.second;
        parg[p] = st.arg;
    }
}

__global__ void __launch_bounds__(256) nn_final_kernel(const int* __restrict__ colmax, const float* __restrict__ pbest,
                                                       const float* __restrict__ psecond, const int* __restrict__ parg,
                                                       int* __restrict__ match0, float* __restrict__ score0, int* __restrict__ count,
                                                       int n0, int nsplit, float ratio) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (i < n0) {
        NnRow st = {pbest[i], psecond[i], parg[i]};
        for (int s = 1; s < nsplit; ++s) {
            const size_t p = (size_t)s * n0 + i;
            st = nn_merge(st, NnRow{pbest[p], psecond[p], parg[p]});
        }
        if (st.arg >= 0) {
            valid = st.best == nn_dec(colmax[st.arg]);
            // lightning.py:224-225; a row without a second value (n1 == 1) fails the test
            if (ratio > 0.f) valid = valid && st.second > -INFINITY && sqrtf(2.f - 2.f * st.best) / sqrtf(2.f - 2.f * st.second) < ratio;
        }
        match0[i] = valid ? st.arg : -1;
        score0[i] = st.arg >= 0 ? st.best : 0.f;
    }
    const unsigned long long m = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && m && count) atomicAdd(count, __popcll(m));
}

inline int nn_smem_bytes(int D, int KC) { return (NN_BM * (D + NN_PAD) + 2 * NN_BN * (KC + NN_PAD)) * (int)sizeof(float); }

// column splits of the sweep: enough workgroups for two per CU's worth of the chip when the row blocks alone are few
inline int nn_splits(int n0, int n1) {
    const int nblk = (n0 + NN_BM - 1) / NN_BM, ntile = (n1 + NN_BN - 1) / NN_BN;
    int s = 512 / nblk;
    s = s < 1 ? 1 : (s > NN_MAX_SPLIT ? NN_MAX_SPLIT : s);
    return s > ntile ? ntile : s;
}

struct NnWs { int64_t colmax, best, second, arg, nd0, nd1, total; };
inline NnWs nn_ws(int n0, int n1, int D, int rootsift) {
    NnWs w;
    const int64_t rows = (int64_t)NN_MAX_SPLIT * n0 * 4;
    w.colmax = 0;
    w.best = w.colmax + nn_align((int64_t)n1 * 4);
    w.second = w.best + nn_align(rows);
    w.arg = w.second + nn_align(rows);
    w.nd0 = w.arg + nn_align(rows);
    w.nd1 = w.nd0 + (rootsift ? nn_align((int64_t)n0 * D * 4) : 0);
    w.total = w.nd1 + (rootsift ? nn_align((int64_t)n1 * D * 4) : 0);
    return w;
}

}  // namespace

extern "C" int64_t gim_nn_match_ws_bytes(int n0, int n1, int D, int rootsift) {
    if (n0 < 0 || n1 < 0 || D < 0) return 0;
    return nn_ws(n0, n1, D, rootsift).total;
}

extern "C" int gim_nn_match(const float* desc0, const float* desc1, int n0, int n1, int D, int rootsift, float ratio, int32_t* match0,
                            float* score0, int32_t* count, void* ws, gim_stream_t stream) {
    GIM_REQUIRE(n0 >= 0 && n1 >= 0, "gim_nn_match: n0=%d n1=%d", n0, n1);
    GIM_REQUIRE(D >= 16 && D <= 256 && D % 16 == 0, "gim_nn_match: D=%d is not a multiple of 16 in [16, 256]", D);
    GIM_REQUIRE(count, "gim_nn_match: NULL count");
    hipStream_t st = (hipStream_t)stream;
    if (n0 == 0 || n1 == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess) { gim_set_error("gim_nn_match: hipMemsetAsync(count)"); return GIM_ERR_LAUNCH; }
        return GIM_OK;
    }
    GIM_REQUIRE(desc0 && desc1 && match0 && score0 && ws, "gim_nn_match: NULL pointer");
    GIM_REQUIRE((((uintptr_t)desc0 | (uintptr_t)desc1 | (uintptr_t)ws) & 15) == 0, "gim_nn_match: desc0, desc1 and ws must be 16-byte aligned");
    const NnWs w = nn_ws(n0, n1, D, rootsift);
    char* const base = (char*)ws;
    int* const colmax = (int*)(base + w.colmax);
    float* const pbest = (float*)(base + w.best);
    float* const psecond = (float*)(base + w.second);
    int* const parg = (int*)(base + w.arg);
    float* const nd0 = (float*)(base + w.nd0);
    float* const nd1 = (float*)(base + w.nd1);

    const int KC = D % 32 == 0 ? 32 : 16;
    const int smem = nn_smem_bytes(D, KC);
    static GimPerDevice attr;
    if (attr.needed()) {
        const int top = nn_smem_bytes(256, 32);
        if (hipFuncSetAttribute((const void*)nn_sweep_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, top) != hipSuccess ||
            hipFuncSetAttribute((const void*)nn_sweep_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, top) != hipSuccess) {
            gim_set_error("gim_nn_match: hipFuncSetAttribute(%d B LDS)", top);
            return GIM_ERR_LAUNCH;
        }
        attr.done();
    }

    const int64_t prep_items = rootsift ? ((int64_t)n0 + n1) * 16 : (int64_t)n1;
    int64_t pg = (prep_items + 255) / 256;
    pg = pg < 1 ? 1 : (pg > 4096 ? 4096 : pg);
    hipLaunchKernelGGL(nn_prep_kernel, dim3((unsigned)pg), dim3(256), 0, st, desc0, desc1, nd0, nd1, colmax, count, n0, n1, D, rootsift);
    int rc = gim_check_launch("nn_prep_kernel");
    if (rc != GIM_OK) return rc;

    const float* a = rootsift ? nd0 : desc0;
    const float* b = rootsift ? nd1 : desc1;
    const int nblk = (n0 + NN_BM - 1) / NN_BM, ntile = (n1 + NN_BN - 1) / NN_BN;
    const int tps = (ntile + nn_splits(n0, n1) - 1) / nn_splits(n0, n1);
    const int nsplit = (ntile + tps - 1) / tps;          // every split owns at least one tile
    if (KC == 32)
        hipLaunchKernelGGL(nn_sweep_kernel<32>, dim3(nblk, nsplit), dim3(NN_THREADS), smem, st, a, b, colmax, pbest, psecond, parg, n0, n1, D, tps);
    else
        hipLaunchKernelGGL(nn_sweep_kernel<16>, dim3(nblk, nsplit), dim3(NN_THREADS), smem, st, a, b, colmax, pbest, psecond, parg, n0, n1, D, tps);
    rc = gim_check_launch("nn_sweep_kernel");
    if (rc != GIM_OK) return rc;

    hipLaunchKernelGGL(nn_final_kernel, dim3((n0 + 255) / 256), dim3(256), 0, st, colmax, pbest, psecond, parg, match0, score0, count, n0,
                       nsplit, ratio);
    return gim_check_launch("nn_final_kernel");
}
