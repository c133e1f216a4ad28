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
// Pair lists (gim_nn_bank_put, gim_nn_match_pairs_plan, gim_nn_match_pairs): the descriptors of many images stay resident in a bank
// desc [S][R][D] + n [S], normalised once at insertion, and P pairs of slots are matched in three launches whatever P is:
//   nn_bank_put_kernel      one image into its slot through nn_rootsift_row, the normalisation nn_prep_kernel calls (same bits), or a copy
//   nn_reset_pairs_kernel   column maxima [sum of n1] reset, count [P] = 0
//   nn_sweep_pairs_kernel   nn_sweep_tile -- the body of nn_sweep_kernel, shared -- per item of a host-built work table (pair, row block,
//                           first column tile, one past the last).  The column split comes from the row blocks of the WHOLE batch;
//                           nn_merge makes the result independent of it, so every pair gets the bits of its single-pair call.
//   nn_final_pairs_kernel   nn_final_kernel's decision over the ragged rows (pair of a row by bisection of row_off), hloc's int16 / fp16
//                           datasets in the same pass
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
#include <hip/hip_fp16.h>
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

// RootSIFT of one row by its 16 lanes (sub = lane & 15): a lane sums float4 pieces, the 16 partial sums meet in a xor butterfly inside the
// group, o = sqrt(s / sum).  The one normalisation of this file: nn_prep_kernel and nn_bank_put_kernel store the same bits.
__device__ __forceinline__ void nn_rootsift_row(const float* __restrict__ s, float* __restrict__ o, int D, int sub) {
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

__global__ void __launch_bounds__(256) nn_prep_kernel(const float* __restrict__ d0, const float* __restrict__ d1, float* __restrict__ o0,
                                                      float* __restrict__ o1, int* __restrict__ colmax, int* __restrict__ count,
                                                      int n0, int n1, int D, int rootsift) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, gstep = (int64_t)gridDim.x * 256;
    for (int64_t j = gid; j < n1; j += gstep) colmax[j] = INT32_MIN;
    if (gid == 0 && count) *count = 0;
    if (!rootsift) return;
    const int sub = threadIdx.x & 15;
    const int64_t nrow = (int64_t)n0 + n1;
    for (int64_t r = gid >> 4; r < nrow; r += gstep >> 4) {
        const float* __restrict__ s = r < n0 ? d0 + r * D : d1 + (r - n0) * D;
        float* __restrict__ o = r < n0 ? o0 + r * D : o1 + (r - n0) * D;
        nn_rootsift_row(s, o, D, sub);
    }
}

// one image into its bank slot: rootsift rows through nn_rootsift_row, else a 16-byte copy; the slot's count
__global__ void __launch_bounds__(256) nn_bank_put_kernel(const float* __restrict__ desc, float* __restrict__ slot_desc,
                                                          int* __restrict__ slot_n, int n, int D, int rootsift) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, gstep = (int64_t)gridDim.x * 256;
    if (gid == 0) *slot_n = n;
    if (rootsift) {
        const int sub = threadIdx.x & 15;
        for (int64_t r = gid >> 4; r < n; r += gstep >> 4) nn_rootsift_row(desc + r * D, slot_desc + r * D, D, sub);
    } else {
        const int64_t n4 = (int64_t)n * D / 4;
        for (int64_t i = gid; i < n4; i += gstep) ((float4*)slot_desc)[i] = ((const float4*)desc)[i];
    }
}

// One workgroup's share of the sweep: rows row0 .. row0 + 127 of d0 against the column tiles [tile_lo, tile_hi) of d1.  colmax: the
// column maxima of this d1; the row statistics go to pbest / psecond / parg [part + row].  Shared by the single-pair kernel and the
// pair-list kernel: one tile, one k order, one set of bits.
template <int KC>
__device__ __forceinline__ void nn_sweep_tile(const float* __restrict__ d0, const float* __restrict__ d1, int* __restrict__ colmax,
                                              float* __restrict__ pbest, float* __restrict__ psecond, int* __restrict__ parg,
                                              int n0, int n1, int D, int row0, int tile_lo, int tile_hi, size_t part) {
    extern __shared__ float smem[];
    constexpr int LDB = KC + NN_PAD;
    const int lda = D + NN_PAD;
    float* const sA = smem;                          // [NN_BM][lda]
    float* const sB = smem + NN_BM * lda;            // [2][NN_BN][LDB]; after the sweep: the row statistics of column group 1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave & 3, cg = wave >> 2, l31 = lane & 31, h = lane >> 5;
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
        const size_t p = part + row;
        pbest[p] = st.best;
        psecond[p] = st.second;
        parg[p] = st.arg;
    }
}

// KC: k depth of one desc1 stage (32, or 16 when D is an odd multiple of 16)
template <int KC>
__global__ void __launch_bounds__(NN_THREADS) nn_sweep_kernel(const float* __restrict__ d0, const float* __restrict__ d1,
                                                               int* __restrict__ colmax, float* __restrict__ pbest,
                                                               float* __restrict__ psecond, int* __restrict__ parg,
                                                               int n0, int n1, int D, int tiles_per_split) {
    const int ntile = (n1 + NN_BN - 1) / NN_BN;
    const int tile_lo = blockIdx.y * tiles_per_split;
    nn_sweep_tile<KC>(d0, d1, colmax, pbest, psecond, parg, n0, n1, D, blockIdx.x * NN_BM, tile_lo, min(ntile, tile_lo + tiles_per_split),
                      (size_t)blockIdx.y * n0);
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

// ---- pair list over a descriptor bank ------------------------------------------------------------------------------------------------
// tiles per split and number of splits of one pair of n1 columns under the batch's column split s (gim_nn_match's own rule: every
// split owns at least one tile); n1 == 0: no split
__host__ __device__ inline void nn_pair_split(int n1, int s, int* tps, int* ns) {
    const int ntile = (n1 + NN_BN - 1) / NN_BN;
    const int k = s < ntile ? s : ntile;
    *tps = k > 0 ? (ntile + k - 1) / k : 0;
    *ns = k > 0 ? (ntile + *tps - 1) / *tps : 0;
}

__global__ void __launch_bounds__(256) nn_reset_pairs_kernel(int* __restrict__ colmax, int* __restrict__ count, int rows1, int P) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, gstep = (int64_t)gridDim.x * 256;
    for (int64_t j = gid; j < rows1; j += gstep) colmax[j] = INT32_MIN;
    for (int64_t j = gid; j < P; j += gstep) count[j] = 0;
}

// one work item (pair, row block, first tile, one past the last tile) per workgroup.  Every entry of the tables is checked against the
// bank and the offsets before it becomes an address; an item that does not fit is skipped as a whole (all tests are block-uniform).
template <int KC>
__global__ void __launch_bounds__(NN_THREADS) nn_sweep_pairs_kernel(const float* __restrict__ bank, const int* __restrict__ bank_n,
                                                                     const int* __restrict__ idx0, const int* __restrict__ idx1,
                                                                     const int* __restrict__ row_off, const int* __restrict__ col_off,
                                                                     const int* __restrict__ work, int* __restrict__ colmax,
                                                                     float* __restrict__ pbest, float* __restrict__ psecond,
                                                                     int* __restrict__ parg, int P, int nsplit, int rows0, int rows1,
                                                                     int n_slots, int R, int D) {
    const int* const w = work + (size_t)blockIdx.x * 4;
    const int p = w[0], blk = w[1], tile_lo = w[2], tile_hi = w[3];
    if (p < 0 || p >= P) return;
    const int s0 = idx0[p], s1 = idx1[p];
    if (s0 < 0 || s0 >= n_slots || s1 < 0 || s1 >= n_slots) return;
    const int ro = row_off[p], co = col_off[p];
    const int n0 = row_off[p + 1] - ro, n1 = col_off[p + 1] - co;
    if (ro < 0 || co < 0 || n0 <= 0 || n1 <= 0 || n0 > rows0 - ro || n1 > rows1 - co) return;
    if (n0 > R || n1 > R || n0 > bank_n[s0] || n1 > bank_n[s1]) return;
    int tps, ns;
    nn_pair_split(n1, nsplit, &tps, &ns);
    const int ntile = (n1 + NN_BN - 1) / NN_BN;
    if (blk < 0 || blk > (n0 - 1) / NN_BM || tile_lo < 0 || tile_lo >= tile_hi || tile_hi > ntile) return;
    const int split = tile_lo / tps;
    if (split >= ns || split >= NN_MAX_SPLIT) return;
    nn_sweep_tile<KC>(bank + (size_t)s0 * R * D, bank + (size_t)s1 * R * D, colmax + co, pbest, psecond, parg, n0, n1, D, blk * NN_BM,
                      tile_lo, tile_hi, (size_t)split * rows0 + ro);
}

// nn_final_kernel over the ragged rows of the batch: a thread finds the pair of its row in row_off (P + 1 prefix sums), merges that
// pair's splits and decides with nn_final_kernel's expressions; hloc's int16 / fp16 datasets in the same pass when asked for
__global__ void __launch_bounds__(256) nn_final_pairs_kernel(const int* __restrict__ colmax, const float* __restrict__ pbest,
                                                             const float* __restrict__ psecond, const int* __restrict__ parg,
                                                             const int* __restrict__ row_off, const int* __restrict__ col_off,
                                                             int* __restrict__ match0, float* __restrict__ score0,
                                                             int* __restrict__ count, short* __restrict__ m16, __half* __restrict__ s16,
                                                             int P, int nsplit, int rows0, int rows1, float ratio) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    int p = -1;
    if (i < rows0) {
        int lo = 0, hi = P;                          // row_off[lo] <= i < row_off[hi]; pairs without rows repeat an offset
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (row_off[mid] <= i) lo = mid; else hi = mid;
        }
        p = lo;
        const int co = col_off[p];
        int n1 = col_off[p + 1] - co;
        if (co < 0 || n1 < 0 || n1 > rows1 - co) n1 = 0;
        int tps, ns;
        nn_pair_split(n1, nsplit, &tps, &ns);
        ns = ns > NN_MAX_SPLIT ? NN_MAX_SPLIT : ns;
        NnRow st = {-INFINITY, -INFINITY, -1};
        if (ns > 0) st = NnRow{pbest[i], psecond[i], parg[i]};
        for (int s = 1; s < ns; ++s) {
            const size_t q = (size_t)s * rows0 + i;
            st = nn_merge(st, NnRow{pbest[q], psecond[q], parg[q]});
        }
        const bool has = st.arg >= 0 && st.arg < n1;
        if (has) {
            valid = st.best == nn_dec(colmax[co + st.arg]);
            if (ratio > 0.f) valid = valid && st.second > -INFINITY && sqrtf(2.f - 2.f * st.best) / sqrtf(2.f - 2.f * st.second) < ratio;
        }
        const float sc = has ? st.best : 0.f;
        match0[i] = valid ? st.arg : -1;
        score0[i] = sc;
        if (m16) {
            m16[i] = (short)(valid ? st.arg : -1);
            s16[i] = __float2half_rn(valid ? (sc + 1.f) / 2.f : 0.f);
        }
    }
    // rows are ordered by pair: the valid lanes of a wave form one run per pair, one atomic per run
    unsigned long long m = __ballot(valid);
    const int lane = threadIdx.x & 63;
    while (m) {
        const int leader = __ffsll((long long)m) - 1;
        const int lp = __shfl(p, leader, 64);
        const unsigned long long same = __ballot(valid && p == lp);
        if (lane == leader) atomicAdd(count + lp, __popcll(same));
        m &= ~same;
    }
}

inline int nn_smem_bytes(int D, int KC) { return (NN_BM * (D + NN_PAD) + 2 * NN_BN * (KC + NN_PAD)) * (int)sizeof(float); }

// column splits of the sweep: enough workgroups for two per CU's worth of the chip when the row blocks alone are few
inline int nn_splits(int n0, int n1) {
    const int nblk = (n0 + NN_BM - 1) / NN_BM, ntile = (n1 + NN_BN - 1) / NN_BN;
    int s = 512 / nblk;
    s = s < 1 ? 1 : (s > NN_MAX_SPLIT ? NN_MAX_SPLIT : s);
    return s > ntile ? ntile : s;
}

// the sweep kernels may use the LDS of the widest descriptor
template <typename K32, typename K16>
inline bool nn_sweep_lds(GimPerDevice& attr, K32 k32, K16 k16) {
    if (!attr.needed()) return true;
    const int top = nn_smem_bytes(256, 32);
    if (hipFuncSetAttribute((const void*)k32, hipFuncAttributeMaxDynamicSharedMemorySize, top) != hipSuccess ||
        hipFuncSetAttribute((const void*)k16, hipFuncAttributeMaxDynamicSharedMemorySize, top) != hipSuccess)
        return false;
    attr.done();
    return true;
}

// column split of a pair-list batch: gim_nn_match's "about 512 workgroups", from the row blocks of ALL pairs
inline int nn_batch_splits(int64_t nblk_total) {
    const int64_t s = 512 / (nblk_total < 1 ? 1 : nblk_total);
    return s < 1 ? 1 : (s > NN_MAX_SPLIT ? NN_MAX_SPLIT : (int)s);
}

struct NnPairsWs { int64_t colmax, best, second, arg, total; };
inline NnPairsWs nn_pairs_ws(int64_t rows0, int64_t rows1) {
    NnPairsWs w;
    const int64_t rows = nn_align((int64_t)NN_MAX_SPLIT * rows0 * 4);
    w.colmax = 0;
    w.best = nn_align(rows1 * 4);
    w.second = w.best + rows;
    w.arg = w.second + rows;
    w.total = w.arg + rows;
    return w;
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
    if (!nn_sweep_lds(attr, nn_sweep_kernel<32>, nn_sweep_kernel<16>)) {
        gim_set_error("gim_nn_match: hipFuncSetAttribute(%d B LDS)", nn_smem_bytes(256, 32));
        return GIM_ERR_LAUNCH;
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

extern "C" int gim_nn_bank_put(const float* desc, int n, int D, int rootsift, int slot, float* bank_desc, int32_t* bank_n, int n_slots,
                               int max_rows, gim_stream_t stream) {
    GIM_REQUIRE(D >= 16 && D <= 256 && D % 16 == 0, "gim_nn_bank_put: D=%d is not a multiple of 16 in [16, 256]", D);
    GIM_REQUIRE(n_slots >= 1 && max_rows >= 1, "gim_nn_bank_put: n_slots=%d max_rows=%d", n_slots, max_rows);
    GIM_REQUIRE(slot >= 0 && slot < n_slots, "gim_nn_bank_put: slot %d is outside [0, %d)", slot, n_slots);
    GIM_REQUIRE(n >= 0 && n <= max_rows, "gim_nn_bank_put: n=%d descriptors do not fit a slot of max_rows=%d", n, max_rows);
    GIM_REQUIRE(bank_desc && bank_n && (desc || n == 0), "gim_nn_bank_put: NULL pointer");
    GIM_REQUIRE((((uintptr_t)desc | (uintptr_t)bank_desc) & 15) == 0, "gim_nn_bank_put: desc and bank_desc must be 16-byte aligned");
    const int64_t items = rootsift ? (int64_t)n * 16 : (int64_t)n * D / 4;
    int64_t g = (items + 255) / 256;
    g = g < 1 ? 1 : (g > 4096 ? 4096 : g);
    hipLaunchKernelGGL(nn_bank_put_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, desc,
                       bank_desc + (size_t)slot * max_rows * D, bank_n + slot, n, D, rootsift ? 1 : 0);
    return gim_check_launch("nn_bank_put_kernel");
}

extern "C" int gim_nn_match_pairs_plan(const int32_t* idx0, const int32_t* idx1, const int32_t* n, int P, int n_slots, int32_t* row_off,
                                       int32_t* col_off, int32_t* work, int work_cap, int32_t* n_work, int32_t* nsplit) {
    GIM_REQUIRE(P >= 0 && n_slots >= 1 && work_cap >= 0, "gim_nn_match_pairs_plan: P=%d n_slots=%d work_cap=%d", P, n_slots, work_cap);
    GIM_REQUIRE(row_off && col_off && n_work && nsplit && n && (P == 0 || (idx0 && idx1)), "gim_nn_match_pairs_plan: NULL pointer");
    int64_t r = 0, c = 0, nblk = 0;
    for (int p = 0; p < P; ++p) {
        GIM_REQUIRE(idx0[p] >= 0 && idx0[p] < n_slots && idx1[p] >= 0 && idx1[p] < n_slots,
                    "gim_nn_match_pairs_plan: pair %d names slot (%d, %d) outside [0, %d)", p, idx0[p], idx1[p], n_slots);
        const int n0 = n[idx0[p]], n1 = n[idx1[p]];
        GIM_REQUIRE(n0 >= 0 && n1 >= 0, "gim_nn_match_pairs_plan: negative count %d / %d in the slots of pair %d", n0, n1, p);
        r += n0;
        c += n1;
        if (n0 > 0 && n1 > 0) nblk += (n0 + NN_BM - 1) / NN_BM;
    }
    GIM_REQUIRE(r <= INT32_MAX / NN_MAX_SPLIT && c <= INT32_MAX / NN_MAX_SPLIT,
                "gim_nn_match_pairs_plan: %lld rows against %lld rows is too much for one batch", (long long)r, (long long)c);
    const int s = nn_batch_splits(nblk);
    int64_t items = 0;
    r = c = 0;
    for (int p = 0; p < P; ++p) {
        const int n0 = n[idx0[p]], n1 = n[idx1[p]];
        row_off[p] = (int32_t)r;
        col_off[p] = (int32_t)c;
        r += n0;
        c += n1;
        if (n0 == 0 || n1 == 0) continue;
        int tps, ns;
        nn_pair_split(n1, s, &tps, &ns);
        const int ntile = (n1 + NN_BN - 1) / NN_BN, blocks = (n0 + NN_BM - 1) / NN_BM;
        if (work) {
            GIM_REQUIRE(items + (int64_t)blocks * ns <= work_cap, "gim_nn_match_pairs_plan: the work table holds %d items, the batch needs more",
                        work_cap);
            for (int b = 0; b < blocks; ++b)
                for (int k = 0; k < ns; ++k) {
                    int32_t* const w = work + (items + (int64_t)b * ns + k) * 4;
                    w[0] = p;
                    w[1] = b;
                    w[2] = k * tps;
                    w[3] = (k + 1) * tps < ntile ? (k + 1) * tps : ntile;
                }
        }
        items += (int64_t)blocks * ns;
    }
    GIM_REQUIRE(items <= INT32_MAX, "gim_nn_match_pairs_plan: %lld work items", (long long)items);
    row_off[P] = (int32_t)r;
    col_off[P] = (int32_t)c;
    *n_work = (int32_t)items;
    *nsplit = s;
    return GIM_OK;
}

extern "C" int64_t gim_nn_match_pairs_ws_bytes(int rows0, int rows1) {
    if (rows0 < 0 || rows1 < 0) return 0;
    return nn_pairs_ws(rows0, rows1).total;
}

extern "C" int gim_nn_match_pairs(const float* bank_desc, const int32_t* bank_n, const int32_t* idx0, const int32_t* idx1,
                                  const int32_t* row_off, const int32_t* col_off, const int32_t* work, int P, int n_work, int nsplit,
                                  int rows0, int rows1, int n_slots, int max_rows, int D, float ratio, int32_t* match0, float* score0,
                                  int32_t* count, int hloc, int16_t* matches0_i16, void* scores_f16, void* ws, gim_stream_t stream) {
    GIM_REQUIRE(P >= 0 && n_work >= 0 && rows0 >= 0 && rows1 >= 0, "gim_nn_match_pairs: P=%d n_work=%d rows0=%d rows1=%d", P, n_work, rows0, rows1);
    GIM_REQUIRE(D >= 16 && D <= 256 && D % 16 == 0, "gim_nn_match_pairs: D=%d is not a multiple of 16 in [16, 256]", D);
    GIM_REQUIRE(n_slots >= 1 && max_rows >= 1, "gim_nn_match_pairs: n_slots=%d max_rows=%d", n_slots, max_rows);
    GIM_REQUIRE(!hloc || max_rows <= 32767, "gim_nn_match_pairs: max_rows=%d descriptors do not fit hloc's int16 matches0 (at most 32767)", max_rows);
    GIM_REQUIRE(nsplit >= 1 && nsplit <= NN_MAX_SPLIT, "gim_nn_match_pairs: nsplit=%d is outside [1, %d]", nsplit, NN_MAX_SPLIT);
    GIM_REQUIRE(rows0 <= INT32_MAX / NN_MAX_SPLIT && rows1 <= INT32_MAX / NN_MAX_SPLIT, "gim_nn_match_pairs: rows0=%d rows1=%d is too much for one batch", rows0, rows1);
    if (P == 0) return GIM_OK;
    GIM_REQUIRE(bank_desc && bank_n && idx0 && idx1 && row_off && col_off && count, "gim_nn_match_pairs: NULL pointer");
    GIM_REQUIRE(work || n_work == 0, "gim_nn_match_pairs: NULL work table of %d items", n_work);
    GIM_REQUIRE(rows0 == 0 || (match0 && score0 && ws), "gim_nn_match_pairs: NULL output or workspace");
    GIM_REQUIRE(rows0 == 0 || !hloc || (matches0_i16 && scores_f16), "gim_nn_match_pairs: hloc output asked for and not given");
    GIM_REQUIRE(n_work == 0 || (rows0 > 0 && rows1 > 0), "gim_nn_match_pairs: %d work items over rows0=%d rows1=%d", n_work, rows0, rows1);
    GIM_REQUIRE((((uintptr_t)bank_desc | (uintptr_t)ws) & 15) == 0, "gim_nn_match_pairs: bank_desc and ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const NnPairsWs w = nn_pairs_ws(rows0, rows1);
    char* const base = (char*)ws;
    int* const colmax = (int*)(base + w.colmax);
    float* const pbest = (float*)(base + w.best);
    float* const psecond = (float*)(base + w.second);
    int* const parg = (int*)(base + w.arg);

    static GimPerDevice attr;
    if (!nn_sweep_lds(attr, nn_sweep_pairs_kernel<32>, nn_sweep_pairs_kernel<16>)) {
        gim_set_error("gim_nn_match_pairs: hipFuncSetAttribute(%d B LDS)", nn_smem_bytes(256, 32));
        return GIM_ERR_LAUNCH;
    }

    const int64_t reset_items = rows1 > P ? rows1 : P;
    int64_t rg = (reset_items + 255) / 256;
    rg = rg < 1 ? 1 : (rg > 4096 ? 4096 : rg);
    hipLaunchKernelGGL(nn_reset_pairs_kernel, dim3((unsigned)rg), dim3(256), 0, st, rows0 > 0 ? colmax : nullptr, count, rows0 > 0 ? rows1 : 0, P);
    int rc = gim_check_launch("nn_reset_pairs_kernel");
    if (rc != GIM_OK || rows0 == 0) return rc;

    if (n_work > 0) {
        const int KC = D % 32 == 0 ? 32 : 16;
        const int smem = nn_smem_bytes(D, KC);
        if (KC == 32)
            hipLaunchKernelGGL(nn_sweep_pairs_kernel<32>, dim3(n_work), dim3(NN_THREADS), smem, st, bank_desc, bank_n, idx0, idx1, row_off, col_off,
                               work, colmax, pbest, psecond, parg, P, nsplit, rows0, rows1, n_slots, max_rows, D);
        else
            hipLaunchKernelGGL(nn_sweep_pairs_kernel<16>, dim3(n_work), dim3(NN_THREADS), smem, st, bank_desc, bank_n, idx0, idx1, row_off, col_off,
                               work, colmax, pbest, psecond, parg, P, nsplit, rows0, rows1, n_slots, max_rows, D);
        rc = gim_check_launch("nn_sweep_pairs_kernel");
        if (rc != GIM_OK) return rc;
    }

    hipLaunchKernelGGL(nn_final_pairs_kernel, dim3((rows0 + 255) / 256), dim3(256), 0, st, colmax, pbest, psecond, parg, row_off, col_off, match0,
                       score0, count, hloc ? (short*)matches0_i16 : nullptr, hloc ? (__half*)scores_f16 : nullptr, P, nsplit, rows0, rows1, ratio);
    return gim_check_launch("nn_final_pairs_kernel");
}
