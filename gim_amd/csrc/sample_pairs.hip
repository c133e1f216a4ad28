// RegressionMatcher.sample (dkm.py:583-620, roma.py:680-714) for a batch of pairs: gim_balanced_sample_pairs.
//
// gim_amd.dense.balanced_sample runs per pair: a host read of n_pos, two gim_weighted_sample calls (sample.hip), gim_kde (dkm.hip),
// two torch.sort, gathers and elementwise ops -- about 30 launches and one synchronisation per pair.  Here the pair is blockIdx.y,
// every per-pair quantity (n_pos, k1, k2, the radix-select state) stays in a device-side state block, and the launch sequence is the
// same 20 launches for any B <= GIM_SAMPLE_MAX_PAIRS:
//
//   memset(hist, state)
//   sp_keys_kernel       w = cert > thresh ? 1 : cert, first-draw key (ws_key, sample_common.h), 12-bit histogram, n_pos[b]
//   sp_rekey_kernel      pairs with n_pos == 0 only: keys of w + 1e-8 (every other pair's blocks return after one load)
//   draw 0 over the n keys of a pair, draw 1 over the k1[b] keys of its first-draw rows -- the same six kernels:
//     sp_pick / sp_hist / sp_pick / sp_hist / sp_pick    radix select (12 + 12 + 8 bits) of the k-th largest key, k on the device
//     sp_count_kernel    per block of 2048 consecutive keys: how many lie above the threshold key, how many tie with it
//     sp_scan_kernel     one workgroup per pair: exclusive scan of the blocks -> output offset and tie rank at every block's start
//     sp_emit_kernel     in-block scan, rows written IN ASCENDING INDEX; a tied key is taken iff its rank among the ties is < need
//   sp_kde_kernel        between the draws: density of the first-draw rows (kde_block, the per-pair kernel's summation order),
//                        p = density < 10 ? 1e-7 : 1 / (density + 1), second-draw key and histogram
//
// The ordered emit replaces the atomic compaction + tie list + torch.sort of the per-pair path: the selected SET is the same (top-k
// of the same keys, ties by ascending index), and ascending index is the order torch.sort gave it.  It holds for any number of ties;
// the per-pair path is arrival-ordered behind 4096 of them (TIE_CAP in sample.hip), so there -- and only there -- the two may differ.
// Key 0 (weight <= 0) is never taken; k1 / k2 are the numbers of rows actually written, so nothing downstream reads an unwritten row.
#include <algorithm>
#include "gim_common.h"
#include "sample_common.h"

namespace {

constexpr int SP_ITEMS = 8;                 // consecutive keys per thread in count / emit
constexpr int SP_CHUNK = 256 * SP_ITEMS;    // consecutive keys per block in count / emit

struct SpState {       // per pair, 64 bytes
    int n_pos;         // #(w > 0) as counted by sp_keys_kernel (0: the pair was re-keyed and counts as n)
    int k[2];          // rows of the first / second draw (sp_pick: asked for; sp_scan: written)
    unsigned prefix;   // radix select: bits decided so far
    int need;          // radix select: keys still to take from the current bucket
    int pad_[11];
};
static_assert(sizeof(SpState) == 64, "SpState is documented as int32 [16]");

struct SpArgs {
    const float* matches; const float* cert;
    float* sparse; float* mconf; int* count;
    unsigned* keys1; float* rows; float* rowcert; float* density; unsigned* keys2; int2* blocks1; int2* blocks2; unsigned* hist; SpState* st;
    int n, np, num, K1, nb1, nb2, half;
    float thresh, inv2s2;
    unsigned seeds[GIM_SAMPLE_MAX_PAIRS][2];
};

// keys and key count of draw D of pair b
template <int D> __device__ __forceinline__ const unsigned* sp_keys(const SpArgs& a, int b) {
    return D == 0 ? a.keys1 + (size_t)b * a.np : a.keys2 + (size_t)b * a.K1;
}
template <int D> __device__ __forceinline__ int sp_len(const SpArgs& a, int b) { return D == 0 ? a.n : a.st[b].k[0]; }
template <int D> __device__ __forceinline__ int2* sp_blocks(const SpArgs& a, int b) {
    return D == 0 ? a.blocks1 + (size_t)b * a.nb1 : a.blocks2 + (size_t)b * a.nb2;
}

// exclusive scan of v over the 256 threads of the block (thread order); *total = the sum.  sh: 4 ints of LDS.
__device__ __forceinline__ int block_excl_scan(int v, int* total, int* sh) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();                  // the previous use of sh is over
    if (lane == 63) sh[wv] = x;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += sh[w];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + x - v;
}

// histogram of one key into the block's LDS bins; key 0 is not counted: the walk of sp_pick never looks at the count of bucket 0
__device__ __forceinline__ void flush_hist(const unsigned* h, unsigned* hist, int nb) {
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

template <bool REKEY>
__global__ void __launch_bounds__(256) sp_keys_kernel(const SpArgs a) {
    const int b = blockIdx.y;
    if (REKEY && a.st[b].n_pos != 0) return;       // only a pair without a positive weight is keyed again
    __shared__ unsigned h[4096];
    __shared__ int cnt[4];
    for (int i = threadIdx.x; i < 4096; i += 256) h[i] = 0u;
    __syncthreads();
    const float* cert = a.cert + (size_t)b * a.n;
    unsigned* keys = a.keys1 + (size_t)b * a.np;
    const unsigned seed = a.seeds[b][0];
    int pos = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256) {
        const float c = cert[i];
        float w = c > a.thresh ? 1.f : c;          // dense_certainty[> thresh] = 1
        if (REKEY) w = w + 1e-8f;
        const unsigned key = ws_key(w, (unsigned)i, seed);
        keys[i] = key;
        if (key) atomicAdd(&h[key >> 20], 1u);
        pos += w > 0.f ? 1 : 0;
    }
    flush_hist(h, a.hist + (size_t)b * 4096, 4096);
    if (!REKEY) {
        int total;
        block_excl_scan(pos, &total, cnt);
        if (threadIdx.x == 0 && total) atomicAdd(&a.st[b].n_pos, total);
    }
}

// later passes: histogram of the next `bits` bits among keys whose decided high bits match the prefix
template <int D>
__global__ void __launch_bounds__(256) sp_hist_kernel(const SpArgs a, int shift, int bits, int decided_shift) {
    const int b = blockIdx.y;
    const int n = sp_len<D>(a, b);
    if (blockIdx.x * 256 >= n) return;
    __shared__ unsigned h[4096];
    const int nb = 1 << bits;
    for (int i = threadIdx.x; i < nb; i += 256) h[i] = 0u;
    __syncthreads();
    const unsigned* keys = sp_keys<D>(a, b);
    const unsigned prefix = a.st[b].prefix;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned key = keys[i];
        if (key && (key >> decided_shift) == (prefix >> decided_shift)) atomicAdd(&h[(key >> shift) & (nb - 1)], 1u);
    }
    flush_hist(h, a.hist + (size_t)b * 4096, nb);
}

// one workgroup per pair: walk the histogram from the top, find the bucket that contains the need-th largest key
template <int D>
__global__ void __launch_bounds__(256) sp_pick_kernel(const SpArgs a, int bits, int shift, int first) {
    const int b = blockIdx.x;
    __shared__ unsigned h[4096];
    unsigned* hist = a.hist + (size_t)b * 4096;
    const int nb = 1 << bits;
    for (int i = threadIdx.x; i < nb; i += 256) { h[i] = hist[i]; hist[i] = 0u; }   // leave the histogram clean for the next pass
    __syncthreads();
    if (threadIdx.x == 0) {
        SpState* st = a.st + b;
        int need;
        if (first) {
            if (D == 0) {
                const int n_pos = st->n_pos == 0 ? a.n : st->n_pos;      // the `+ 1e-8` path draws from every row
                need = min(a.K1, n_pos);                                 // k1 = min(4 * num, n, n_pos)
            } else {
                need = min(a.num, st->k[0]);                             // k2 = min(num, k1)
            }
            st->k[D] = need;
        } else {
            need = st->need;
        }
        int bk = nb - 1;
        for (; bk > 0; --bk) {
            if ((int)h[bk] >= need) break;
            need -= (int)h[bk];
        }
        st->prefix = (first ? 0u : st->prefix) | ((unsigned)bk << shift);
        st->need = need;
    }
}

// per block of SP_CHUNK consecutive keys: (keys above the threshold key, keys tied with it)
template <int D>
__global__ void __launch_bounds__(256) sp_count_kernel(const SpArgs a) {
    const int b = blockIdx.y;
    const int n = sp_len<D>(a, b);
    const int lo = blockIdx.x * SP_CHUNK;
    if (lo >= n) return;
    __shared__ int sh[4];
    const unsigned* keys = sp_keys<D>(a, b);
    const unsigned T = a.st[b].prefix;
    int above = 0, tied = 0;
    for (int e = 0; e < SP_ITEMS; ++e) {
        const int i = lo + e * 256 + threadIdx.x;
        const unsigned key = i < n ? keys[i] : 0u;
        above += key > T ? 1 : 0;
        tied += (key == T && key != 0u) ? 1 : 0;
    }
    int ta, tt;
    block_excl_scan(above, &ta, sh);
    block_excl_scan(tied, &tt, sh);
    if (threadIdx.x == 0) sp_blocks<D>(a, b)[blockIdx.x] = make_int2(ta, tt);
}

// one workgroup per pair: (above, tied) of every block -> (rows written before the block, ties seen before the block); k[D] = rows written
template <int D>
__global__ void __launch_bounds__(256) sp_scan_kernel(const SpArgs a) {
    const int b = blockIdx.x;
    const int n = sp_len<D>(a, b);
    const int nblk = (n + SP_CHUNK - 1) / SP_CHUNK;
    __shared__ int sh[4];
    int2* blk = sp_blocks<D>(a, b);
    const int need = a.st[b].need;
    int out_run = 0, tie_run = 0;
    for (int j0 = 0; j0 < nblk; j0 += 256) {
        const int j = j0 + threadIdx.x;
        const int2 c = j < nblk ? blk[j] : make_int2(0, 0);
        int tt, ts;
        const int tie_off = tie_run + block_excl_scan(c.y, &tt, sh);
        const int sel = c.x + min(max(need - tie_off, 0), c.y);
        const int out_off = out_run + block_excl_scan(sel, &ts, sh);
        if (j < nblk) blk[j] = make_int2(out_off, tie_off);
        out_run += ts;
        tie_run += tt;
    }
    if (threadIdx.x == 0) a.st[b].k[D] = min(out_run, D == 0 ? a.K1 : a.num);
}

// the selected keys of a block, written in ascending index.  D == 0: rows / rowcert from the maps; D == 1: sparse / mconf from the
// first-draw rows, zeros behind the k2 rows of the pair, count[b]
template <int D>
__global__ void __launch_bounds__(256) sp_emit_kernel(const SpArgs a) {
    const int b = blockIdx.y;
    const int n = sp_len<D>(a, b);
    const int cap = D == 0 ? a.K1 : a.num;
    if (D == 1) {
        const int k2 = a.st[b].k[1];
        float4* sp = (float4*)a.sparse + (size_t)b * a.num;
        float* mc = a.mconf + (size_t)b * a.num;
        for (int r = k2 + blockIdx.x * 256 + threadIdx.x; r < a.num; r += gridDim.x * 256) {
            sp[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            mc[r] = 0.f;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) a.count[b] = k2;
    }
    const int lo = blockIdx.x * SP_CHUNK;
    if (lo >= n) return;
    __shared__ int sh[4];
    const unsigned* keys = sp_keys<D>(a, b);
    const unsigned T = a.st[b].prefix;
    const int need = a.st[b].need;
    const int2 off = sp_blocks<D>(a, b)[blockIdx.x];
    const int i0 = lo + threadIdx.x * SP_ITEMS;       // this thread's SP_ITEMS consecutive keys
    unsigned key[SP_ITEMS];
    int tied = 0;
#pragma unroll
    for (int e = 0; e < SP_ITEMS; ++e) {
        key[e] = i0 + e < n ? keys[i0 + e] : 0u;
        tied += (key[e] == T && key[e] != 0u) ? 1 : 0;
    }
    int total;
    int tie_rank = off.y + block_excl_scan(tied, &total, sh);
    unsigned take = 0u;
    int sel = 0;
#pragma unroll
    for (int e = 0; e < SP_ITEMS; ++e) {
        bool t = key[e] > T;
        if (key[e] == T && key[e] != 0u) t = tie_rank++ < need;
        take |= (t ? 1u : 0u) << e;
        sel += t ? 1 : 0;
    }
    int pos = off.x + block_excl_scan(sel, &total, sh);
    const float4* src = D == 0 ? (const float4*)a.matches + (size_t)b * a.n : (const float4*)a.rows + (size_t)b * a.K1;
    const float* srcc = D == 0 ? a.cert + (size_t)b * a.n : a.rowcert + (size_t)b * a.K1;
    float4* dst = D == 0 ? (float4*)a.rows + (size_t)b * a.K1 : (float4*)a.sparse + (size_t)b * a.num;
    float* dstc = D == 0 ? a.rowcert + (size_t)b * a.K1 : a.mconf + (size_t)b * a.num;
#pragma unroll
    for (int e = 0; e < SP_ITEMS; ++e) {
        if ((take >> e) & 1u) {
            if (pos < cap) {
                dst[pos] = src[i0 + e];
                dstc[pos] = srcc[i0 + e];     // the un-thresholded certainty
            }
            ++pos;
        }
    }
}

// density of the first-draw rows, then the second draw's keys: p = density < 10 ? 1e-7 : 1 / (density + 1), hashed by the row's rank
__global__ void __launch_bounds__(256) sp_kde_kernel(const SpArgs a) {
    const int b = blockIdx.y;
    const int n = a.st[b].k[0];
    if (blockIdx.x * 64 >= n) return;
    __shared__ float4 tile[4][64];
    __shared__ float part[4][64];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const float d = kde_block(a.rows + (size_t)b * a.K1 * 4, n, a.inv2s2, a.half, blockIdx.x, tile, part);
    if ((threadIdx.x >> 6) == 0 && i < n) {
        a.density[(size_t)b * a.K1 + i] = d;
        const float p = d < 10.f ? 1e-7f : 1.f / (d + 1.f);
        const unsigned key = ws_key(p, (unsigned)i, a.seeds[b][1]);
        a.keys2[(size_t)b * a.K1 + i] = key;
        if (key) atomicAdd(&a.hist[(size_t)b * 4096 + (key >> 20)], 1u);
    }
}

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

struct SpLayout {
    int np, K1, nb1, nb2;
    int64_t keys1, rows, rowcert, density, keys2, blocks1, blocks2, hist, st, end;
    SpLayout(int B, int n, int num) {
        np = (int)(((int64_t)n + 3) / 4 * 4);
        K1 = (int)std::min<int64_t>((int64_t)4 * num, n);
        nb1 = (n + SP_CHUNK - 1) / SP_CHUNK;
        nb2 = (K1 + SP_CHUNK - 1) / SP_CHUNK;
        keys1 = 0;
        rows = keys1 + up256((int64_t)B * np * 4);
        rowcert = rows + up256((int64_t)B * K1 * 16);
        density = rowcert + up256((int64_t)B * K1 * 4);
        keys2 = density + up256((int64_t)B * K1 * 4);
        blocks1 = keys2 + up256((int64_t)B * K1 * 4);
        blocks2 = blocks1 + up256((int64_t)B * nb1 * 8);
        hist = blocks2 + up256((int64_t)B * nb2 * 8);
        st = hist + up256((int64_t)B * 4096 * 4);
        end = st + up256((int64_t)B * sizeof(SpState));
    }
};

template <int D>
void sp_draw(const SpArgs& a, int B, int len, hipStream_t s) {
    const dim3 grid((unsigned)(len < 256 * 1024 ? (len + 255) / 256 : 1024), (unsigned)B);
    const dim3 chunks((unsigned)((len + SP_CHUNK - 1) / SP_CHUNK), (unsigned)B);
    hipLaunchKernelGGL(sp_pick_kernel<D>, dim3(B), dim3(256), 0, s, a, 12, 20, 1);
    hipLaunchKernelGGL(sp_hist_kernel<D>, grid, dim3(256), 0, s, a, 8, 12, 20);
    hipLaunchKernelGGL(sp_pick_kernel<D>, dim3(B), dim3(256), 0, s, a, 12, 8, 0);
    hipLaunchKernelGGL(sp_hist_kernel<D>, grid, dim3(256), 0, s, a, 0, 8, 8);
    hipLaunchKernelGGL(sp_pick_kernel<D>, dim3(B), dim3(256), 0, s, a, 8, 0, 0);
    hipLaunchKernelGGL(sp_count_kernel<D>, chunks, dim3(256), 0, s, a);
    hipLaunchKernelGGL(sp_scan_kernel<D>, dim3(B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sp_emit_kernel<D>, chunks, dim3(256), 0, s, a);
}

}  // namespace

extern "C" int64_t gim_balanced_sample_pairs_ws_bytes(int B, int n, int num) {
    if (B < 1 || n < 1 || num < 1) return 0;
    return SpLayout(B, n, num).end;
}

extern "C" int gim_balanced_sample_pairs(const float* matches, const float* certainty, const uint32_t* seeds, float* sparse, float* mconf,
                                         int32_t* count, void* ws, int B, int n, int num, float thresh, int kde_half, gim_stream_t stream) {
    GIM_REQUIRE(B >= 1 && B <= GIM_SAMPLE_MAX_PAIRS && n > 0 && num > 0, "balanced_sample_pairs: B=%d (1..%d) n=%d num=%d", B,
                GIM_SAMPLE_MAX_PAIRS, n, num);
    GIM_REQUIRE(matches && certainty && seeds && sparse && mconf && count && ws, "balanced_sample_pairs: NULL pointer");
    GIM_REQUIRE(((uintptr_t)matches & 15) == 0 && ((uintptr_t)sparse & 15) == 0 && ((uintptr_t)ws & 255) == 0,
                "balanced_sample_pairs: matches / sparse must be 16-byte, the workspace 256-byte aligned");
    GIM_REQUIRE(n <= 0x40000000 && num <= 0x7fffffff / 4 / GIM_SAMPLE_MAX_PAIRS, "balanced_sample_pairs: n=%d num=%d", n, num);
    hipStream_t s = (hipStream_t)stream;
    const SpLayout L(B, n, num);
    char* base = (char*)ws;
    SpArgs a;
    a.matches = matches; a.cert = certainty; a.sparse = sparse; a.mconf = mconf; a.count = count;
    a.keys1 = (unsigned*)(base + L.keys1); a.rows = (float*)(base + L.rows); a.rowcert = (float*)(base + L.rowcert);
    a.density = (float*)(base + L.density); a.keys2 = (unsigned*)(base + L.keys2); a.blocks1 = (int2*)(base + L.blocks1);
    a.blocks2 = (int2*)(base + L.blocks2); a.hist = (unsigned*)(base + L.hist); a.st = (SpState*)(base + L.st);
    a.n = n; a.np = L.np; a.num = num; a.K1 = L.K1; a.nb1 = L.nb1; a.nb2 = L.nb2; a.half = kde_half ? 1 : 0;
    a.thresh = thresh;
    const float std_ = 0.1f;                      // the KDE bandwidth of sample() (dkm.py:611, roma.py:706), as gim_kde computes it
    a.inv2s2 = 1.0f / (2.0f * std_ * std_);
    for (int b = 0; b < GIM_SAMPLE_MAX_PAIRS; ++b) {
        a.seeds[b][0] = b < B ? seeds[2 * b] : 0u;
        a.seeds[b][1] = b < B ? seeds[2 * b + 1] : 0u;
    }
    if (hipMemsetAsync(base + L.hist, 0, (size_t)(L.end - L.hist), s) != hipSuccess) return gim_check_launch("balanced_sample_pairs memset");
    const dim3 grid((unsigned)(n < 256 * 1024 ? (n + 255) / 256 : 1024), (unsigned)B);
    hipLaunchKernelGGL(sp_keys_kernel<false>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(sp_keys_kernel<true>, grid, dim3(256), 0, s, a);
    sp_draw<0>(a, B, n, s);
    hipLaunchKernelGGL(sp_kde_kernel, dim3((unsigned)((L.K1 + 63) / 64), (unsigned)B), dim3(256), 0, s, a);
    sp_draw<1>(a, B, L.K1, s);
    return gim_check_launch("balanced_sample_pairs");
}
