// Dense SfM bookkeeping on the device (gfx950): the dense matches of a pair list are aggregated into one keypoint set per image and
// turned into keypoint-indexed one-to-one matches, next to the matches `sample()` left on the device.  IEEE arithmetic, no fast-math
// flag on this file; the divisions are real divisions.
//
// Replaces (reference file:line): hloc/match_dense.py:43-85 (to_cpts, assign_keypoints), :88-130 (kpids_to_matches0), :298-390
// (aggregate_matches) and :393-419 (assign_matches) for the SfM branch (every image binned, conf max_error / cell_size), i.e.
// gim_amd/hloc_formats.py's ImageKeypoints / nearest_ids / matches0_from_ids of this project, which stay the host oracle.
//
// Geometry (the contract of include/gim_hip.h): patch = max(cell_size, max_error), vote = int(max_error), r = patch / vote,
// h = (r + 1) / 2, nb = 2 h + 1 bins per axis and cell (r + 1 for an even r).  A point x of an image W x H has, per axis and in fp32,
//     c = rint((x + 0.5) / patch)  in [0, W / patch + 1],      b = rint((x + 0.5) / vote),      b - r c + h in [0, nb)
// and votes with llrint(score * 2^32) for bin b of cell c.  Only integer sums cross threads (as in ransac_score.hip): what an image's
// keypoints are does not depend on the launch shape or on the order in which its pairs arrive.
#include "gim_common.h"

namespace {

constexpr int AG_THREADS = 256;
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

struct AggConf {
    float fpatch, fvote, max_error;
    int patch, vote, r, h, nb;
};

struct AggGeom {
    int W, H, Gw, Gh;
    int64_t cell0;
    bool ok;
};

// slot -> its image size and its piece of the flat cell arrays; ok == false: the slot, its size or its piece does not fit, and
// nothing of it is used as an address
__device__ __forceinline__ AggGeom agg_geom(const int32_t* __restrict__ geom, int slot, int n_slots, int patch, int64_t total_cells) {
    AggGeom g = {0, 0, 0, 0, 0, false};
    if (slot < 0 || slot >= n_slots) return g;
    g.W = geom[4 * slot];
    g.H = geom[4 * slot + 1];
    g.cell0 = geom[4 * slot + 2];
    if (g.W < 1 || g.H < 1 || g.cell0 < 0) return g;
    g.Gw = g.W / patch + 2;
    g.Gh = g.H / patch + 2;
    g.ok = g.cell0 + (int64_t)g.Gw * g.Gh <= total_cells;
    return g;
}

// cell (cx, cy) and bin of a point; false: the point is outside [-0.5, W - 0.5] x [-0.5, H - 0.5] (a NaN coordinate is) or, which the
// arithmetic excludes, its cell or bin is outside the grid
__device__ __forceinline__ bool agg_quantize(f32x2_t x, const AggGeom& g, const AggConf& c, int& cx, int& cy, int& bin) {
    if (!(x.x >= -0.5f && x.x <= (float)g.W - 0.5f && x.y >= -0.5f && x.y <= (float)g.H - 0.5f)) return false;
    const float tx = x.x + 0.5f, ty = x.y + 0.5f;
    cx = (int)rintf(tx / c.fpatch);
    cy = (int)rintf(ty / c.fpatch);
    const int bx = (int)rintf(tx / c.fvote) - c.r * cx + c.h;
    const int by = (int)rintf(ty / c.fvote) - c.r * cy + c.h;
    bin = by * c.nb + bx;
    return cx >= 0 && cx < g.Gw && cy >= 0 && cy < g.Gh && bx >= 0 && bx < c.nb && by >= 0 && by < c.nb;
}

// the pair that owns pool row `row`: the largest p of [0, P) with offsets[p] <= row (offsets rise), checked by the caller
__device__ __forceinline__ int agg_find_pair(const int32_t* __restrict__ offsets, int P, int row) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// what makes a match count: both slots usable, a finite score in [0, 65536), both points inside their images
struct AggMatch {
    AggGeom g0, g1;
    int cx0, cy0, bin0, cx1, cy1, bin1;
    float score;
    bool ok;
};
__device__ __forceinline__ AggMatch agg_match(const f32x2_t* __restrict__ kpts0, const f32x2_t* __restrict__ kpts1,
                                              const float* __restrict__ scores, const int32_t* __restrict__ geom, int s0, int s1, int row,
                                              int n_slots, int64_t total_cells, const AggConf& c) {
    AggMatch m;
    m.g0 = agg_geom(geom, s0, n_slots, c.patch, total_cells);
    m.g1 = agg_geom(geom, s1, n_slots, c.patch, total_cells);
    m.score = scores[row];
    m.ok = m.g0.ok && m.g1.ok && m.score >= 0.0f && m.score < 65536.0f;      // a NaN score fails both comparisons
    m.ok = m.ok && agg_quantize(kpts0[row], m.g0, c, m.cx0, m.cy0, m.bin0);
    m.ok = m.ok && agg_quantize(kpts1[row], m.g1, c, m.cx1, m.cy1, m.bin1);
    return m;
}

// one lane per stored match of rows [row_lo, row_hi): two 64-bit integer adds and two vote counts
__global__ void __launch_bounds__(AG_THREADS) agg_vote_kernel(const f32x2_t* __restrict__ kpts0, const f32x2_t* __restrict__ kpts1,
                                                              const float* __restrict__ scores, const int32_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ slot0, const int32_t* __restrict__ slot1,
                                                              const int32_t* __restrict__ geom, u64* __restrict__ votes,
                                                              int32_t* __restrict__ cell_n, int32_t* __restrict__ dropped, int P, int row_lo,
                                                              int row_hi, int n_slots, int64_t total_cells, AggConf c) {
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x + row_lo;
    if (i >= row_hi) return;
    const int row = (int)i;
    const int p = agg_find_pair(offsets, P, row);
    if (!(offsets[p] <= row && row < offsets[p + 1])) return;
    const AggMatch m = agg_match(kpts0, kpts1, scores, geom, slot0[p], slot1[p], row, n_slots, total_cells, c);
    if (!m.ok) {
        atomicAdd(&dropped[p], 1);
        return;
    }
    const u64 fix = (u64)llrint((double)m.score * 4294967296.0);            // exact: an fp32 below 2^16 times 2^32
    const int64_t c0 = m.g0.cell0 + (int64_t)m.cy0 * m.g0.Gw + m.cx0, c1 = m.g1.cell0 + (int64_t)m.cy1 * m.g1.Gw + m.cx1;
    const int nb2 = c.nb * c.nb;
    atomicAdd(&votes[c0 * nb2 + m.bin0], fix);
    atomicAdd(&cell_n[c0], 1);
    atomicAdd(&votes[c1 * nb2 + m.bin1], fix);
    atomicAdd(&cell_n[c1], 1);
}

// one lane per cell: the bin with the largest sum (the lowest bin index wins an exact tie), and the key the host sorts by
__global__ void __launch_bounds__(AG_THREADS) agg_finalize_kernel(const u64* __restrict__ votes, const int32_t* __restrict__ cell_n,
                                                                  int64_t total_cells, int nb2, int64_t* __restrict__ cell_key,
                                                                  int32_t* __restrict__ cell_bin) {
    const int64_t cell = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (cell >= total_cells) return;
    int64_t key = 0;
    int bin = -1;
    if (cell_n[cell] > 0) {
        u64 best = votes[cell * nb2];
        bin = 0;
        for (int k = 1; k < nb2; ++k) {
            const u64 v = votes[cell * nb2 + k];
            if (v > best) { best = v; bin = k; }
        }
        const u64 cap = 0x7ffffffffffffffeull;
        key = (int64_t)((best < cap ? best : cap) + 1);                    // > 0: a voted cell whose sum is 0 is still a cell
    }
    cell_key[cell] = key;
    cell_bin[cell] = bin;
}

// one lane per selected cell: its id in id_grid, its keypoint b * vote - 0.5, its score and its cell
__global__ void __launch_bounds__(AG_THREADS) agg_keypoints_kernel(const u64* __restrict__ votes, const int32_t* __restrict__ cell_bin,
                                                                   const int32_t* __restrict__ geom, const int32_t* __restrict__ sel,
                                                                   const int32_t* __restrict__ sel_slot, const int32_t* __restrict__ kp_off,
                                                                   int n_sel, int n_slots, int64_t total_cells, AggConf c,
                                                                   int32_t* __restrict__ id_grid, f32x2_t* __restrict__ keypoints,
                                                                   double* __restrict__ score, int32_t* __restrict__ cells) {
    const int i = blockIdx.x * AG_THREADS + threadIdx.x;
    if (i >= n_sel) return;
    float kx = 0.0f, ky = 0.0f;
    double sc = 0.0;
    int cx = -1, cy = -1;
    const int slot = sel_slot[i];
    const AggGeom g = agg_geom(geom, slot, n_slots, c.patch, total_cells);
    if (g.ok) {
        const int64_t local = (int64_t)sel[i] - g.cell0;
        const int id = i - kp_off[slot];
        if (local >= 0 && local < (int64_t)g.Gw * g.Gh && id >= 0 && i < kp_off[slot + 1]) {
            const int bin = cell_bin[sel[i]];
            if (bin >= 0 && bin < c.nb * c.nb) {
                cx = (int)(local % g.Gw);
                cy = (int)(local / g.Gw);
                kx = (float)((c.r * cx + bin % c.nb - c.h) * c.vote) - 0.5f;
                ky = (float)((c.r * cy + bin / c.nb - c.h) * c.vote) - 0.5f;
                sc = (double)votes[(int64_t)sel[i] * (c.nb * c.nb) + bin] * (1.0 / 4294967296.0);
                id_grid[sel[i]] = id;
            }
        }
    }
    const f32x2_t kp = {kx, ky};
    keypoints[i] = kp;
    score[i] = sc;
    cells[2 * i] = cx;
    cells[2 * i + 1] = cy;
}

// the keypoint id of one point: its own cell's (nearest == 0), or the nearest final keypoint within max_error among the 3 x 3 cells
// around its own -- fp64 distance with a correctly rounded sqrt, the lowest id wins a tie
__device__ __forceinline__ int agg_point_id(f32x2_t x, const AggGeom& g, int cx, int cy, int slot, const int32_t* __restrict__ id_grid,
                                            const f32x2_t* __restrict__ keypoints, const int32_t* __restrict__ kp_off, int n_kp, int nearest,
                                            double max_error) {
    const int k0 = kp_off[slot], K = kp_off[slot + 1] - k0;
    if (k0 < 0 || K <= 0 || (int64_t)k0 + K > n_kp) return -1;
    if (!nearest) {
        const int id = id_grid[g.cell0 + (int64_t)cy * g.Gw + cx];
        return id >= 0 && id < K ? id : -1;
    }
    int best_id = -1;
    double best = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
            const int ex = cx + dx, ey = cy + dy;
            if (ex < 0 || ex >= g.Gw || ey < 0 || ey >= g.Gh) continue;
            const int id = id_grid[g.cell0 + (int64_t)ey * g.Gw + ex];
            if (id < 0 || id >= K) continue;
            const f32x2_t kp = keypoints[k0 + id];
            const double ux = (double)x.x - (double)kp.x, uy = (double)x.y - (double)kp.y;
            const double d = sqrt(ux * ux + uy * uy);
            if (d <= max_error && (best_id < 0 || d < best || (d == best && id < best_id))) {
                best = d;
                best_id = id;
            }
        }
    }
    return best_id;
}

__device__ __forceinline__ u64 agg_pack(float score, int m) { return ((u64)__float_as_uint(score) << 32) | (u64)(~(unsigned)m); }

// pass 1, one lane per stored match: both ids, and the match's (score, lowest index first) key maximised per id on both sides
__global__ void __launch_bounds__(AG_THREADS) agg_ids_kernel(const f32x2_t* __restrict__ kpts0, const f32x2_t* __restrict__ kpts1,
                                                             const float* __restrict__ scores, const int32_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ slot0, const int32_t* __restrict__ slot1,
                                                             const int32_t* __restrict__ geom, const int32_t* __restrict__ id_grid,
                                                             const f32x2_t* __restrict__ keypoints, const int32_t* __restrict__ kp_off,
                                                             const int32_t* __restrict__ koff0, const int32_t* __restrict__ koff1, int P,
                                                             int row_lo, int row_hi, int n_slots, int64_t total_cells, int n_kp, int rows0,
                                                             int rows1, int nearest, AggConf c, int32_t* __restrict__ ids,
                                                             u64* __restrict__ best0, u64* __restrict__ best1) {
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x + row_lo;
    if (i >= row_hi) return;
    const int row = (int)i, n = row_hi - row_lo;
    int id0 = -1, id1 = -1;
    const int p = agg_find_pair(offsets, P, row);
    if (offsets[p] <= row && row < offsets[p + 1]) {
        const int s0 = slot0[p], s1 = slot1[p];
        const AggMatch m = agg_match(kpts0, kpts1, scores, geom, s0, s1, row, n_slots, total_cells, c);
        if (m.ok) {
            id0 = agg_point_id(kpts0[row], m.g0, m.cx0, m.cy0, s0, id_grid, keypoints, kp_off, n_kp, nearest, (double)c.max_error);
            id1 = agg_point_id(kpts1[row], m.g1, m.cx1, m.cy1, s1, id_grid, keypoints, kp_off, n_kp, nearest, (double)c.max_error);
            // the pair's scratch rows must hold the ids: koff0 / koff1 are the prefix sums of the keypoint counts of the pairs' sides
            const int a0 = koff0[p], a1 = koff1[p];
            const bool fits = a0 >= 0 && a1 >= 0 && koff0[p + 1] <= rows0 && koff1[p + 1] <= rows1 && id0 < koff0[p + 1] - a0 &&
                              id1 < koff1[p + 1] - a1;
            if (!fits) id0 = id1 = -1;
            if (id0 >= 0 && id1 >= 0) {
                const u64 key = agg_pack(m.score, row - offsets[p]);
                atomicMax(&best0[a0 + id0], key);
                atomicMax(&best1[a1 + id1], key);
            }
        }
    }
    ids[row - row_lo] = id0;
    ids[n + row - row_lo] = id1;
}

__device__ __forceinline__ int agg_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// pass 2: a match stays iff it holds the maximum of its id on both sides; it writes its row entry and the pair's row length.  The row
// length is one word per pair: a wave's survivors (nearly always of one pair: 64 consecutive rows) fold their id0 + 1 first and send one
// atomicMax, not one each to the same address.  No lane leaves before the fold.
__global__ void __launch_bounds__(AG_THREADS) agg_emit_kernel(const float* __restrict__ scores, const int32_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ koff0, const int32_t* __restrict__ koff1, int P,
                                                              int row_lo, int row_hi, const int32_t* __restrict__ ids,
                                                              const u64* __restrict__ best0, const u64* __restrict__ best1,
                                                              int32_t* __restrict__ matches0, unsigned short* __restrict__ scores_f16,
                                                              int32_t* __restrict__ row_len) {
    const int64_t i = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x + row_lo;
    int p = -1, len = 0;                                                    // len > 0: this lane's match stays, in pair p
    if (i < row_hi) {
        const int row = (int)i, n = row_hi - row_lo;
        const int id0 = ids[row - row_lo], id1 = ids[n + row - row_lo];
        if (id0 >= 0 && id1 >= 0) {                                         // pass 1 checked the pair and the rows of every id >= 0
            p = agg_find_pair(offsets, P, row);
            const float s = scores[row];
            const u64 key = agg_pack(s, row - offsets[p]);
            const int a0 = koff0[p] + id0;
            if (best0[a0] == key && best1[koff1[p] + id1] == key) {
                matches0[a0] = id1;
                scores_f16[a0] = __builtin_bit_cast(unsigned short, (_Float16)s);   // round to nearest even, as gim_lg_emit_hloc
                len = id0 + 1;
            }
        }
    }
    const int p_hi = agg_wave_max(len > 0 ? p : -1), p_lo = -agg_wave_max(len > 0 ? -p : -0x7fffffff);
    const int len_max = agg_wave_max(len);
    if (p_hi < 0) return;                                                   // no survivor in this wave
    if (p_hi == p_lo) {
        if ((threadIdx.x & 63) == 0) atomicMax(&row_len[p_hi], len_max);
    } else if (len > 0) {
        atomicMax(&row_len[p], len);
    }
}

// max_error / patch -> the constants of the kernels; refuses, with a message, a geometry the kernels are not written for
int agg_conf(const char* who, float max_error, int patch, AggConf* c) {
    GIM_REQUIRE(max_error >= 1.0f && max_error <= 1024.0f, "%s: max_error=%g (1 <= max_error <= 1024)", who, (double)max_error);
    const int vote = (int)max_error;
    GIM_REQUIRE(patch >= 1 && patch <= 4096 && (float)patch >= max_error, "%s: patch=%d (max(cell_size, max_error), at most 4096)", who, patch);
    GIM_REQUIRE(patch % vote == 0 && patch / vote <= 8, "%s: patch / vote = %d / %d must be an integer in 1..8", who, patch, vote);
    GIM_REQUIRE(2.0f * max_error <= (float)patch, "%s: max_error=%g > patch / 2 = %g: a keypoint could be nearest from two cells away", who,
                (double)max_error, 0.5 * patch);
    c->max_error = max_error;
    c->patch = patch;
    c->vote = vote;
    c->fpatch = (float)patch;
    c->fvote = (float)vote;
    c->r = patch / vote;
    c->h = (c->r + 1) / 2;
    c->nb = 2 * c->h + 1;
    return GIM_OK;
}

int agg_rows(const char* who, int P, int row_lo, int row_hi, int pool_rows, int n_slots, int64_t total_cells) {
    GIM_REQUIRE(P >= 0 && n_slots >= 1 && total_cells >= 0, "%s: P=%d n_slots=%d total_cells=%lld (P >= 0, n_slots >= 1, total_cells >= 0)", who,
                P, n_slots, (long long)total_cells);
    GIM_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= pool_rows, "%s: rows [%d, %d) of a pool of %d", who, row_lo, row_hi, pool_rows);
    GIM_REQUIRE(total_cells <= 0x7fffffffLL, "%s: total_cells=%lld does not fit the int32 cell indices", who, (long long)total_cells);
    return GIM_OK;
}

inline unsigned agg_blocks(int64_t n) { return (unsigned)((n + AG_THREADS - 1) / AG_THREADS); }

inline bool agg_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int gim_agg_bins(float max_error, int patch) {
    AggConf c;
    if (agg_conf("gim_agg_bins", max_error, patch, &c) != GIM_OK) return 0;
    return c.nb * c.nb;
}

extern "C" int gim_agg_vote(const float* kpts0, const float* kpts1, const float* scores, const int32_t* offsets, const int32_t* slot0,
                            const int32_t* slot1, const int32_t* geom, uint64_t* votes, int32_t* cell_n, int32_t* dropped, int P,
                            int row_lo, int row_hi, int pool_rows, int n_slots, int64_t total_cells, float max_error, int patch,
                            gim_stream_t stream) {
    AggConf c;
    if (int rc = agg_conf("gim_agg_vote", max_error, patch, &c)) return rc;
    if (int rc = agg_rows("gim_agg_vote", P, row_lo, row_hi, pool_rows, n_slots, total_cells)) return rc;
    if (P == 0) return GIM_OK;
    GIM_REQUIRE(offsets && slot0 && slot1 && dropped, "gim_agg_vote: NULL pointer");
    GIM_REQUIRE(row_hi == row_lo || (kpts0 && kpts1 && scores && geom && votes && cell_n), "gim_agg_vote: NULL pointer");
    GIM_REQUIRE(!agg_misaligned(kpts0, 8) && !agg_misaligned(kpts1, 8) && !agg_misaligned(votes, 8), "gim_agg_vote: kpts0, kpts1 and votes must be 8-byte aligned");
    GIM_REQUIRE(!agg_misaligned(scores, 4) && !agg_misaligned(offsets, 4) && !agg_misaligned(slot0, 4) && !agg_misaligned(slot1, 4) &&
                !agg_misaligned(geom, 4) && !agg_misaligned(cell_n, 4) && !agg_misaligned(dropped, 4), "gim_agg_vote: misaligned 4-byte array");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(dropped, 0, (size_t)P * sizeof(int32_t), st) != hipSuccess) {
        gim_set_error("gim_agg_vote: hipMemsetAsync(dropped)");
        return GIM_ERR_LAUNCH;
    }
    if (row_hi == row_lo) return GIM_OK;
    // one lane per match: the workgroup count comes from the rows of the whole batch (8 192 matches are 32 workgroups)
    hipLaunchKernelGGL(agg_vote_kernel, dim3(agg_blocks((int64_t)row_hi - row_lo)), dim3(AG_THREADS), 0, st, (const f32x2_t*)kpts0,
                       (const f32x2_t*)kpts1, scores, offsets, slot0, slot1, geom, (u64*)votes, cell_n, dropped, P, row_lo, row_hi, n_slots,
                       total_cells, c);
    return gim_check_launch("agg_vote_kernel");
}

extern "C" int gim_agg_finalize(const uint64_t* votes, const int32_t* cell_n, int64_t total_cells, float max_error, int patch,
                                int64_t* cell_key, int32_t* cell_bin, gim_stream_t stream) {
    AggConf c;
    if (int rc = agg_conf("gim_agg_finalize", max_error, patch, &c)) return rc;
    GIM_REQUIRE(total_cells >= 0 && total_cells <= 0x7fffffffLL, "gim_agg_finalize: total_cells=%lld (0 <= total_cells < 2^31)", (long long)total_cells);
    if (total_cells == 0) return GIM_OK;
    GIM_REQUIRE(votes && cell_n && cell_key && cell_bin, "gim_agg_finalize: NULL pointer");
    GIM_REQUIRE(!agg_misaligned(votes, 8) && !agg_misaligned(cell_key, 8) && !agg_misaligned(cell_n, 4) && !agg_misaligned(cell_bin, 4),
                "gim_agg_finalize: votes and cell_key must be 8-byte aligned, cell_n and cell_bin 4-byte aligned");
    hipLaunchKernelGGL(agg_finalize_kernel, dim3(agg_blocks(total_cells)), dim3(AG_THREADS), 0, (hipStream_t)stream, (const u64*)votes, cell_n,
                       total_cells, c.nb * c.nb, cell_key, cell_bin);
    return gim_check_launch("agg_finalize_kernel");
}

extern "C" int gim_agg_keypoints(const uint64_t* votes, const int32_t* cell_bin, const int32_t* geom, const int32_t* sel,
                                 const int32_t* sel_slot, const int32_t* kp_off, int n_sel, int n_slots, int64_t total_cells,
                                 float max_error, int patch, int32_t* id_grid, float* keypoints, double* score, int32_t* cells,
                                 gim_stream_t stream) {
    AggConf c;
    if (int rc = agg_conf("gim_agg_keypoints", max_error, patch, &c)) return rc;
    GIM_REQUIRE(n_sel >= 0 && n_slots >= 1 && total_cells >= 0 && total_cells <= 0x7fffffffLL,
                "gim_agg_keypoints: n_sel=%d n_slots=%d total_cells=%lld (n_sel >= 0, n_slots >= 1, 0 <= total_cells < 2^31)", n_sel, n_slots,
                (long long)total_cells);
    if (total_cells == 0) return GIM_OK;
    GIM_REQUIRE(id_grid && !agg_misaligned(id_grid, 4), "gim_agg_keypoints: id_grid is NULL or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(id_grid, 0xff, (size_t)total_cells * sizeof(int32_t), st) != hipSuccess) {     // -1: no keypoint
        gim_set_error("gim_agg_keypoints: hipMemsetAsync(id_grid)");
        return GIM_ERR_LAUNCH;
    }
    if (n_sel == 0) return GIM_OK;
    GIM_REQUIRE(votes && cell_bin && geom && sel && sel_slot && kp_off && keypoints && score && cells, "gim_agg_keypoints: NULL pointer");
    GIM_REQUIRE(!agg_misaligned(votes, 8) && !agg_misaligned(keypoints, 8) && !agg_misaligned(score, 8), "gim_agg_keypoints: votes, keypoints and score must be 8-byte aligned");
    GIM_REQUIRE(!agg_misaligned(cell_bin, 4) && !agg_misaligned(geom, 4) && !agg_misaligned(sel, 4) && !agg_misaligned(sel_slot, 4) &&
                !agg_misaligned(kp_off, 4) && !agg_misaligned(cells, 4), "gim_agg_keypoints: misaligned 4-byte array");
    hipLaunchKernelGGL(agg_keypoints_kernel, dim3(agg_blocks(n_sel)), dim3(AG_THREADS), 0, st, (const u64*)votes, cell_bin, geom, sel, sel_slot,
                       kp_off, n_sel, n_slots, total_cells, c, id_grid, (f32x2_t*)keypoints, score, cells);
    return gim_check_launch("agg_keypoints_kernel");
}

extern "C" int64_t gim_agg_assign_ws_bytes(int n_rows, int rows0, int rows1) {
    if (n_rows < 0 || rows0 < 0 || rows1 < 0) return 0;
    return 8 * ((int64_t)rows0 + rows1) + 8 * (int64_t)n_rows;              // best0, best1 (64-bit) in front, then the two id arrays
}

extern "C" int gim_agg_assign(const float* kpts0, const float* kpts1, const float* scores, const int32_t* offsets, const int32_t* slot0,
                              const int32_t* slot1, const int32_t* geom, const int32_t* id_grid, const float* keypoints,
                              const int32_t* kp_off, const int32_t* koff0, const int32_t* koff1, int P, int row_lo, int row_hi,
                              int pool_rows, int n_slots, int64_t total_cells, int n_kp, int rows0, int rows1, float max_error, int patch,
                              int nearest, int32_t* matches0, void* scores_f16, int32_t* row_len, void* ws, gim_stream_t stream) {
    AggConf c;
    if (int rc = agg_conf("gim_agg_assign", max_error, patch, &c)) return rc;
    if (int rc = agg_rows("gim_agg_assign", P, row_lo, row_hi, pool_rows, n_slots, total_cells)) return rc;
    GIM_REQUIRE(n_kp >= 0 && rows0 >= 0 && rows1 >= 0, "gim_agg_assign: n_kp=%d rows0=%d rows1=%d must not be negative", n_kp, rows0, rows1);
    if (P == 0) return GIM_OK;
    GIM_REQUIRE(offsets && slot0 && slot1 && koff0 && koff1 && row_len, "gim_agg_assign: NULL pointer");
    GIM_REQUIRE(rows0 == 0 || (matches0 && scores_f16), "gim_agg_assign: NULL output rows");
    const int n = row_hi - row_lo;
    const bool work = n > 0 && rows0 > 0 && rows1 > 0 && n_kp > 0;
    GIM_REQUIRE(!work || (kpts0 && kpts1 && scores && geom && id_grid && keypoints && kp_off && ws), "gim_agg_assign: NULL pointer");
    GIM_REQUIRE(!agg_misaligned(kpts0, 8) && !agg_misaligned(kpts1, 8) && !agg_misaligned(keypoints, 8) && !agg_misaligned(ws, 8),
                "gim_agg_assign: kpts0, kpts1, keypoints and ws must be 8-byte aligned");
    GIM_REQUIRE(!agg_misaligned(scores, 4) && !agg_misaligned(offsets, 4) && !agg_misaligned(slot0, 4) && !agg_misaligned(slot1, 4) &&
                !agg_misaligned(geom, 4) && !agg_misaligned(id_grid, 4) && !agg_misaligned(kp_off, 4) && !agg_misaligned(koff0, 4) &&
                !agg_misaligned(koff1, 4) && !agg_misaligned(matches0, 4) && !agg_misaligned(row_len, 4) && !agg_misaligned(scores_f16, 2),
                "gim_agg_assign: misaligned array");
    hipStream_t st = (hipStream_t)stream;
    bool ok = hipMemsetAsync(row_len, 0, (size_t)P * sizeof(int32_t), st) == hipSuccess;
    if (rows0) {
        ok = ok && hipMemsetAsync(matches0, 0xff, (size_t)rows0 * sizeof(int32_t), st) == hipSuccess;      // -1: unmatched
        ok = ok && hipMemsetAsync(scores_f16, 0, (size_t)rows0 * 2, st) == hipSuccess;
    }
    if (work) ok = ok && hipMemsetAsync(ws, 0, 8 * ((size_t)rows0 + rows1), st) == hipSuccess;
    if (!ok) {
        gim_set_error("gim_agg_assign: hipMemsetAsync");
        return GIM_ERR_LAUNCH;
    }
    if (!work) return GIM_OK;
    u64* best0 = (u64*)ws;
    u64* best1 = best0 + rows0;
    int32_t* ids = (int32_t*)(best1 + rows1);
    hipLaunchKernelGGL(agg_ids_kernel, dim3(agg_blocks(n)), dim3(AG_THREADS), 0, st, (const f32x2_t*)kpts0, (const f32x2_t*)kpts1, scores,
                       offsets, slot0, slot1, geom, id_grid, (const f32x2_t*)keypoints, kp_off, koff0, koff1, P, row_lo, row_hi, n_slots,
                       total_cells, n_kp, rows0, rows1, nearest ? 1 : 0, c, ids, best0, best1);
    if (int rc = gim_check_launch("agg_ids_kernel")) return rc;
    hipLaunchKernelGGL(agg_emit_kernel, dim3(agg_blocks(n)), dim3(AG_THREADS), 0, st, scores, offsets, koff0, koff1, P, row_lo, row_hi, ids,
                       best0, best1, matches0, (unsigned short*)scores_f16, row_len);
    return gim_check_launch("agg_emit_kernel");
}
