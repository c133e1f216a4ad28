// Video pseudo-labels on the device (gfx950): `link` of the reference's datasets/walk/walk.py:217-247 as a hash join on rounded pixel
// keys with an ordered compaction, and the tail of a labelling step (video_preprocessor.py:513-555) as one compacting launch.
// The arithmetic is csrc/label_key.h; gim_amd/video_labels.py (link_tables, label_pack_np) is the numpy restatement.
//
// gim_label_link is three launches over B links:
//   build    one lane per row of either side: atomicMax(table[key], row + 1) -- the largest row of a key wins, as dict(zip(..)) keeps
//            the last one; rows without a usable key are counted
//   compact  one workgroup per link walks lab0 in chunks of LL_CHUNK rows: row i survives iff table0[key] == i + 1 and table1[key] > 0;
//            survivors are placed by a block scan with a carried offset -- plain stores, ascending i, no atomics
//   clear    one lane per row again: a zero into every slot `build` wrote, so that the workspace is all zero for the next call
#include "gim_common.h"
#include "label_key.h"

namespace {

constexpr int LL_THREADS = 1024, LL_WAVES = LL_THREADS / 64, LL_ITEMS = 4, LL_CHUNK = LL_THREADS * LL_ITEMS;
constexpr int LL_ROW_THREADS = 256;

struct LinkGeom {
    int lo0, n0, lo1, n1, w, h;
    bool ok;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the rows and the key range of link b (workgroup- or lane-local; every bound is clamped into the slabs, a link whose key range does
// not fit the workspace has no usable key)
__device__ __forceinline__ LinkGeom link_geom(int b, const int32_t* off0, const int32_t* off1, const int32_t* wh, int w1, int h1, int n0_total,
                                              int n1_total, int max_keys) {
    LinkGeom g;
    g.lo0 = off0 ? clampi(off0[b], 0, n0_total) : 0;
    g.n0 = max((off0 ? clampi(off0[b + 1], 0, n0_total) : n0_total) - g.lo0, 0);
    g.lo1 = off1 ? clampi(off1[b], 0, n1_total) : 0;
    g.n1 = max((off1 ? clampi(off1[b + 1], 0, n1_total) : n1_total) - g.lo1, 0);
    g.w = wh ? wh[2 * b] : w1;
    g.h = wh ? wh[2 * b + 1] : h1;
    g.ok = g.w >= 1 && g.h >= 1 && (int64_t)g.w * ((int64_t)g.h + 1) < (int64_t)max_keys;
    return g;
}

// the link that holds row `row` of a slab: the last b with off[b] <= row (offsets ascend), checked against its end by the caller
__device__ __forceinline__ int find_link(const int32_t* off, int B, int row) {
    if (!off) return 0;
    int lo = 0, hi = B - 1;
#pragma unroll 1
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// CLEAR = false: build; CLEAR = true: clear.  grid.x covers n0_total + n1_total rows, side 0 first.
template <bool CLEAR>
__global__ void __launch_bounds__(LL_ROW_THREADS) label_link_rows_kernel(const float4* __restrict__ lab0, const int32_t* __restrict__ off0,
                                                                         int n0_total, const float4* __restrict__ lab1,
                                                                         const int32_t* __restrict__ off1, int n1_total,
                                                                         const int32_t* __restrict__ wh, int w1, int h1, int B, int max_keys,
                                                                         int32_t* __restrict__ ws, int32_t* __restrict__ dropped) {
    const int64_t t = (int64_t)blockIdx.x * LL_ROW_THREADS + threadIdx.x;
    if (t >= (int64_t)n0_total + n1_total) return;
    const int side = t >= n0_total;
    const int row = side ? (int)(t - n0_total) : (int)t;
    const int b = find_link(side ? off1 : off0, B, row);
    const LinkGeom g = link_geom(b, off0, off1, wh, w1, h1, n0_total, n1_total, max_keys);
    const int i = row - (side ? g.lo1 : g.lo0);
    if (i < 0 || i >= (side ? g.n1 : g.n0)) return;              // a row outside every link
    const float4 r = side ? lab1[row] : lab0[row];
    const int slot = g.ok ? gim_label_slot(side ? gim_label_key(r.x, r.y, g.w) : gim_label_key(r.z, r.w, g.w), g.w, g.h) : -1;
    if (slot < 0) {
        if (!CLEAR) atomicAdd(dropped + 2 * b + side, 1);        // the exception: one atomic per such row
        return;
    }
    int32_t* cell = ws + ((int64_t)2 * b + side) * max_keys + slot;
    if (CLEAR) *cell = 0;
    else atomicMax(cell, i + 1);
}

__global__ void __launch_bounds__(LL_THREADS) label_link_compact_kernel(const float4* __restrict__ lab0, const int32_t* __restrict__ off0,
                                                                        int n0_total, const float4* __restrict__ lab1,
                                                                        const int32_t* __restrict__ off1, int n1_total,
                                                                        const int32_t* __restrict__ wh, int w1, int h1, int max_keys,
                                                                        const int32_t* __restrict__ ws, float4* __restrict__ out,
                                                                        int2* __restrict__ ij, int32_t* __restrict__ count) {
    __shared__ int sCnt[LL_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LinkGeom g = link_geom(b, off0, off1, wh, w1, h1, n0_total, n1_total, max_keys);   // workgroup-uniform
    const int32_t* t0 = ws + (int64_t)2 * b * max_keys;
    const int32_t* t1 = t0 + max_keys;
    int placed = 0;                                              // survivors of the chunks before this one
    if (g.ok) {
#pragma unroll 1
        for (int s0 = 0; s0 < g.n0; s0 += LL_CHUNK) {
            float4 r[LL_ITEMS];
            int j[LL_ITEMS];
            int mine = 0;
#pragma unroll
            for (int q = 0; q < LL_ITEMS; ++q) {
                const int i = s0 + tid * LL_ITEMS + q;
                j[q] = -1;
                if (i < g.n0) {
                    r[q] = lab0[g.lo0 + i];
                    const int slot = gim_label_slot(gim_label_key(r[q].z, r[q].w, g.w), g.w, g.h);
                    if (slot >= 0 && t0[slot] == i + 1) {
                        const int v = t1[slot];
                        if (v > 0 && v <= g.n1) j[q] = v - 1, ++mine;
                    }
                }
            }
            int incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (lane == 63) sCnt[wave] = incl;
            __syncthreads();
            int base = placed + incl - mine, total = placed;
#pragma unroll
            for (int w = 0; w < LL_WAVES; ++w) {
                if (w < wave) base += sCnt[w];
                total += sCnt[w];
            }
#pragma unroll
            for (int q = 0; q < LL_ITEMS; ++q) {
                if (j[q] >= 0) {
                    const float4 p = lab1[g.lo1 + j[q]];
                    out[g.lo0 + base] = make_float4(r[q].x, r[q].y, p.z, p.w);
                    ij[g.lo0 + base] = make_int2(s0 + tid * LL_ITEMS + q, j[q]);
                    ++base;
                }
            }
            placed = total;
            __syncthreads();                                     // sCnt is rewritten by the next chunk
        }
    }
    if (tid == 0) count[b] = placed;
}

struct PackAffine {
    double v[8];   // sx0, sy0, ox0, oy0, sx1, sy1, ox1, oy1
};

// one workgroup: the rows in chunks of LL_CHUNK, kept rows placed in input order by the same scan
template <bool AFFINE>
__global__ void __launch_bounds__(LL_THREADS) label_pack_kernel(const float2* __restrict__ k0, const float2* __restrict__ k1,
                                                                const uint8_t* __restrict__ keep, int n, float moved_thr, PackAffine a,
                                                                double vratio, float4* __restrict__ out, int32_t* __restrict__ count) {
    __shared__ int sCnt[LL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int placed = 0;
#pragma unroll 1
    for (int s0 = 0; s0 < n; s0 += LL_CHUNK) {
        float2 p0[LL_ITEMS], p1[LL_ITEMS];
        bool kept[LL_ITEMS];
        int mine = 0;
#pragma unroll
        for (int q = 0; q < LL_ITEMS; ++q) {
            const int i = s0 + tid * LL_ITEMS + q;
            kept[q] = false;
            if (i < n) {
                p0[q] = k0[i], p1[q] = k1[i];
                kept[q] = (keep == nullptr || keep[i] != 0) &&
                          (!(moved_thr > 0.0f) || gim_label_moved(p0[q].x, p0[q].y, p1[q].x, p1[q].y, moved_thr));
                mine += kept[q];
            }
        }
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) sCnt[wave] = incl;
        __syncthreads();
        int base = placed + incl - mine, total = placed;
#pragma unroll
        for (int w = 0; w < LL_WAVES; ++w) {
            if (w < wave) base += sCnt[w];
            total += sCnt[w];
        }
#pragma unroll
        for (int q = 0; q < LL_ITEMS; ++q) {
            if (kept[q]) {
                float4 o;
                if (AFFINE) {
                    o.x = gim_label_rescale(p0[q].x, a.v[0], a.v[2], vratio);
                    o.y = gim_label_rescale(p0[q].y, a.v[1], a.v[3], vratio);
                    o.z = gim_label_rescale(p1[q].x, a.v[4], a.v[6], vratio);
                    o.w = gim_label_rescale(p1[q].y, a.v[5], a.v[7], vratio);
                } else {
                    o.x = gim_label_scale(p0[q].x, vratio), o.y = gim_label_scale(p0[q].y, vratio);
                    o.z = gim_label_scale(p1[q].x, vratio), o.w = gim_label_scale(p1[q].y, vratio);
                }
                out[base++] = o;
            }
        }
        placed = total;
        __syncthreads();
    }
    if (tid == 0) *count = placed;
}

}  // namespace

extern "C" int64_t gim_label_link_ws_bytes(int B, int max_keys) {
    if (B < 0 || max_keys < 0) return -1;
    return (int64_t)B * 2 * (int64_t)max_keys * (int64_t)sizeof(int32_t);
}

extern "C" int gim_label_link(const float* lab0, const int32_t* off0, int n0_total, const float* lab1, const int32_t* off1, int n1_total,
                              const int32_t* wh, const int32_t* wh_dev, int B, int max_keys, void* ws, float* out, int32_t* ij,
                              int32_t* count, int32_t* dropped, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && B <= 65535, "gim_label_link: B=%d (0 <= B <= 65535)", B);
    GIM_REQUIRE(n0_total >= 0 && n1_total >= 0, "gim_label_link: negative row count (%d, %d)", n0_total, n1_total);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(wh, "gim_label_link: NULL wh");
    int64_t top = 0;
    for (int b = 0; b < B; ++b) {
        const int w = wh[2 * b], h = wh[2 * b + 1];
        GIM_REQUIRE(w >= 1 && h >= 1, "gim_label_link: link %d has width %d, height %d (both >= 1)", b, w, h);
        GIM_REQUIRE((int64_t)w * ((int64_t)h + 1) <= GIM_LABEL_MAX_KEY, "gim_label_link: link %d: key range %lld above 2^24", b,
                    (long long)w * ((long long)h + 1));
        top = (int64_t)w * (h + 1) > top ? (int64_t)w * (h + 1) : top;
    }
    GIM_REQUIRE(top < max_keys, "gim_label_link: max_keys=%d, the key range needs %lld", max_keys, (long long)top + 1);
    GIM_REQUIRE(B == 1 || (off0 && off1 && wh_dev), "gim_label_link: B=%d needs both offsets and wh_dev", B);
    GIM_REQUIRE((lab0 || n0_total == 0) && (lab1 || n1_total == 0) && ws && (out || n0_total == 0) && (ij || n0_total == 0) && count && dropped,
                "gim_label_link: NULL pointer");
    GIM_REQUIRE((((uintptr_t)lab0 | (uintptr_t)lab1 | (uintptr_t)out) & 15) == 0, "gim_label_link: lab0, lab1 and out must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)ij) & 7) == 0 && (((uintptr_t)off0 | (uintptr_t)off1 | (uintptr_t)wh_dev | (uintptr_t)ws | (uintptr_t)count |
                                                 (uintptr_t)dropped) & 3) == 0, "gim_label_link: misaligned offsets, wh_dev, ws, ij, count or dropped");
    const hipStream_t s = (hipStream_t)stream;
    const int w1 = wh[0], h1 = wh[1];
    if (hipMemsetAsync(dropped, 0, (size_t)B * 2 * sizeof(int32_t), s) != hipSuccess) {
        gim_set_error("gim_label_link: hipMemsetAsync failed");
        return GIM_ERR_LAUNCH;
    }
    const int64_t rows = (int64_t)n0_total + n1_total;
    const dim3 rgrid((unsigned)((rows + LL_ROW_THREADS - 1) / LL_ROW_THREADS)), rblock(LL_ROW_THREADS);
    if (rows)
        hipLaunchKernelGGL(label_link_rows_kernel<false>, rgrid, rblock, 0, s, (const float4*)lab0, off0, n0_total, (const float4*)lab1, off1,
                           n1_total, wh_dev, w1, h1, B, max_keys, (int32_t*)ws, dropped);
    hipLaunchKernelGGL(label_link_compact_kernel, dim3((unsigned)B), dim3(LL_THREADS), 0, s, (const float4*)lab0, off0, n0_total,
                       (const float4*)lab1, off1, n1_total, wh_dev, w1, h1, max_keys, (const int32_t*)ws, (float4*)out, (int2*)ij, count);
    if (rows)
        hipLaunchKernelGGL(label_link_rows_kernel<true>, rgrid, rblock, 0, s, (const float4*)lab0, off0, n0_total, (const float4*)lab1, off1,
                           n1_total, wh_dev, w1, h1, B, max_keys, (int32_t*)ws, dropped);
    return gim_check_launch("label_link kernels");
}

extern "C" int gim_label_pack(const float* k0, const float* k1, const uint8_t* keep, int n, float moved_thr, const double* affine,
                              double vratio, float* out, int32_t* count, gim_stream_t stream) {
    GIM_REQUIRE(n >= 0, "gim_label_pack: n=%d", n);
    GIM_REQUIRE(count && ((k0 && k1 && out) || n == 0), "gim_label_pack: NULL pointer");
    GIM_REQUIRE((((uintptr_t)k0 | (uintptr_t)k1) & 7) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)count) & 3) == 0,
                "gim_label_pack: k0 / k1 must be 8-byte, out 16-byte, count 4-byte aligned");
    PackAffine a = {};
    if (affine)
        for (int q = 0; q < 8; ++q) a.v[q] = affine[q];
    const dim3 grid(1), block(LL_THREADS);
    if (affine)
        hipLaunchKernelGGL(label_pack_kernel<true>, grid, block, 0, (hipStream_t)stream, (const float2*)k0, (const float2*)k1, keep, n, moved_thr,
                           a, vratio, (float4*)out, count);
    else
        hipLaunchKernelGGL(label_pack_kernel<false>, grid, block, 0, (hipStream_t)stream, (const float2*)k0, (const float2*)k1, keep, n, moved_thr,
                           a, vratio, (float4*)out, count);
    return gim_check_launch("label_pack_kernel");
}
