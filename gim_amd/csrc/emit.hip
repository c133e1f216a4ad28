// Output hand-out of the gim_loftr forward (gfx950): the small device-to-device moves that follow coarse matching.
//
// A HIP-graph replay re-uses its output buffers, so every forward hands out private copies of the M-row match lists
// (b_ids, i_ids, j_ids, m_bids, mkpts0_c, mkpts1_c, mconf) plus an all-false gt_mask: eight torch copy / fill kernels
// (clone, zeros) per forward before -- one launch here.  `gim_pack_matches` is the reporting row
// [pair_id, x0, y0, x1, y1, conf] of gim_amd/runner.py (was: index + 4-way torch.cat + a pageable host-to-device copy).
//
// `gim_fine_tile_list` turns the match lists into the ascending list of 8 x 32 patches of the 1/2-resolution maps that the fine level
// can read (5 x 5 windows at stride 4 around every coarse match, plus the 3 x 3 receptive field of the FPN's last convolution): the last
// two FPN layers then run on those patches only (conv_igemm.hip: gim_conv3x3_halo_tiles).  `gim_fine_tile_lists` also emits the list one
// pixel wider, for the lateral sum those layers read (gim_conv2d_ups_tiles); `gim_fine_tile_lists4` adds, still from that launch, the three
// patch lists of the 1/4-resolution maps that this lateral's upsample operand and the two 3 x 3 layers in front of it need (gim_conv2d_tiles).
//
// Replaces (reference file:line): the tensor construction at networks/loftr/utils/coarse_matching.py:236-259 as far as it
// only moves data, and the per-pair metric rows of trainer/lightning.py:258-270 (packed form).
#include "gim_common.h"

namespace {

struct Segs { gim_copy_segs s; };

// grid.y = segment; 16-byte lanes where source, destination and length allow, bytes otherwise.  src == NULL: zero fill.
__global__ void __launch_bounds__(256) copy_segments_kernel(const Segs a) {
    const int k = blockIdx.y;
    const char* src = (const char*)a.s.src[k];
    char* dst = (char*)a.s.dst[k];
    const int64_t n = a.s.bytes[k];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int64_t nv = vec ? n >> 4 : 0;
    for (int64_t i = t; i < nv; i += nt) ((uint4*)dst)[i] = src ? ((const uint4*)src)[i] : make_uint4(0u, 0u, 0u, 0u);
    for (int64_t i = (nv << 4) + t; i < n; i += nt) dst[i] = src ? src[i] : (char)0;
}

__global__ void __launch_bounds__(256) pack_matches_kernel(const int64_t* __restrict__ m_bids, const float2* __restrict__ mk0,
                                                           const float2* __restrict__ mk1, const float* __restrict__ conf,
                                                           const int64_t* __restrict__ pair_ids, int64_t pid_base,
                                                           float* __restrict__ out, int M) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int64_t b = m_bids[m];
    const float pid = (float)(pair_ids ? pair_ids[b] : pid_base + b);
    const float2 p0 = mk0[m], p1 = mk1[m];
    float* o = out + (size_t)m * 6;   // 24-byte rows: three 8-byte stores
    *(float2*)(o + 0) = make_float2(pid, p0.x);
    *(float2*)(o + 2) = make_float2(p0.y, p1.x);
    *(float2*)(o + 4) = make_float2(p1.y, conf[m]);
}

// One workgroup: zero the patch flags in LDS, mark the patches every match's reach touches, compact the flags in ascending order.
// The reach of match cell (cy, cx) is [stride * cy - 3, stride * cy + 3] x [stride * cx - 3, stride * cx + 3] clipped to the map: the fine
// window's +-2 (fine_fused.hip, gather) and one more pixel for the input of the last 3 x 3 convolution.  Rows whose ids lie outside the
// batch or the coarse map are skipped.
//
// REACH2 (gim_fine_tile_lists): a second list from the same launch -- the patches of the reach grown by one more pixel, +-4: what the
// INPUT of the last-but-one 3 x 3 convolution has to hold (the lateral sum x1_out, gim_conv2d_ups_tiles).  Flag bit 0 = the +-3 reach,
// bit 1 = the +-4 reach (a superset); one scan over the pair of counts, two compactions.
//
// QUARTER (gim_fine_tile_lists4): three more lists from the same launch, of 8 x 32 patches of the 1/4-resolution maps [2 bs, H / 2, W / 2]
// (h x w below).  The lateral launch that walks the +-4 list reads its upsample operand x2_out where Epilogue::ups_accumulate (conv_igemm.hip,
// lambda `issue`) STAGES it: for every 32-pixel pass (row Y, columns X0 .. X0 + 31) of a listed patch, source rows y0 = (int)(sy Y) and
// y1 = y0 + (y0 < h - 1), columns xa .. min(xa + 23, w - 1), xa = (int)(sx X0), in fp32 with sy = (float)(h - 1) / (float)(H - 1), sx
// likewise.  All 2 x 24 of them enter the MFMA, most with weight 0 -- and 0 x NaN = NaN, so every staged source must hold a computed value,
// not only those a pixel interpolates from.  S = the union of the staged sources, computed here with the same fp32 expressions.  Quarter
// flag bit 0 = the patch holds a pixel of S (list C: the last 3 x 3 layer in front of the lateral), bit 1 = of S dilated by 1 (list B: the
// 3 x 3 layer before it), bit 2 = of S dilated by 2 (list A: the 1/4-level lateral), dilations clipped to the map; C <= B <= A.  The
// dilation of a union is the union of the dilations, and the staged set of one half-level patch is a product rows x column range, so
// each listed patch marks rectangles of quarter patches.
constexpr int TL_THREADS = 1024, TL_MAX_FLAGS = 32768;

template <bool REACH2, bool QUARTER>
__device__ __forceinline__ void fine_tile_list_body(const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                                    const int64_t* __restrict__ j_ids, const int* __restrict__ count, int cap,
                                                    int bs, int w0c, int w1c, int stride, int H, int W,
                                                    int* __restrict__ tiles, int* __restrict__ n_tiles, int tiles_cap,
                                                    int* __restrict__ tiles2, int* __restrict__ n_tiles2,
                                                    int* __restrict__ tilesq, int* __restrict__ n_tilesq, int tilesq_cap,
                                                    int b_lo, int b_hi) {
    static_assert(!QUARTER || REACH2, "the quarter-level lists are derived from the +-4 flags");
    __shared__ __attribute__((aligned(16))) unsigned char flags[TL_MAX_FLAGS];
    __shared__ int part[TL_THREADS];
    __shared__ int part2[REACH2 ? TL_THREADS : 1];
    __shared__ int partq[QUARTER ? TL_THREADS : 1][2];   // [0]: |A| << 16 | |B| (each <= TL_MAX_FLAGS / 5 < 2^16), [1]: |C|
    const int t = threadIdx.x;
    const int tiles_x = (W + 31) / 32, tiles_y = (H + 7) / 8, per_img = tiles_x * tiles_y, nflags = 2 * bs * per_img;
    // QUARTER: the quarter-level flags live behind the half-level ones, from the next multiple of four on (word-wise atomicOr)
    const int h = H / 2, w = W / 2, qtiles_x = w / 32, qtiles_y = h / 8, qper_img = qtiles_x * qtiles_y;
    const int qbase = (nflags + 3) & ~3, nqflags = QUARTER ? 2 * bs * qper_img : 0;
    for (int i = t; i < (QUARTER ? qbase + nqflags : nflags); i += TL_THREADS) flags[i] = 0;
    __syncthreads();
    int M = count[0];
    M = M < 0 ? 0 : (M < cap ? M : cap);
    for (int m = t; m < M; m += TL_THREADS) {
        const int64_t b = b_ids[m];
        if (b < b_lo || b >= b_hi) continue;   // [b_lo, b_hi) lies inside [0, bs): a match of another pair range marks nothing
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int64_t cell = side ? j_ids[m] : i_ids[m];
            const int wc = side ? w1c : w0c;
            if (cell < 0 || cell >= (int64_t)wc * ((H + stride - 1) / stride)) continue;
            const int cy = (int)cell / wc, cx = (int)cell - cy * wc;
            int y0 = cy * stride - 3, y1 = cy * stride + 3, x0 = cx * stride - 3, x1 = cx * stride + 3;
            y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;
            y1 = y1 > H - 1 ? H - 1 : y1; x1 = x1 > W - 1 ? W - 1 : x1;
            if (y0 > y1 || x0 > x1) continue;
            const int img = side * bs + (int)b;
            if constexpr (REACH2) {
                // a patch of the +-3 reach gets 3, one that only the fourth pixel touches gets 2: bytes of different writers differ, so they
                // are OR-ed into the flag's 32-bit word
                int Y0 = cy * stride - 4, Y1 = cy * stride + 4, X0 = cx * stride - 4, X1 = cx * stride + 4;
                Y0 = Y0 < 0 ? 0 : Y0; X0 = X0 < 0 ? 0 : X0;
                Y1 = Y1 > H - 1 ? H - 1 : Y1; X1 = X1 > W - 1 ? W - 1 : X1;
                for (int ty = Y0 >> 3; ty <= (Y1 >> 3); ++ty)
                    for (int tx = X0 >> 5; tx <= (X1 >> 5); ++tx) {
                        const bool in3 = ty >= (y0 >> 3) && ty <= (y1 >> 3) && tx >= (x0 >> 5) && tx <= (x1 >> 5);
                        const int f = (img * tiles_y + ty) * tiles_x + tx;
                        atomicOr((unsigned*)flags + (f >> 2), (in3 ? 3u : 2u) << (8 * (f & 3)));
                    }
            } else {
            for (int ty = y0 >> 3; ty <= (y1 >> 3); ++ty)
                for (int tx = x0 >> 5; tx <= (x1 >> 5); ++tx) flags[(img * tiles_y + ty) * tiles_x + tx] = 1;   // (every writer stores the same byte)
            }
        }
    }
    __syncthreads();
    if constexpr (QUARTER) {
        unsigned char* const qf = flags + qbase;
        const float sy = (float)(h - 1) / (float)(H - 1), sx = (float)(w - 1) / (float)(W - 1);   // ups_accumulate's, to the letter
        for (int i = t; i < nflags; i += TL_THREADS) {
            if (!(flags[i] & 2)) continue;
            const int img = i / per_img, r = i - img * per_img, ty = r / tiles_x, tx = r - ty * tiles_x;
            const int xa = (int)(sx * (32 * tx));
            const int xe = xa + 23 < w - 1 ? xa + 23 : w - 1;
            for (int Y = 8 * ty; Y < 8 * ty + 8 && Y < H; ++Y) {
                const float fy = sy * Y;
                const int y0 = (int)fy, y1 = y0 + (y0 < h - 1 ? 1 : 0);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int ra = y0 - d > 0 ? y0 - d : 0, rb = y1 + d < h - 1 ? y1 + d : h - 1;
                    const int ca = xa - d > 0 ? xa - d : 0, cb = xe + d < w - 1 ? xe + d : w - 1;
                    const unsigned bits = d == 0 ? 7u : (d == 1 ? 6u : 4u);
                    for (int qy = ra >> 3; qy <= (rb >> 3); ++qy)
                        for (int qx = ca >> 5; qx <= (cb >> 5); ++qx) {
                            const int f = (img * qtiles_y + qy) * qtiles_x + qx;
                            if ((qf[f] & bits) != bits) atomicOr((unsigned*)qf + (f >> 2), bits << (8 * (f & 3)));
                        }
                }
            }
        }
        __syncthreads();
    }
    // ordered compaction: thread t owns flags [t * per, (t + 1) * per)
    const int per = (nflags + TL_THREADS - 1) / TL_THREADS;
    const int lo = t * per < nflags ? t * per : nflags, hi = lo + per < nflags ? lo + per : nflags;
    int n = 0, n2 = 0;
    for (int i = lo; i < hi; ++i) { n += flags[i] & 1; n2 += flags[i] >> 1; }
    part[t] = n;
    if constexpr (REACH2) part2[t] = n2;
    // QUARTER: thread t owns quarter flags [t * qper, (t + 1) * qper); the three counts ride the same scan
    const int qper = (nqflags + TL_THREADS - 1) / TL_THREADS;
    const int qlo = t * qper < nqflags ? t * qper : nqflags, qhi = qlo + qper < nqflags ? qlo + qper : nqflags;
    int nab = 0, nc = 0;
    if constexpr (QUARTER) {
        for (int i = qlo; i < qhi; ++i) {
            const int f = flags[qbase + i];
            nab += ((f >> 2) & 1) << 16 | ((f >> 1) & 1);
            nc += f & 1;
        }
        partq[t][0] = nab; partq[t][1] = nc;
    }
    __syncthreads();
    for (int d = 1; d < TL_THREADS; d <<= 1) {   // inclusive scan
        const int v = t >= d ? part[t - d] : 0;
        const int v2 = REACH2 && t >= d ? part2[t - d] : 0;
        const int vab = QUARTER && t >= d ? partq[t - d][0] : 0, vc = QUARTER && t >= d ? partq[t - d][1] : 0;
        __syncthreads();
        part[t] += v;
        if constexpr (REACH2) part2[t] += v2;
        if constexpr (QUARTER) { partq[t][0] += vab; partq[t][1] += vc; }
        __syncthreads();
    }
    int o = part[t] - n;
    for (int i = lo; i < hi; ++i)
        if (flags[i] & 1) {
            if (o < tiles_cap) tiles[o] = i;
            ++o;
        }
    if (t == TL_THREADS - 1) n_tiles[0] = part[t] < tiles_cap ? part[t] : tiles_cap;
    if constexpr (REACH2) {
        int o2 = part2[t] - n2;
        for (int i = lo; i < hi; ++i)
            if (flags[i] & 2) {
                if (o2 < tiles_cap) tiles2[o2] = i;
                ++o2;
            }
        if (t == TL_THREADS - 1) n_tiles2[0] = part2[t] < tiles_cap ? part2[t] : tiles_cap;
    }
    if constexpr (QUARTER) {
        // tilesq: three lists of tilesq_cap entries each -- A, B, C; n_tilesq: their three counts
        int oa = (partq[t][0] >> 16) - (nab >> 16), ob = (partq[t][0] & 0xffff) - (nab & 0xffff), oc = partq[t][1] - nc;
        for (int i = qlo; i < qhi; ++i) {
            const int f = flags[qbase + i];
            if (f & 4) { if (oa < tilesq_cap) tilesq[oa] = i; ++oa; }
            if (f & 2) { if (ob < tilesq_cap) tilesq[tilesq_cap + ob] = i; ++ob; }
            if (f & 1) { if (oc < tilesq_cap) tilesq[2 * tilesq_cap + oc] = i; ++oc; }
        }
        if (t == TL_THREADS - 1) {
            const int ta = partq[t][0] >> 16, tb = partq[t][0] & 0xffff, tc = partq[t][1];
            n_tilesq[0] = ta < tilesq_cap ? ta : tilesq_cap;
            n_tilesq[1] = tb < tilesq_cap ? tb : tilesq_cap;
            n_tilesq[2] = tc < tilesq_cap ? tc : tilesq_cap;
        }
    }
}

template <bool REACH2>
__global__ void __launch_bounds__(TL_THREADS) fine_tile_list_kernel(const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                                                  const int64_t* __restrict__ j_ids, const int* __restrict__ count, int cap,
                                                                  int bs, int w0c, int w1c, int stride, int H, int W,
                                                                  int* __restrict__ tiles, int* __restrict__ n_tiles, int tiles_cap,
                                                                  int* __restrict__ tiles2, int* __restrict__ n_tiles2) {
    fine_tile_list_body<REACH2, false>(b_ids, i_ids, j_ids, count, cap, bs, w0c, w1c, stride, H, W, tiles, n_tiles, tiles_cap, tiles2, n_tiles2,
                                       nullptr, nullptr, 0, 0, bs);
}

__global__ void __launch_bounds__(TL_THREADS) fine_tile_lists4_kernel(const int64_t* __restrict__ b_ids, const int64_t* __restrict__ i_ids,
                                                                    const int64_t* __restrict__ j_ids, const int* __restrict__ count, int cap,
                                                                    int bs, int w0c, int w1c, int stride, int H, int W,
                                                                    int* __restrict__ tiles, int* __restrict__ n_tiles, int tiles_cap,
                                                                    int* __restrict__ tiles2, int* __restrict__ n_tiles2,
                                                                    int* __restrict__ tilesq, int* __restrict__ n_tilesq, int tilesq_cap,
                                                                    int b_lo, int b_hi) {
    fine_tile_list_body<true, true>(b_ids, i_ids, j_ids, count, cap, bs, w0c, w1c, stride, H, W, tiles, n_tiles, tiles_cap, tiles2, n_tiles2,
                                    tilesq, n_tilesq, tilesq_cap, b_lo, b_hi);
}

}  // namespace

extern "C" int gim_fine_tile_list_max_flags(void) { return TL_MAX_FLAGS; }

extern "C" int gim_fine_tile_list(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                                  int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int tiles_cap, gim_stream_t stream) {
    GIM_REQUIRE(b_ids && i_ids && j_ids && count && tiles && n_tiles, "gim_fine_tile_list: NULL pointer");
    GIM_REQUIRE(cap >= 0 && bs > 0 && w0c > 0 && w1c > 0 && stride > 0 && H > 0 && W > 0, "gim_fine_tile_list: bad geometry");
    const int64_t nflags = 2ll * bs * ((W + 31) / 32) * ((H + 7) / 8);
    GIM_REQUIRE(nflags <= TL_MAX_FLAGS, "gim_fine_tile_list: %lld patches exceed the %d flags of the one-workgroup kernel", (long long)nflags, TL_MAX_FLAGS);
    GIM_REQUIRE(tiles_cap >= nflags, "gim_fine_tile_list: the list holds %d entries, the maps have %lld patches", tiles_cap, (long long)nflags);
    hipLaunchKernelGGL(fine_tile_list_kernel<false>, dim3(1), dim3(TL_THREADS), 0, (hipStream_t)stream, b_ids, i_ids, j_ids, count, cap, bs, w0c, w1c,
                       stride, H, W, tiles, n_tiles, tiles_cap, nullptr, nullptr);
    return gim_check_launch("fine_tile_list_kernel");
}

// gim_fine_tile_list plus, from the same launch, the list of the reach grown to +-4 (tiles4 / n_tiles4, the same capacity)
extern "C" int gim_fine_tile_lists(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                                   int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int* tiles4, int* n_tiles4,
                                   int tiles_cap, gim_stream_t stream) {
    GIM_REQUIRE(b_ids && i_ids && j_ids && count && tiles && n_tiles && tiles4 && n_tiles4, "gim_fine_tile_lists: NULL pointer");
    GIM_REQUIRE(cap >= 0 && bs > 0 && w0c > 0 && w1c > 0 && stride > 0 && H > 0 && W > 0, "gim_fine_tile_lists: bad geometry");
    const int64_t nflags = 2ll * bs * ((W + 31) / 32) * ((H + 7) / 8);
    GIM_REQUIRE(nflags <= TL_MAX_FLAGS, "gim_fine_tile_lists: %lld patches exceed the %d flags of the one-workgroup kernel", (long long)nflags, TL_MAX_FLAGS);
    GIM_REQUIRE(tiles_cap >= nflags, "gim_fine_tile_lists: the lists hold %d entries each, the maps have %lld patches", tiles_cap, (long long)nflags);
    hipLaunchKernelGGL(fine_tile_list_kernel<true>, dim3(1), dim3(TL_THREADS), 0, (hipStream_t)stream, b_ids, i_ids, j_ids, count, cap, bs, w0c, w1c,
                       stride, H, W, tiles, n_tiles, tiles_cap, tiles4, n_tiles4);
    return gim_check_launch("fine_tile_list_kernel");
}

// gim_fine_tile_lists plus, from the same launch, the three patch lists of the 1/4-resolution maps [2 bs, H / 2, W / 2] (see QUARTER above):
// tilesq = int32 [3][tilesq_cap], lists A, B, C in that order; n_tilesq = int32 [3].  Only the matches of the pairs [b_lo, b_hi) mark
// patches (gim_fine_tile_lists4: all of them, [0, bs)): the forward's two pair-range chains each build the lists of their own images.
extern "C" int gim_fine_tile_lists4_range(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                                          int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int* tiles4, int* n_tiles4,
                                          int tiles_cap, int* tilesq, int* n_tilesq, int tilesq_cap, int b_lo, int b_hi, gim_stream_t stream) {
    GIM_REQUIRE(b_ids && i_ids && j_ids && count && tiles && n_tiles && tiles4 && n_tiles4 && tilesq && n_tilesq, "gim_fine_tile_lists4: NULL pointer");
    GIM_REQUIRE(cap >= 0 && bs > 0 && w0c > 0 && w1c > 0 && stride > 0 && H > 0 && W > 0, "gim_fine_tile_lists4: bad geometry");
    GIM_REQUIRE(0 <= b_lo && b_lo <= b_hi && b_hi <= bs, "gim_fine_tile_lists4: the pair range [%d, %d) is not inside [0, %d)", b_lo, b_hi, bs);
    GIM_REQUIRE(H % 16 == 0 && W % 64 == 0, "gim_fine_tile_lists4: the 1/4-resolution maps (%d x %d) must be whole 8 x 32 patches", H / 2, W / 2);
    const int64_t nflags = 2ll * bs * (W / 32) * (H / 8), nq = 2ll * bs * (W / 64) * (H / 16);
    GIM_REQUIRE(((nflags + 3) & ~3ll) + nq <= TL_MAX_FLAGS, "gim_fine_tile_lists4: %lld + %lld patches exceed the %d flags of the one-workgroup kernel",
                (long long)nflags, (long long)nq, TL_MAX_FLAGS);
    GIM_REQUIRE(tiles_cap >= nflags && tilesq_cap >= nq, "gim_fine_tile_lists4: the lists hold %d / %d entries each, the maps have %lld / %lld patches",
                tiles_cap, tilesq_cap, (long long)nflags, (long long)nq);
    hipLaunchKernelGGL(fine_tile_lists4_kernel, dim3(1), dim3(TL_THREADS), 0, (hipStream_t)stream, b_ids, i_ids, j_ids, count, cap, bs, w0c, w1c,
                       stride, H, W, tiles, n_tiles, tiles_cap, tiles4, n_tiles4, tilesq, n_tilesq, tilesq_cap, b_lo, b_hi);
    return gim_check_launch("fine_tile_lists4_kernel");
}

extern "C" int gim_fine_tile_lists4(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                                    int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int* tiles4, int* n_tiles4,
                                    int tiles_cap, int* tilesq, int* n_tilesq, int tilesq_cap, gim_stream_t stream) {
    return gim_fine_tile_lists4_range(b_ids, i_ids, j_ids, count, cap, bs, w0c, w1c, stride, H, W, tiles, n_tiles, tiles4, n_tiles4, tiles_cap,
                                      tilesq, n_tilesq, tilesq_cap, 0, bs, stream);
}

extern "C" int gim_copy_segments(const gim_copy_segs* sp, gim_stream_t stream) {
    GIM_REQUIRE(sp, "gim_copy_segments: NULL args");
    GIM_REQUIRE(sp->n >= 0 && sp->n <= GIM_MAX_COPY_SEGS, "gim_copy_segments: n=%d outside [0, %d]", sp->n, GIM_MAX_COPY_SEGS);
    int64_t mx = 0;
    for (int k = 0; k < sp->n; ++k) {
        GIM_REQUIRE(sp->bytes[k] >= 0 && (sp->bytes[k] == 0 || sp->dst[k]), "gim_copy_segments: segment %d: bad size / NULL dst", k);
        mx = sp->bytes[k] > mx ? sp->bytes[k] : mx;
    }
    if (sp->n == 0 || mx == 0) return GIM_OK;
    Segs a;
    a.s = *sp;
    int64_t blocks = (mx / 16 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(copy_segments_kernel, dim3((unsigned)blocks, (unsigned)sp->n), dim3(256), 0, (hipStream_t)stream, a);
    return gim_check_launch("copy_segments_kernel");
}

extern "C" int gim_pack_matches(const int64_t* m_bids, const float* mkpts0, const float* mkpts1, const float* mconf,
                                const int64_t* pair_ids, int64_t pid_base, float* out, int M, gim_stream_t stream) {
    GIM_REQUIRE(M >= 0, "gim_pack_matches: M=%d", M);
    if (M == 0) return GIM_OK;
    GIM_REQUIRE(m_bids && mkpts0 && mkpts1 && mconf && out, "gim_pack_matches: NULL pointer");
    hipLaunchKernelGGL(pack_matches_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m_bids,
                       (const float2*)mkpts0, (const float2*)mkpts1, mconf, pair_ids, pid_base, out, M);
    return gim_check_launch("pack_matches_kernel");
}
