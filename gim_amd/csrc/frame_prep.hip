// Frame preparation of the video labeller on the device (gfx950): the stretch between a decoded frame and a matcher's input, the
// reference's video_preprocessor.py:292-366 (crop to the previous pass's labels, INTER_AREA resize, class-exclusion mask through two
// nearest-neighbour resizes), :406-493 (the per-method tensors) and :603-621 (the segmenter's input), for a table of jobs in one launch.
// The arithmetic is csrc/frame_prep_math.h; gim_amd/frame_prep.py (frame_prep_np) is the numpy restatement.
//
// One workgroup of 256 lanes owns one tile (at most 64 x 16 output pixels, smaller where a job's factor is large) of one job; the
// (job, tile) work table is built on the host from the whole batch.  A workgroup
//   1. tabulates the coverage weights of its tile's columns and rows in LDS (double arithmetic, rounded once to fp32);
//   2. stages the source footprint of the tile in LDS, row by row, with 16-byte loads from the 16-byte aligned address at or below each
//      row's first byte (the bytes in front are the row's shift; a granule that would reach past the slab is read byte by byte);
//   3. computes every pixel from LDS: per channel t_y = sum_k wx_k * src[y][k], v = sum_y wy_y * t_y in fp32, k and y ascending, each
//      product and sum rounded separately, then rintf and the clamp to a byte; the mask by the integer chain; the requested outputs
//      by plain vector stores; the kept count by an integer sum over the wave and one integer atomic per wave.
// LDS: 40 KiB footprint + 5.6 KiB weight tables + 256 B exclusion table: three workgroups per CU.  No scratch, every loop bounded.
#include "gim_common.h"
#include "frame_prep_math.h"

namespace {

constexpr int FP_THREADS = 256;

struct FpOut {
    uint8_t* u8;
    uint8_t* mask;
    uint8_t* mask8;
    float* rgb;
    float* gray;
    float* norm;
    int32_t* kept;
};

__global__ __launch_bounds__(FP_THREADS) void frame_prep_kernel(const uint8_t* __restrict__ frames, int H, int W, int64_t slab_bytes,
                                                                 const uint8_t* __restrict__ seg, int Hs, int Ws,
                                                                 const uint8_t* __restrict__ exclude, const int64_t* __restrict__ jobs,
                                                                 const int4* __restrict__ work, FpOut out) {
    __shared__ __attribute__((aligned(16))) uint8_t sSrc[GIM_FP_LDS_BYTES];
    __shared__ float sWx[GIM_FP_TILE_W][GIM_FP_TAPS];
    __shared__ float sWy[GIM_FP_TILE_H][GIM_FP_TAPS];
    __shared__ int sKx[GIM_FP_TILE_W], sNx[GIM_FP_TILE_W], sKy[GIM_FP_TILE_H], sNy[GIM_FP_TILE_H];
    __shared__ __attribute__((aligned(16))) uint8_t sExcl[256];

    const int tid = threadIdx.x;
    const int4 wk = work[blockIdx.x];
    const int64_t* jb = jobs + (int64_t)wk.x * GIM_FP_JOB_WORDS;
    const int slot = (int)jb[GIM_FP_SLOT], x0 = (int)jb[GIM_FP_X0], y0 = (int)jb[GIM_FP_Y0];
    const int wc = (int)jb[GIM_FP_X1] - x0, hc = (int)jb[GIM_FP_Y1] - y0;
    const int wn = (int)jb[GIM_FP_WN], hn = (int)jb[GIM_FP_HN], flags = (int)jb[GIM_FP_FLAGS];
    const int ox0 = wk.y, oy0 = wk.z;
    const int tw = min((int)jb[GIM_FP_TW], wn - ox0), th = min((int)jb[GIM_FP_TH], hn - oy0);
    // the entry point has checked every job and every work item; these bounds only keep a stale table from leaving the buffers
    if (tw < 1 || th < 1 || tw > GIM_FP_TILE_W || th > GIM_FP_TILE_H || wc < 1 || hc < 1 || ox0 < 0 || oy0 < 0) return;

    // ---- 1. weight tables ------------------------------------------------------------------------------------------------------
    for (int i = tid; i < (tw + th) * GIM_FP_TAPS; i += FP_THREADS) {
        const int e = i / GIM_FP_TAPS, t = i - e * GIM_FP_TAPS;
        const bool isx = e < tw;
        const int d = isx ? ox0 + e : oy0 + (e - tw), n = isx ? wc : hc, m = isx ? wn : hn;
        int cnt;
        const int k0 = gim_fp_span(d, n, m, &cnt);
        cnt = min(cnt, GIM_FP_TAPS);
        const float w = t < cnt ? gim_fp_weight(d, k0 + t, n, m) : 0.0f;
        if (isx) {
            sWx[e][t] = w;
            if (t == 0) sKx[e] = k0, sNx[e] = cnt;
        } else {
            sWy[e - tw][t] = w;
            if (t == 0) sKy[e - tw] = k0, sNy[e - tw] = cnt;
        }
    }
    if (tid < 16) reinterpret_cast<uint4*>(sExcl)[tid] = reinterpret_cast<const uint4*>(exclude)[tid];

    // ---- 2. the source footprint -----------------------------------------------------------------------------------------------
    int c0, c1, r0, r1;
    c0 = gim_fp_span(ox0, wc, wn, &c1);
    r0 = gim_fp_span(oy0, hc, hn, &r1);
    {
        int cnt;
        const int k = gim_fp_span(ox0 + tw - 1, wc, wn, &cnt);
        c1 = min(k + cnt, wc);
        const int q = gim_fp_span(oy0 + th - 1, hc, hn, &cnt);
        r1 = min(q + cnt, hc);
    }
    const int ncols = c1 - c0, nrows = r1 - r0;
    const int cpr = (ncols * 3 + 15 + 15) >> 4;          // 16-byte granules per row, the shift in front included
    const int pitch = cpr << 4;
    if (ncols < 1 || nrows < 1 || (int64_t)nrows * pitch > GIM_FP_LDS_BYTES) return;
    const int64_t row_bytes = (int64_t)W * 3;
    const int64_t first = ((int64_t)slot * H + (y0 + r0)) * row_bytes + (int64_t)(x0 + c0) * 3;   // byte of the footprint's first pixel
    for (int i = tid; i < nrows * cpr; i += FP_THREADS) {
        const int r = i / cpr, c = i - r * cpr;
        const int64_t g = first + (int64_t)r * row_bytes;
        const int shift = (int)(g & 15);
        if (c * 16 >= shift + ncols * 3) continue;        // nothing of this row in the granule
        const int64_t a = (g - shift) + (int64_t)c * 16;
        uint8_t* dst = sSrc + r * pitch + c * 16;
        if (a + 16 <= slab_bytes) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(frames + a);
        } else {
            for (int b = 0; b < 16; ++b) dst[b] = a + b < slab_bytes ? frames[a + b] : (uint8_t)0;
        }
    }
    __syncthreads();

    // ---- 3. the pixels ---------------------------------------------------------------------------------------------------------
    const bool want_mask = (flags & (GIM_FP_OUT_MASK | GIM_FP_OUT_MASK8 | GIM_FP_MASKED)) != 0 || out.kept != nullptr;
    const int64_t plane = (int64_t)hn * wn;
    int kept = 0;
    for (int p0 = 0; p0 < tw * th; p0 += FP_THREADS) {       // at most GIM_FP_TILE_W * GIM_FP_TILE_H / FP_THREADS = 4 rounds
        const int p = p0 + tid;
        if (p < tw * th) {
            const int ty = p / tw, tx = p - ty * tw;
            const int ox = ox0 + tx, oy = oy0 + ty;
            const int kx = sKx[tx] - c0, nx = sNx[tx], ky = sKy[ty] - r0, ny = sNy[ty];
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
            for (int iy = 0; iy < ny; ++iy) {
                const int r = ky + iy;
                const int shift = (int)((first + (int64_t)r * row_bytes) & 15);
                const uint8_t* src = sSrc + r * pitch + shift + kx * 3;
                float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
                for (int ix = 0; ix < nx; ++ix) {
                    const float w = sWx[tx][ix];
                    t0 = gim_fp_acc(t0, w, (float)src[ix * 3]);
                    t1 = gim_fp_acc(t1, w, (float)src[ix * 3 + 1]);
                    t2 = gim_fp_acc(t2, w, (float)src[ix * 3 + 2]);
                }
                const float wy = sWy[ty][iy];
                v0 = gim_fp_acc(v0, wy, t0);
                v1 = gim_fp_acc(v1, wy, t1);
                v2 = gim_fp_acc(v2, wy, t2);
            }
            const uint8_t b0 = gim_fp_round_u8(v0), b1 = gim_fp_round_u8(v1), b2 = gim_fp_round_u8(v2);
            uint8_t m = 1;
            if (want_mask) {
                const int sx = gim_fp_mask_index(ox, x0, wc, wn, W, Ws), sy = gim_fp_mask_index(oy, y0, hc, hn, H, Hs);
                m = sExcl[seg[((int64_t)slot * Hs + sy) * Ws + sx]] ? 0 : 1;
                kept += m;
            }
            const int64_t px = (int64_t)oy * wn + ox;
            if (flags & GIM_FP_OUT_U8) {
                uint8_t* o = out.u8 + jb[GIM_FP_OFF_U8] + px * 3;
                o[0] = b0, o[1] = b1, o[2] = b2;
            }
            if (flags & GIM_FP_OUT_MASK) out.mask[jb[GIM_FP_OFF_MASK] + px] = m;
            if ((flags & GIM_FP_OUT_MASK8) && (ox & 7) == 0 && (oy & 7) == 0)
                out.mask8[jb[GIM_FP_OFF_MASK8] + (int64_t)(oy >> 3) * (wn >> 3) + (ox >> 3)] = m;
            const uint8_t mm = (flags & GIM_FP_MASKED) ? m : (uint8_t)1;
            if (flags & GIM_FP_OUT_RGB) {
                float* o = out.rgb + jb[GIM_FP_OFF_RGB] + px;
                o[0] = gim_fp_unit((uint8_t)(b0 * mm)), o[plane] = gim_fp_unit((uint8_t)(b1 * mm)), o[2 * plane] = gim_fp_unit((uint8_t)(b2 * mm));
            }
            if (flags & GIM_FP_OUT_GRAY) out.gray[jb[GIM_FP_OFF_GRAY] + px] = gim_fp_unit((uint8_t)(gim_fp_gray(b0, b1, b2) * mm));
            if (flags & GIM_FP_OUT_NORM) {
                float* o = out.norm + jb[GIM_FP_OFF_NORM] + px;
                o[0] = gim_fp_norm(b0, 0), o[plane] = gim_fp_norm(b1, 1), o[2 * plane] = gim_fp_norm(b2, 2);
            }
        }
    }
    if (out.kept != nullptr) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) kept += __shfl_down(kept, o, 64);
        if ((tid & 63) == 0 && kept) atomicAdd(out.kept + wk.x, kept);
    }
}

}  // namespace

extern "C" int gim_frame_prep_tile(int wc, int hc, int wn, int hn, int* tw, int* th) {
    GIM_REQUIRE(tw && th, "gim_frame_prep_tile: NULL pointer");
    GIM_REQUIRE(wc >= 1 && hc >= 1 && wn >= 1 && hn >= 1, "gim_frame_prep_tile: crop %d x %d -> %d x %d (all >= 1)", wc, hc, wn, hn);
    GIM_REQUIRE((int64_t)wc <= (int64_t)GIM_FP_MAX_FACTOR * wn && (int64_t)hc <= (int64_t)GIM_FP_MAX_FACTOR * hn,
                "gim_frame_prep_tile: crop %d x %d -> %d x %d shrinks an axis by more than %d", wc, hc, wn, hn, GIM_FP_MAX_FACTOR);
    int w = GIM_FP_TILE_W, h = GIM_FP_TILE_H;
    while (gim_fp_tile_bytes(w, h, wc, wn, hc, hn) > GIM_FP_LDS_BYTES && (w > 1 || h > 1)) {
        if (h > 1) h >>= 1;
        else w >>= 1;
    }
    GIM_REQUIRE(gim_fp_tile_bytes(w, h, wc, wn, hc, hn) <= GIM_FP_LDS_BYTES, "gim_frame_prep_tile: no tile fits");
    *tw = w, *th = h;
    return GIM_OK;
}

extern "C" int gim_frame_prep(const uint8_t* frames, int S, int H, int W, const uint8_t* seg, int Hs, int Ws, const uint8_t* exclude,
                              const int64_t* jobs, const int64_t* jobs_dev, int J, const int32_t* work, const int32_t* work_dev, int n_work,
                              const int64_t* out_elems, uint8_t* out_u8, uint8_t* out_mask, uint8_t* out_mask8, float* out_rgb,
                              float* out_gray, float* out_norm, int32_t* kept, gim_stream_t stream) {
    GIM_REQUIRE(J >= 0 && n_work >= 0, "gim_frame_prep: J=%d, n_work=%d", J, n_work);
    if (J == 0 || n_work == 0) return GIM_OK;
    GIM_REQUIRE(frames && exclude && jobs && jobs_dev && work && work_dev && out_elems, "gim_frame_prep: NULL pointer");
    GIM_REQUIRE(S >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "gim_frame_prep: frames [%d, %d, %d, 3]", S, H, W);
    GIM_REQUIRE((((uintptr_t)frames | (uintptr_t)exclude | (uintptr_t)work_dev) & 15) == 0 && ((uintptr_t)jobs_dev & 7) == 0 &&
                    (((uintptr_t)out_rgb | (uintptr_t)out_gray | (uintptr_t)out_norm | (uintptr_t)kept) & 3) == 0,
                "gim_frame_prep: frames, exclude and work_dev must be 16-byte, jobs_dev 8-byte, the fp32 / int32 outputs 4-byte aligned");
    const void* outs[6] = {out_u8, out_mask, out_mask8, out_rgb, out_gray, out_norm};
    bool need_seg = kept != nullptr;
    for (int j = 0; j < J; ++j) {
        const int64_t* jb = jobs + (int64_t)j * GIM_FP_JOB_WORDS;
        const int64_t x0 = jb[GIM_FP_X0], y0 = jb[GIM_FP_Y0], x1 = jb[GIM_FP_X1], y1 = jb[GIM_FP_Y1], wn = jb[GIM_FP_WN], hn = jb[GIM_FP_HN];
        const int64_t flags = jb[GIM_FP_FLAGS];
        GIM_REQUIRE(jb[GIM_FP_SLOT] >= 0 && jb[GIM_FP_SLOT] < S, "gim_frame_prep: job %d names slot %lld of %d", j, (long long)jb[GIM_FP_SLOT], S);
        GIM_REQUIRE(0 <= x0 && x0 < x1 && x1 <= W && 0 <= y0 && y0 < y1 && y1 <= H, "gim_frame_prep: job %d: box (%lld, %lld, %lld, %lld) in a %d x %d frame",
                    j, (long long)x0, (long long)y0, (long long)x1, (long long)y1, W, H);
        GIM_REQUIRE(wn >= 1 && hn >= 1 && wn <= 32768 && hn <= 32768, "gim_frame_prep: job %d: output %lld x %lld", j, (long long)wn, (long long)hn);
        GIM_REQUIRE(x1 - x0 <= GIM_FP_MAX_FACTOR * wn && y1 - y0 <= GIM_FP_MAX_FACTOR * hn,
                    "gim_frame_prep: job %d: %lld x %lld -> %lld x %lld shrinks an axis by more than %d", j, (long long)(x1 - x0),
                    (long long)(y1 - y0), (long long)wn, (long long)hn, GIM_FP_MAX_FACTOR);
        GIM_REQUIRE(flags >= 0 && (flags & ~(int64_t)GIM_FP_ALL_FLAGS) == 0, "gim_frame_prep: job %d: flags %lld", j, (long long)flags);
        GIM_REQUIRE(!(flags & GIM_FP_OUT_MASK8) || (wn % 8 == 0 && hn % 8 == 0), "gim_frame_prep: job %d: mask8 needs an output of multiples of 8, got %lld x %lld",
                    j, (long long)wn, (long long)hn);
        const int64_t tw = jb[GIM_FP_TW], th = jb[GIM_FP_TH];
        GIM_REQUIRE(tw >= 1 && tw <= GIM_FP_TILE_W && th >= 1 && th <= GIM_FP_TILE_H &&
                        gim_fp_tile_bytes((int)tw, (int)th, (int)(x1 - x0), (int)wn, (int)(y1 - y0), (int)hn) <= GIM_FP_LDS_BYTES,
                    "gim_frame_prep: job %d: a %lld x %lld tile does not fit (gim_frame_prep_tile)", j, (long long)tw, (long long)th);
        const int64_t need[6] = {hn * wn * 3, hn * wn, (hn / 8) * (wn / 8), hn * wn * 3, hn * wn, hn * wn * 3};
        for (int o = 0; o < 6; ++o) {
            if (!(flags & (1 << o))) continue;
            const int64_t off = jb[GIM_FP_OFF_U8 + o];
            GIM_REQUIRE(outs[o] != nullptr, "gim_frame_prep: job %d asks for output %d, its buffer is NULL", j, o);
            GIM_REQUIRE(off >= 0 && off + need[o] <= out_elems[o], "gim_frame_prep: job %d: output %d at %lld + %lld leaves its buffer of %lld", j, o,
                        (long long)off, (long long)need[o], (long long)out_elems[o]);
        }
        need_seg = need_seg || (flags & (GIM_FP_OUT_MASK | GIM_FP_OUT_MASK8 | GIM_FP_MASKED)) != 0;
    }
    GIM_REQUIRE(!need_seg || (seg && Hs >= 1 && Ws >= 1 && Hs <= 32768 && Ws <= 32768), "gim_frame_prep: a mask needs class maps, got [%d, %d]", Hs, Ws);
    for (int i = 0; i < n_work; ++i) {
        const int32_t* wk = work + (int64_t)i * 4;
        GIM_REQUIRE(wk[0] >= 0 && wk[0] < J, "gim_frame_prep: work item %d names job %d of %d", i, wk[0], J);
        const int64_t* jb = jobs + (int64_t)wk[0] * GIM_FP_JOB_WORDS;
        GIM_REQUIRE(wk[1] >= 0 && wk[1] < jb[GIM_FP_WN] && wk[1] % jb[GIM_FP_TW] == 0 && wk[2] >= 0 && wk[2] < jb[GIM_FP_HN] && wk[2] % jb[GIM_FP_TH] == 0,
                    "gim_frame_prep: work item %d: tile origin (%d, %d) of job %d", i, wk[1], wk[2], wk[0]);
    }
    const hipStream_t s = (hipStream_t)stream;
    if (kept && hipMemsetAsync(kept, 0, (size_t)J * sizeof(int32_t), s) != hipSuccess) {
        gim_set_error("gim_frame_prep: hipMemsetAsync failed");
        return GIM_ERR_LAUNCH;
    }
    const FpOut out = {out_u8, out_mask, out_mask8, out_rgb, out_gray, out_norm, kept};
    hipLaunchKernelGGL(frame_prep_kernel, dim3((unsigned)n_work), dim3(FP_THREADS), 0, s, frames, H, W, (int64_t)S * H * W * 3, seg, Hs, Ws, exclude,
                       jobs_dev, (const int4*)work_dev, out);
    return gim_check_launch("frame_prep_kernel");
}
