// Glue kernels of the semantic segmenter (networks/mit_semseg: ResnetDilated + PPMDeepsup, models.py:208-268, 438-495) for gfx950.
// The convolutions run on conv_igemm.hip (dilated 3x3s through the K-group table, gim_amd/packing.py::pack_conv(dilation=));
// what is left is pyramid pooling and the inference head, all plain vector work (no MFMA, no scratch).  Maps are NHWC rows.
//
//   ppm_pool              nn.AdaptiveAvgPool2d(s) for s = 1, 2, 3, 6 of conv5 in one launch        models.py:446-451, 472-477
//   ppm_upsample_concat   F.interpolate(bilinear, align_corners=False) of the four branch outputs to h8 x w8, written straight
//                         into channels c_off.. of the concat buffer conv_last reads (no torch.cat)  models.py:471-478
//   seg_head_argmax       F.interpolate(logits, segSize) + softmax + torch.max(dim=1) per output pixel; the full-resolution
//                         150-channel tensor is never written: a tile's logits rows sit in LDS        models.py:482-486, hloc/utils:42-49
#include <cmath>
#include "gim_common.h"

namespace {

inline unsigned nblocks(size_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

constexpr int PPM_BINS = 50;   // 1 + 4 + 9 + 36

// bin q of the concatenated pyramid -> (scale s, row i, column j); bins of scale s start at offsets 0, 1, 5, 14
__device__ __forceinline__ void ppm_bin(int q, int& s, int& i, int& j) {
    int off;
    if (q < 1) { s = 1; off = 0; } else if (q < 5) { s = 2; off = 1; } else if (q < 14) { s = 3; off = 5; } else { s = 6; off = 14; }
    i = (q - off) / s;
    j = (q - off) - i * s;
}

// ---- adaptive average pooling to the four pyramid scales ---------------------------------------------------------------------
// grid (50 bins, B, C / 64); 1024 threads = 16 four-channel groups x 64 pixel phases (the scale-1 bin is the whole map: its C / 64
// workgroups carry a quarter of all loads, so each gets 16 waves).  Bin i of s spans [floor(i H / s),
// ceil((i + 1) H / s)) (PyTorch's adaptive pooling rule; bins overlap when H < s).  Phase partial sums + a tree over the phases.
template <bool BF16>
__global__ void __launch_bounds__(1024) ppm_pool_kernel(const void* __restrict__ x, float* __restrict__ out, int H, int W, int C, int ldx) {
    constexpr int NPH = 64;
    __shared__ float4 red[NPH][16];
    const int b = blockIdx.y, cg = threadIdx.x & 15, ph = threadIdx.x >> 4;
    const int c = blockIdx.z * 64 + cg * 4;
    int s, i, j;
    ppm_bin(blockIdx.x, s, i, j);
    const int y0 = (i * H) / s, y1 = ((i + 1) * H + s - 1) / s;
    const int x0 = (j * W) / s, x1 = ((j + 1) * W + s - 1) / s;
    const int bw = x1 - x0, n = (y1 - y0) * bw;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
        for (int p = ph; p < n; p += NPH) {
            const int yy = y0 + p / bw, xx = x0 + p % bw;
            const float4 v = ElemIO<BF16>::ld4(x, (((size_t)b * H + yy) * W + xx) * ldx + c);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    red[ph][cg] = acc;
    __syncthreads();
#pragma unroll
    for (int h = NPH / 2; h >= 1; h >>= 1) {
        if (ph < h) {
            const float4 o = red[ph + h][cg];
            float4 m = red[ph][cg];
            m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
            red[ph][cg] = m;
        }
        __syncthreads();
    }
    if (ph == 0 && c < C) {
        const float4 m = red[0][cg];
        const float inv = (float)n;
        *(float4*)(out + ((size_t)b * PPM_BINS + blockIdx.x) * C + c) = make_float4(m.x / inv, m.y / inv, m.z / inv, m.w / inv);
    }
}

// PyTorch's bilinear source coordinate (align_corners=False): src = max(0, (dst + 0.5) * in / out - 0.5), index = (int)src,
// neighbour = index + 1 unless on the last row / column, weight of the neighbour = src - index (upsample_bilinear2d)
struct Lerp { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lerp lerp_src(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Lerp r;
    r.i0 = min((int)src, in - 1);
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// ---- the four branch outputs upsampled into the concat buffer --------------------------------------------------------------------
// br [B][50][Cb] fp32 (bins in ppm_bin order, after 1x1 conv + BN + ReLU); y rows [B*h*w][ldy] of the activation dtype, channels
// c_off + si * Cb + c.  One thread per (pixel, scale, 4 channels).
template <bool BF16>
__global__ void ppm_upsample_concat_kernel(const float* __restrict__ br, void* __restrict__ y, int B, int h, int w, int Cb4, int ldy, int c_off) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * h * w * 4 * Cb4) return;
    const int c = (int)(idx % Cb4) * 4;
    const int si = (int)((idx / Cb4) % 4);
    const size_t pix = idx / ((size_t)Cb4 * 4);
    const int xo = (int)(pix % w), yo = (int)((pix / w) % h), b = (int)(pix / ((size_t)w * h));
    const int s = si == 0 ? 1 : si == 1 ? 2 : si == 2 ? 3 : 6;
    const int off = si == 0 ? 0 : si == 1 ? 1 : si == 2 ? 5 : 14;
    const Lerp ly = lerp_src(yo, s, h), lx = lerp_src(xo, s, w);
    const int Cb = Cb4 * 4;
    const float* base = br + ((size_t)b * PPM_BINS + off) * Cb + c;
    const float4 v00 = *(const float4*)(base + (size_t)(ly.i0 * s + lx.i0) * Cb), v01 = *(const float4*)(base + (size_t)(ly.i0 * s + lx.i1) * Cb);
    const float4 v10 = *(const float4*)(base + (size_t)(ly.i1 * s + lx.i0) * Cb), v11 = *(const float4*)(base + (size_t)(ly.i1 * s + lx.i1) * Cb);
    auto bl = [&](float a00, float a01, float a10, float a11) {
        return ly.l0 * (lx.l0 * a00 + lx.l1 * a01) + ly.l1 * (lx.l0 * a10 + lx.l1 * a11);
    };
    ElemIO<BF16>::st4(y, pix * ldy + c_off + si * Cb + c,
                      make_float4(bl(v00.x, v01.x, v10.x, v11.x), bl(v00.y, v01.y, v10.y, v11.y), bl(v00.z, v01.z, v10.z, v11.z),
                                  bl(v00.w, v01.w, v10.w, v11.w)));
}

// ---- inference head: bilinear upsampling of the logits + arg-max (+ max softmax probability) --------------------------------------
// grid (ceil(W / TX), ceil(H / TY), B), 256 threads; output pixel (ty, tx) of the TY x TX tile = thread ty * TX + tx (TY * TX <= 256).
// The source rows / columns the tile touches (<= RS x CS, host bound) are staged in LDS as [row][col][C] fp32; every thread then
// interpolates all C classes of its pixel from LDS.  Softmax is monotone: the class is the arg-max of the interpolated logits
// (strict '>': the lowest index wins a tie, as torch.max); the probability is 1 / sum_c exp(v_c - max) (online log-sum-exp).
// `flag` (NULL: no check): OR 1 when a staged logit is not finite.
__global__ void __launch_bounds__(256) seg_head_kernel(const float* __restrict__ lg, uint8_t* __restrict__ cls, float* __restrict__ prob,
                                                       int* __restrict__ flag, int h, int w, int C, int ld, int H, int W, int TY, int TX,
                                                       int RS, int CS) {
    extern __shared__ float tile[];
    const int b = blockIdx.z, oy0 = blockIdx.y * TY, ox0 = blockIdx.x * TX;
    const int oy1 = min(oy0 + TY, H) - 1, ox1 = min(ox0 + TX, W) - 1;
    const int r0 = lerp_src(oy0, h, H).i0, c0 = lerp_src(ox0, w, W).i0;
    const int nr = min(min(lerp_src(oy1, h, H).i1 - r0 + 1, RS), h - r0);
    const int nc = min(min(lerp_src(ox1, w, W).i1 - c0 + 1, CS), w - c0);
    const int per = nc * C;
    bool bad = false;
    for (int e = threadIdx.x; e < nr * per; e += 256) {
        const int r = e / per, rem = e - r * per, cc = rem / C, k = rem - cc * C;
        const float v = lg[(((size_t)b * h + r0 + r) * w + c0 + cc) * ld + k];
        bad |= !isfinite(v);
        tile[(r * CS + cc) * C + k] = v;
    }
    if (__syncthreads_or(bad) && flag != nullptr && threadIdx.x == 0) atomicOr(flag, 1);
    const int ty = threadIdx.x / TX, tx = threadIdx.x - ty * TX;
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (ty >= TY || oy >= H || ox >= W) return;
    const Lerp ly = lerp_src(oy, h, H), lx = lerp_src(ox, w, W);
    const int ra = max(0, min(ly.i0 - r0, nr - 1)), rb = max(0, min(ly.i1 - r0, nr - 1));
    const int ca = max(0, min(lx.i0 - c0, nc - 1)), cb = max(0, min(lx.i1 - c0, nc - 1));
    const float* p00 = tile + (ra * CS + ca) * C;
    const float* p01 = tile + (ra * CS + cb) * C;
    const float* p10 = tile + (rb * CS + ca) * C;
    const float* p11 = tile + (rb * CS + cb) * C;
    float m = -INFINITY, sum = 0.f;
    int best = 0;
    for (int k = 0; k < C; ++k) {
        const float v = ly.l0 * (lx.l0 * p00[k] + lx.l1 * p01[k]) + ly.l1 * (lx.l0 * p10[k] + lx.l1 * p11[k]);
        if (v > m) {
            sum = (k == 0 ? 0.f : sum * __expf(m - v)) + 1.f;
            m = v;
            best = k;
        } else {
            sum += __expf(v - m);
        }
    }
    const size_t o = ((size_t)b * H + oy) * W + ox;
    cls[o] = (uint8_t)best;
    if (prob) prob[o] = 1.f / sum;
}

}  // namespace

#define DISPATCH_BF(KERN, bf, grid, ...)                                                                  \
    do {                                                                                                  \
        if (bf) hipLaunchKernelGGL(KERN<true>, grid, dim3(256), 0, s, __VA_ARGS__);                     \
        else hipLaunchKernelGGL(KERN<false>, grid, dim3(256), 0, s, __VA_ARGS__);                       \
    } while (0)

GIM_TWIN(gim_ppm_pool)
extern "C" int GIM_FN(gim_ppm_pool)(const void* x, float* out, int B, int H, int W, int C, int ldx, int dtype, gim_stream_t stream) {
    GIM_ROUTE_ANY(dtype, gim_ppm_pool, x, out, B, H, W, C, ldx, dtype, stream);
    GIM_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0, "ppm_pool: bad args");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(PPM_BINS, B, (C + 63) / 64);
    if (dtype == GIM_H16) hipLaunchKernelGGL(ppm_pool_kernel<true>, grid, dim3(1024), 0, s, x, out, H, W, C, ldx);
    else hipLaunchKernelGGL(ppm_pool_kernel<false>, grid, dim3(1024), 0, s, x, out, H, W, C, ldx);
    return gim_check_launch("ppm_pool");
}

GIM_TWIN(gim_ppm_upsample_concat)
extern "C" int GIM_FN(gim_ppm_upsample_concat)(const float* br, void* y, int B, int h, int w, int Cb, int ldy, int c_off, int dtype,
                                               gim_stream_t stream) {
    GIM_ROUTE_ANY(dtype, gim_ppm_upsample_concat, br, y, B, h, w, Cb, ldy, c_off, dtype, stream);
    GIM_REQUIRE(br && y && B > 0 && h > 0 && w > 0 && Cb > 0 && Cb % 4 == 0 && c_off >= 0 && c_off % 4 == 0 && ldy % 4 == 0 &&
                c_off + 4 * Cb <= ldy, "ppm_upsample_concat: bad args");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nblocks((size_t)B * h * w * Cb, 256));
    DISPATCH_BF(ppm_upsample_concat_kernel, dtype == GIM_H16, grid, br, y, B, h, w, Cb / 4, ldy, c_off);
    return gim_check_launch("ppm_upsample_concat");
}

// tile of the head kernel: the first of 4 x 64 .. 1 x 1 pixels whose staged source window fits 64 KiB of LDS.  Window bound per
// axis: floor((T - 1) * in / out) + 3 (one more than the exact span, for the fp32 rounding of the source coordinates)
static int head_window(int T, int in, int out) { return std::min(in, (int)(((long long)(T - 1) * in) / out) + 3); }

extern "C" int GIM_FN(gim_seg_head_argmax)(const float* logits, uint8_t* cls, float* prob, int* flag, int B, int h, int w, int C, int ld,
                                           int H, int W, gim_stream_t stream) {
    GIM_REQUIRE(logits && cls && B > 0 && h > 0 && w > 0 && C > 0 && C <= 256 && ld >= C && H > 0 && W > 0 && B <= 65535,
                "seg_head_argmax: bad args (C <= 256 classes for a uint8 map)");
    static const int cand[][2] = {{4, 64}, {2, 64}, {1, 64}, {1, 32}, {1, 16}, {1, 8}, {1, 4}, {1, 2}, {1, 1}};
    int TY = 0, TX = 0, RS = 0, CS = 0;
    for (const auto& t : cand) {
        const int rs = head_window(t[0], h, H), cs = head_window(t[1], w, W);
        if ((long long)rs * cs * C * 4 <= 65536) { TY = t[0]; TX = t[1]; RS = rs; CS = cs; break; }
    }
    GIM_REQUIRE(TY > 0, "seg_head_argmax: %d classes do not fit one LDS window", C);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TX - 1) / TX, (H + TY - 1) / TY, B);
    GIM_REQUIRE(grid.y <= 65535, "seg_head_argmax: H too large");
    hipLaunchKernelGGL(seg_head_kernel, grid, dim3(256), (size_t)RS * CS * C * 4, s, logits, cls, prob, flag, h, w, C, ld, H, W, TY, TX, RS, CS);
    return gim_check_launch("seg_head_argmax");
}
