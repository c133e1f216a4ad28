// The arithmetic of the frame-preparation kernel (frame_prep.hip), written once for the device and the host: the coverage weights of
// the area resize, the nearest-neighbour chain of the class mask (the reference's video_preprocessor.py:342-354), OpenCV's 8-bit
// BT.601 grey, and the fp32 conversions of the matchers' and the segmenter's inputs (:418-493, :603-621).  Plain C++:
// tools/frame_prep_host_check.cpp compiles it on the CPU and gim_amd/frame_prep.py restates it in numpy.  Every result is a fixed
// sequence of separately rounded IEEE operations: no fused multiply-add (the pragmas below; build the host side with
// -ffp-contract=off), no fast-math.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GIM_FP_HD __host__ __device__ inline
#else
#define GIM_FP_HD inline
#endif
#if defined(__clang__)
#define GIM_FP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GIM_FP_NO_CONTRACT
#endif

constexpr int GIM_FP_MAX_FACTOR = 16;              // the largest source / destination extent ratio per axis
constexpr int GIM_FP_TAPS = GIM_FP_MAX_FACTOR + 2; // source pixels under one destination pixel: at most factor + 1; one spare
constexpr int GIM_FP_TILE_W = 64, GIM_FP_TILE_H = 16;   // the largest output tile of a workgroup; jobs with large factors take smaller ones
constexpr int GIM_FP_LDS_BYTES = 40960;            // the staged source footprint of a tile
constexpr int GIM_FP_JOB_WORDS = 16;               // int64 words per job, the indices below
enum {
    GIM_FP_SLOT = 0, GIM_FP_X0, GIM_FP_Y0, GIM_FP_X1, GIM_FP_Y1, GIM_FP_WN, GIM_FP_HN, GIM_FP_FLAGS,
    GIM_FP_OFF_U8, GIM_FP_OFF_MASK, GIM_FP_OFF_MASK8, GIM_FP_OFF_RGB, GIM_FP_OFF_GRAY, GIM_FP_OFF_NORM, GIM_FP_TW, GIM_FP_TH
};
enum {
    GIM_FP_OUT_U8 = 1, GIM_FP_OUT_MASK = 2, GIM_FP_OUT_MASK8 = 4, GIM_FP_OUT_RGB = 8, GIM_FP_OUT_GRAY = 16, GIM_FP_OUT_NORM = 32,
    GIM_FP_MASKED = 64, GIM_FP_ALL_FLAGS = 127
};

// destination index d of m over a source extent n covers [a, b) = [d * s, min((d + 1) * s, n)), s = n / m in double.
// -> the first source index floor(a); *count = ceil(b) - floor(a)
GIM_FP_HD int gim_fp_span(int d, int n, int m, int* count) {
    GIM_FP_NO_CONTRACT
    const double s = (double)n / (double)m;
    const double a = (double)d * s;
    const double b = fmin((double)(d + 1) * s, (double)n);
    const int k0 = (int)floor(a);
    *count = (int)ceil(b) - k0;
    return k0;
}

// the weight of source index k under destination index d: (min(b, k + 1) - max(a, k)) / (b - a) in double, rounded once to fp32
GIM_FP_HD float gim_fp_weight(int d, int k, int n, int m) {
    GIM_FP_NO_CONTRACT
    const double s = (double)n / (double)m;
    const double a = (double)d * s;
    const double b = fmin((double)(d + 1) * s, (double)n);
    const double hi = fmin(b, (double)(k + 1));
    const double lo = fmax(a, (double)k);
    const double len = b - a;
    return (float)((hi - lo) / len);
}

// one more term of a weighted sum: the product and the sum are rounded separately
GIM_FP_HD float gim_fp_acc(float acc, float w, float v) {
    GIM_FP_NO_CONTRACT
    const float p = w * v;
    return acc + p;
}

GIM_FP_HD uint8_t gim_fp_round_u8(float v) {
    const float r = rintf(v);
    return (uint8_t)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

// the class-map index under output index j: resize to the frame, crop, resize to the output, each INTER_NEAREST with integer floors
//   c = lo + min(j * nc / nn, nc - 1);  s = min(c * ns / nf, ns - 1)
GIM_FP_HD int gim_fp_mask_index(int j, int lo, int nc, int nn, int nf, int ns) {
    int64_t c = (int64_t)j * nc / nn;
    c = lo + (c < nc - 1 ? c : nc - 1);
    const int64_t s = c * ns / nf;
    return (int)(s < ns - 1 ? s : ns - 1);
}

// cv2.cvtColor(RGB2GRAY) on bytes
GIM_FP_HD uint8_t gim_fp_gray(uint8_t r, uint8_t g, uint8_t b) { return (uint8_t)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14); }

GIM_FP_HD float gim_fp_unit(uint8_t v) { return (float)v / 255.0f; }

// ((float)v / 255 - mean) / std, the ImageNet constants of channel c
GIM_FP_HD float gim_fp_norm(uint8_t v, int c) {
    GIM_FP_NO_CONTRACT
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
    const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    const float u = (float)v / 255.0f;
    return (u - mean) / sd;
}

// the bytes of LDS a tile of tw x th output pixels may need for its source footprint at these extents: rows of (columns * 3 bytes +
// up to 15 bytes in front of an unaligned row start), rounded up to 16
GIM_FP_HD int64_t gim_fp_tile_bytes(int tw, int th, int wc, int wn, int hc, int hn) {
    GIM_FP_NO_CONTRACT
    const double sx = (double)wc / (double)wn, sy = (double)hc / (double)hn;
    const int64_t cols = (int64_t)ceil((double)tw * sx) + 2, rows = (int64_t)ceil((double)th * sy) + 2;
    return rows * (((cols * 3 + 15 + 15) / 16) * 16);
}
