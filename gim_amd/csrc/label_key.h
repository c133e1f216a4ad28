// The arithmetic of the video pseudo-label kernels (label_link.hip), written once for the device and the host: the pixel key of
// `link` (the reference's datasets/walk/walk.py:29 create_table), the key domain, the watermark test (video_preprocessor.py:516) and
// the rescale of a label row (video_preprocessor.py:549 / 552).  Plain C++: tools/label_key_host_check.cpp compiles it on the CPU and
// gim_amd/video_labels.py restates it in numpy.  Every result is a fixed sequence of separately rounded IEEE operations: no fused
// multiply-add (the pragmas below; build the host side with -ffp-contract=off), no fast-math.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GIM_LK_HD __host__ __device__ inline
#else
#define GIM_LK_HD inline
#endif
#if defined(__clang__)
#define GIM_LK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GIM_LK_NO_CONTRACT
#endif

constexpr int GIM_LABEL_MAX_KEY = 1 << 24;   // keys up to here are exact in fp32

// np.round(x) + np.round(y) * w in fp32: round half to even, one product, one sum
GIM_LK_HD float gim_label_key(float x, float y, int w) {
    GIM_LK_NO_CONTRACT
    const float ry = rintf(y) * (float)w;
    return rintf(x) + ry;
}

// the table slot of a key, or -1 when the key is not usable: finite and in [0, w * (h + 1)] (the upper end is the alias of a point
// whose x rounds to w in the last row).  Needs w * (h + 1) <= GIM_LABEL_MAX_KEY.  NaN fails both comparisons.
GIM_LK_HD int gim_label_slot(float key, int w, int h) {
    const float top = (float)(w * (h + 1));
    return (key >= 0.0f && key <= top) ? (int)key : -1;
}

// ~((k0 - k1).abs() < thr).min(dim=1): a match has moved unless BOTH fp32 differences are below thr (a NaN row has moved)
GIM_LK_HD bool gim_label_moved(float x0, float y0, float x1, float y1, float thr) {
    const float dx = x0 - x1, dy = y0 - y1;
    return !(fabsf(dx) < thr && fabsf(dy) < thr);
}

// (x * s + o) * vratio in fp64, three roundings, then to fp32
GIM_LK_HD float gim_label_rescale(float x, double s, double o, double vratio) {
    GIM_LK_NO_CONTRACT
    const double p = (double)x * s;
    const double q = p + o;
    return (float)(q * vratio);
}

// without an affine: the fp32 product with vratio rounded to fp32
GIM_LK_HD float gim_label_scale(float x, double vratio) { return x * (float)vratio; }
