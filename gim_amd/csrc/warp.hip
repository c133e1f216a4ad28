// Perspective warp of an image batch (gfx950): what cv2.warpPerspective(img1, H, size of img0) does at the end of the reference's demo
// (wrap_images, demo.py:230-266), with exact bilinear weights.
//
// dst(x, y) = bilinear(src, (u, v)),  (u, v) = proj(H^-1 (x, y, 1)),  integer pixel centres, channels-first [B][C][H][W], C <= 4.
// The inverse is the adjugate of H, computed once per workgroup in fp64 and used WITHOUT the division by det(H): the projection does not
// see a common factor, and a tiny determinant cannot overflow it.  (u, v) in fp64; the four bilinear weights are formed in fp64 and
// rounded ONCE to fp32; the blend is four fp32 products and three additions.  A neighbour outside the source contributes 0
// (BORDER_CONSTANT 0 blended in, as cv2 does), so the result is a continuous function of (u, v): a last-bit difference in u cannot
// jump a value.  w == 0, a coordinate that is not finite or a footprint wholly outside the source gives 0.  The uint8 flavour stores
// rint (to nearest even) of the fp32 value, saturated to [0, 255].
// Stated difference from cv2: its INTER_LINEAR quantises the weights to 5 fractional bits (INTER_BITS) and blends in fixed point; this is
// the exact-weight operator, tested against its own formula (tests/homography_oracle.py), not against cv2's bytes.
#include "gim_common.h"

namespace {

constexpr int WP_BX = 64, WP_BY = 4;   // a workgroup covers 64 x 4 destination pixels: a wave writes one row segment (coalesced)

template <typename T> __device__ __forceinline__ float wp_load(const T* p) { return (float)*p; }
__device__ __forceinline__ void wp_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void wp_store(uint8_t* p, float v) {
    const float r = rintf(v);
    *p = (uint8_t)(r <= 0.0f ? 0.0f : (r >= 255.0f ? 255.0f : r));   // finite: uint8 pixels under weights in [0, 1]
}

// grid = (ceil(Wd / 64), ceil(Hd / 4), B).  One thread per destination pixel computes the coordinate once and then all C channels.
template <typename T>
__global__ void __launch_bounds__(WP_BX * WP_BY) warp_perspective_kernel(const T* __restrict__ src, int C, int Hs, int Ws,
                                                                         const double* __restrict__ Hmat, T* __restrict__ dst, int Hd,
                                                                         int Wd) {
    __shared__ double sInv[9];
    const int b = blockIdx.z;
    const int t = threadIdx.y * WP_BX + threadIdx.x;
    if (t < 9) {                                              // adjugate entry (r, c) = cofactor (c, r)
        const double* h = Hmat + (int64_t)b * 9;
        const int r = t / 3, c = t % 3;
        const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
        sInv[t] = h[r1 * 3 + c1] * h[r2 * 3 + c2] - h[r1 * 3 + c2] * h[r2 * 3 + c1];
    }
    __syncthreads();
    const int x = blockIdx.x * WP_BX + threadIdx.x, y = blockIdx.y * WP_BY + threadIdx.y;
    if (x >= Wd || y >= Hd) return;
    const double X = (double)x, Y = (double)y;
    const double w = sInv[6] * X + sInv[7] * Y + sInv[8];
    const double u = (sInv[0] * X + sInv[1] * Y + sInv[2]) / w;
    const double v = (sInv[3] * X + sInv[4] * Y + sInv[5]) / w;
    const int64_t plane_s = (int64_t)Hs * Ws, plane_d = (int64_t)Hd * Wd;
    T* out = dst + (int64_t)b * C * plane_d + (int64_t)y * Wd + x;
    // the footprint [floor(u), floor(u) + 1] x [floor(v), floor(v) + 1] meets the source iff -1 < u < Ws and -1 < v < Hs (NaN, and the
    // infinities of w == 0, fail the comparisons)
    if (!(w != 0.0 && u > -1.0 && u < (double)Ws && v > -1.0 && v < (double)Hs)) {
        for (int c = 0; c < C; ++c) wp_store(out + c * plane_d, 0.0f);
        return;
    }
    const double fu = floor(u), fv = floor(v);
    const int x0 = (int)fu, y0 = (int)fv;                     // in [-1, Ws - 1] x [-1, Hs - 1]
    const double ax = u - fu, ay = v - fv;
    const float w00 = (float)((1.0 - ax) * (1.0 - ay)), w01 = (float)(ax * (1.0 - ay));
    const float w10 = (float)((1.0 - ax) * ay), w11 = (float)(ax * ay);
    const bool xl = x0 >= 0, xr = x0 + 1 < Ws, yt = y0 >= 0, yb = y0 + 1 < Hs;
    const T* in = src + (int64_t)b * C * plane_s + (int64_t)y0 * Ws + x0;
    for (int c = 0; c < C; ++c) {
        const T* p = in + c * plane_s;
        const float p00 = (xl && yt) ? wp_load(p) : 0.0f;
        const float p01 = (xr && yt) ? wp_load(p + 1) : 0.0f;
        const float p10 = (xl && yb) ? wp_load(p + Ws) : 0.0f;
        const float p11 = (xr && yb) ? wp_load(p + Ws + 1) : 0.0f;
        wp_store(out + c * plane_d, ((w00 * p00 + w01 * p01) + w10 * p10) + w11 * p11);
    }
}

}  // namespace

extern "C" int gim_warp_perspective(const void* src, int dtype, int B, int C, int Hs, int Ws, const double* Hmat, void* dst, int Hd, int Wd,
                                    gim_stream_t stream) {
    GIM_REQUIRE(dtype == 0 || dtype == 1, "gim_warp_perspective: dtype tag %d (0 = uint8, 1 = fp32: pixel kinds, not the GIM_F32 / GIM_BF16 / GIM_F16 tags)", dtype);
    GIM_REQUIRE(B >= 0 && B <= 65535 && C >= 1 && C <= 4, "gim_warp_perspective: B=%d C=%d (0 <= B <= 65535, 1 <= C <= 4)", B, C);
    GIM_REQUIRE(Hs >= 1 && Ws >= 1 && Hd >= 0 && Wd >= 0, "gim_warp_perspective: source %dx%d, destination %dx%d", Hs, Ws, Hd, Wd);
    if (B == 0 || Hd == 0 || Wd == 0) return GIM_OK;
    GIM_REQUIRE((int64_t)Hs * Ws <= 0x7fffffffLL && (int64_t)Hd * Wd <= 0x7fffffffLL && (Hd + WP_BY - 1) / WP_BY <= 65535,
                "gim_warp_perspective: image too large (%dx%d -> %dx%d)", Hs, Ws, Hd, Wd);
    GIM_REQUIRE(src && Hmat && dst, "gim_warp_perspective: NULL pointer");
    GIM_REQUIRE((((uintptr_t)Hmat) & 7) == 0 && (dtype == 0 || (((uintptr_t)src | (uintptr_t)dst) & 3) == 0), "gim_warp_perspective: misaligned pointer");
    const dim3 grid((unsigned)((Wd + WP_BX - 1) / WP_BX), (unsigned)((Hd + WP_BY - 1) / WP_BY), (unsigned)B), block(WP_BX, WP_BY);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL(warp_perspective_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)src, C, Hs, Ws, Hmat, (uint8_t*)dst, Hd, Wd);
    else
        hipLaunchKernelGGL(warp_perspective_kernel<float>, grid, block, 0, st, (const float*)src, C, Hs, Ws, Hmat, (float*)dst, Hd, Wd);
    return gim_check_launch("warp_perspective_kernel");
}
