// csrc/frame_prep_math.h on the CPU: whole jobs of gim_frame_prep computed with the header's functions in the kernel's order on a fixed
// input set, printed as raw bytes in hex so that tests/test_frame_prep_cpu.py can compare them with gim_amd/frame_prep.py exactly.
// Plain C++ with its own main:
//     c++ -std=c++17 -O1 -ffp-contract=off -I gim_amd/csrc tools/frame_prep_host_check.cpp -o frame_prep_host_check
// (add -g -fsanitize=address,undefined for a sanitizer run of the header).
// Inputs: bytes of the generator x <- 1664525 x + 1013904223 (mod 2^32), byte = x >> 24, seeded per case with 1000 + case; the frame
// [H][W][3] first, then the class map [Hs][Ws] with byte % 7 as the class; classes 2 and 5 are excluded.
// Output per case: "case <i> <H> <W> <Hs> <Ws> <x0> <y0> <x1> <y1> <wn> <hn> <flags> <tw> <th> <kept>" and one line per output in the order
// u8, mask, mask8, rgb, gray, norm (every output is computed, whatever the flags: the flags only say whether rgb / gray are masked).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "frame_prep_math.h"

struct Case {
    int H, W, Hs, Ws, x0, y0, x1, y1, wn, hn, flags;
};

template <class T>
static void dump(const char* name, const std::vector<T>& v) {
    std::printf("%s ", name);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

int main() {
    const Case cases[] = {
        {40, 50, 40, 50, 3, 4, 40, 33, 16, 8, 127},      // 37 x 29 -> 16 x 8: fractional on both axes
        {40, 50, 20, 30, 0, 0, 32, 16, 16, 8, 63},       // integer factor, a smaller class map
        {24, 32, 48, 60, 0, 0, 32, 24, 32, 24, 127},     // identity, a larger class map
        {40, 50, 40, 50, 39, 33, 50, 40, 16, 8, 127},    // 11 x 7 -> 16 x 8: up-scaling, a box at the far borders
        {40, 50, 13, 17, 10, 0, 50, 7, 16, 8, 63},       // down in x, up in y
        {40, 50, 40, 50, 7, 9, 8, 10, 8, 8, 127},        // one pixel
        {64, 128, 64, 128, 0, 0, 128, 64, 8, 8, 127},    // factor 16 in x, 8 in y
    };
    int i = 0;
    for (const Case& c : cases) {
        uint32_t x = 1000u + (uint32_t)i;
        auto next = [&x]() { x = x * 1664525u + 1013904223u; return (uint8_t)(x >> 24); };
        std::vector<uint8_t> frame((size_t)c.H * c.W * 3), seg((size_t)c.Hs * c.Ws);
        for (auto& b : frame) b = next();
        for (auto& b : seg) b = next() % 7;
        uint8_t excl[256] = {};
        excl[2] = excl[5] = 1;
        const int wc = c.x1 - c.x0, hc = c.y1 - c.y0, wn = c.wn, hn = c.hn;
        std::vector<uint8_t> u8((size_t)hn * wn * 3), mask((size_t)hn * wn), mask8((size_t)(hn / 8) * (wn / 8));
        std::vector<float> rgb((size_t)3 * hn * wn), gray((size_t)hn * wn), norm((size_t)3 * hn * wn);
        long kept = 0;
        for (int oy = 0; oy < hn; ++oy)
            for (int ox = 0; ox < wn; ++ox) {
                int nx, ny;
                const int kx = gim_fp_span(ox, wc, wn, &nx), ky = gim_fp_span(oy, hc, hn, &ny);
                if (nx > GIM_FP_TAPS - 1 || ny > GIM_FP_TAPS - 1 || kx < 0 || ky < 0 || kx + nx > wc || ky + ny > hc) {
                    std::printf("span out of range in case %d\n", i);
                    return 1;
                }
                float v[3] = {0.0f, 0.0f, 0.0f};
                for (int iy = 0; iy < ny; ++iy) {
                    float t[3] = {0.0f, 0.0f, 0.0f};
                    for (int ix = 0; ix < nx; ++ix) {
                        const float w = gim_fp_weight(ox, kx + ix, wc, wn);
                        const uint8_t* s = &frame[((size_t)(c.y0 + ky + iy) * c.W + (c.x0 + kx + ix)) * 3];
                        for (int ch = 0; ch < 3; ++ch) t[ch] = gim_fp_acc(t[ch], w, (float)s[ch]);
                    }
                    const float wy = gim_fp_weight(oy, ky + iy, hc, hn);
                    for (int ch = 0; ch < 3; ++ch) v[ch] = gim_fp_acc(v[ch], wy, t[ch]);
                }
                const size_t px = (size_t)oy * wn + ox, plane = (size_t)hn * wn;
                uint8_t b[3];
                for (int ch = 0; ch < 3; ++ch) b[ch] = u8[px * 3 + ch] = gim_fp_round_u8(v[ch]);
                const int sx = gim_fp_mask_index(ox, c.x0, wc, wn, c.W, c.Ws), sy = gim_fp_mask_index(oy, c.y0, hc, hn, c.H, c.Hs);
                const uint8_t m = excl[seg[(size_t)sy * c.Ws + sx]] ? 0 : 1;
                kept += m;
                mask[px] = m;
                if (ox % 8 == 0 && oy % 8 == 0 && ox / 8 < wn / 8 && oy / 8 < hn / 8) mask8[(size_t)(oy / 8) * (wn / 8) + ox / 8] = m;
                const uint8_t mm = (c.flags & GIM_FP_MASKED) ? m : (uint8_t)1;
                for (int ch = 0; ch < 3; ++ch) {
                    rgb[ch * plane + px] = gim_fp_unit((uint8_t)(b[ch] * mm));
                    norm[ch * plane + px] = gim_fp_norm(b[ch], ch);
                }
                gray[px] = gim_fp_unit((uint8_t)(gim_fp_gray(b[0], b[1], b[2]) * mm));
            }
        int tw = GIM_FP_TILE_W, th = GIM_FP_TILE_H;
        while (gim_fp_tile_bytes(tw, th, wc, wn, hc, hn) > GIM_FP_LDS_BYTES && (tw > 1 || th > 1)) {
            if (th > 1) th >>= 1;
            else tw >>= 1;
        }
        std::printf("case %d %d %d %d %d %d %d %d %d %d %d %d %d %d %ld\n", i, c.H, c.W, c.Hs, c.Ws, c.x0, c.y0, c.x1, c.y1, wn, hn, c.flags, tw, th, kept);
        dump("u8", u8);
        dump("mask", mask);
        dump("mask8", mask8);
        dump("rgb", rgb);
        dump("gray", gray);
        dump("norm", norm);
        ++i;
    }
    std::printf("OK\n");
    return 0;
}
