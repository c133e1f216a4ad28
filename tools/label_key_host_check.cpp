// csrc/label_key.h on the CPU: the keys, table slots, watermark tests and rescaled coordinates of a fixed input set, printed as bit
// patterns so that tests/test_label_link_cpu.py can compare them with numpy exactly.  Plain C++ with its own main:
//     c++ -std=c++17 -O1 -ffp-contract=off -I gim_amd/csrc tools/label_key_host_check.cpp -o label_key_host_check
// (add -g -fsanitize=address,undefined for a sanitizer run of the header).
// Output, one record per line:
//     K <x bits> <y bits> <w> <h> <key bits> <slot>
//     M <x0 bits> <y0 bits> <x1 bits> <y1 bits> <thr bits> <moved 0|1>
//     R <x bits> <s bits64> <o bits64> <vratio bits64> <rescaled bits> <scaled bits>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "label_key.h"

static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}
static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int frames[][2] = {{96, 54}, {1920, 1080}, {1, 1}, {4096, 4095}};
    const float xs[] = {0.0f, 0.5f, 1.5f, 2.5f, -0.5f, -0.4f, -0.6f, 95.5f, 95.49f, 96.2f, 1919.5f, 1918.5f, 7.25f, 3e38f, inf, -inf, nan, 16777216.0f};
    const float ys[] = {0.0f, 0.5f, 1.5f, 53.5f, 54.0f, 54.5f, 55.0f, 1079.5f, 1080.0f, 1081.0f, -1.0f, 4095.0f, 4096.0f, 3e38f, inf, nan};
    for (const auto& f : frames)
        for (float x : xs)
            for (float y : ys) {
                const float key = gim_label_key(x, y, f[0]);
                std::printf("K %08" PRIx32 " %08" PRIx32 " %d %d %08" PRIx32 " %d\n", bits(x), bits(y), f[0], f[1], bits(key),
                            gim_label_slot(key, f[0], f[1]));
            }
    const float ds[] = {0.0f, 0.25f, 0.99999994f, 1.0f, 1.0000001f, -1.0f, -0.5f, 3.5f, nan, inf};
    const float thrs[] = {1.0f, 0.5f};
    for (float thr : thrs)
        for (float dx : ds)
            for (float dy : ds) {
                const float x0 = 100.25f, y0 = 40.5f, x1 = x0 + dx, y1 = y0 - dy;
                std::printf("M %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d\n", bits(x0), bits(y0), bits(x1), bits(y1),
                            bits(thr), (int)gim_label_moved(x0, y0, x1, y1, thr));
            }
    const double ss[] = {1920.0 / 1333.0, 1080.0 / 750.0, 1.0, 0.1, 1e-3};
    const double os[] = {0.0, 12.0, -3.25, 0.1, 1e9};
    const double vs[] = {720.0 / 1080.0, 1.0, 0.3, 2.0 / 3.0};
    const float cs[] = {0.0f, 0.1f, 1332.7f, 749.3f, 666.66669f, 1e-3f, -5.5f, 3e38f, nan};
    for (double s : ss)
        for (double o : os)
            for (double v : vs)
                for (float c : cs)
                    std::printf("R %08" PRIx32 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %08" PRIx32 " %08" PRIx32 "\n", bits(c), bits(s), bits(o),
                                bits(v), bits(gim_label_rescale(c, s, o, v)), bits(gim_label_scale(c, v)));
    return 0;
}
