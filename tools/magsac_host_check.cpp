// The MAGSAC++ gain of gim_amd/csrc/magsac_loss.h on the CPU, as plain C++ (no HIP, no Python): the end points, the constants
// (N(u_k) must reproduce g_k), monotonicity on a grid, the refusals (negative, NaN, infinite, beyond k sigma), then one line per u
// of a fixed list with the gain (as hexadecimal bits and in decimal) and the quantised units at max_thr2 = 1;
// tests/test_magsac_cpu.py compares the lines with pose.magsac_gain / pose.magsac_units.  Meant to be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/magsac_host_check.cpp -o magsac_host_check
//     ./magsac_host_check
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "magsac_loss.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) printf("FAIL: %s\n", what), ++failures;
}

}  // namespace

int main() {
    expect(gim_ms_gain(0.0) == 1.0, "gain(0) == 1");
    expect(gim_ms_gain(GIM_MS_UK) == 0.0, "gain(u_k) == 0");
    expect(gim_ms_gain(1.1 * GIM_MS_UK) == 0.0, "gain beyond u_k == 0");
    expect(gim_ms_gain(-1.0) == 0.0, "gain(negative) == 0");
    expect(gim_ms_gain(std::numeric_limits<double>::quiet_NaN()) == 0.0, "gain(NaN) == 0");
    expect(gim_ms_gain(std::numeric_limits<double>::infinity()) == 0.0, "gain(inf) == 0");
    expect(gim_ms_units(0.0, gim_ms_scale(1.0)) == (int64_t)1 << 32, "units(0) == 2^32");
    expect(gim_ms_units(std::numeric_limits<double>::quiet_NaN(), gim_ms_scale(1.0)) == 0, "units(NaN) == 0");
    expect(gim_ms_units(std::numeric_limits<double>::infinity(), gim_ms_scale(1.0)) == 0, "units(inf) == 0");
    expect(gim_ms_units(1.0, gim_ms_scale(1.0)) == 0, "units at k sigma == 0");
    // g_k is N(u_k): the closed form at u_k, without the clamp
    {
        const double u = GIM_MS_UK, t = sqrt(u);
        const double n = GIM_MS_C_ERF * erf(t) - 1.5 * t * exp(-u) + GIM_MS_C_ERFC * u * erfc(t) - u * GIM_MS_GK;
        expect(fabs(n - GIM_MS_LK) <= 1e-15, "N(u_k) == g_k to 1e-15");
        expect(fabs(GIM_MS_C_ERFC * erfc(t) + t * exp(-u) - GIM_MS_GK) <= 1e-15, "Gamma(3/2, u_k) == G_k to 1e-15");
    }
    double prev = 1.0;
    for (int i = 0; i <= 20000; ++i) {
        const double g = gim_ms_gain(GIM_MS_UK * 1.05 * i / 20000.0);
        if (!(g >= 0.0 && g <= 1.0)) expect(false, "gain in [0, 1]");
        if (g > prev + 2e-15) expect(false, "gain non-increasing");      // rounding of the four terms: a few 1e-16
        prev = g;
        if (failures > 5) break;
    }
    const double us[] = {0.0,  1e-30, 1e-12, 1e-6,  1e-3,  0.01,   0.1,    0.25,          0.5,       1.0,
                         1.5,  2.0,   3.0,   4.0,   5.0,   6.0,    6.5,    6.62,          6.6247999, GIM_MS_UK,
                         6.63, 7.0,   100.0, 0.125, 0.375, 2.7182, 3.1415, 0.69314718056, 4.2,       5.9};
    const double scale = gim_ms_scale(1.0);
    for (double u : us) {
        const double g = gim_ms_gain(u);
        uint64_t bits;
        memcpy(&bits, &g, sizeof bits);
        printf("u %.17g gain %016" PRIx64 " %.17g units %" PRId64 "\n", u, bits, g, gim_ms_units(u * scale, scale));
    }
    printf(failures == 0 ? "OK\n" : "FAIL\n");
    return failures == 0 ? 0 : 1;
}
