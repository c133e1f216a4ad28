// The least-squares refit as gim_amd/csrc/model_refit_solve.h computes it, on the CPU, as plain C++ (no HIP, no Python).
//
//     refit_host_check              a few embedded scenes of both kinds (a planar pair for the homography, a general pair for the
//                                   fundamental matrix; 300, 64 and 13 matches, a third of them replaced by uniform points).  Per
//                                   scene it prints, in %.17g:
//                                     "scene S kind K P"            then P lines "ax ay bx by"
//                                     "fit" and nine numbers        gim_mr_fit on the matches that follow the motion (pose.*_ge)
//                                     "start" and nine numbers      the model the loop starts from (the fit, perturbed)
//                                     "refit A C0 C1" nine numbers  gim_mr_refit, four rounds, threshold 1 pixel, from the model's mask
//                                     "mask" and P characters 0 / 1
//                                   and it checks what the contract promises (the counts equal to the masks', the final count not
//                                   below the first, h33 = 1 or unit norm, a skipped pair all zero, guard bytes untouched); the last
//                                   line is OK or FAIL.  tests/test_model_refit_cpu.py compares the numbers with pose.refit_ge.
//
// Meant to be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/refit_host_check.cpp -o refit_host_check
//     ./refit_host_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "model_refit_solve.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform() {   // xorshift64*, in [0, 1)
    state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

struct Scene {
    int kind;
    std::vector<double> a, b;
};

// a camera of focal length 500 turned by `angle` about y and moved by T; kind 0 looks at the plane z = 5 - 0.1 x + 0.2 y
Scene scene(int kind, int P, double angle) {
    Scene s;
    s.kind = kind;
    const double cs = cos(angle), sn = sin(angle), T[3] = {0.4, -0.1, 0.15}, f = 500.0, cx = 320.0, cy = 240.0;
    for (int k = 0; k < P; ++k) {
        const double ax = 20.0 + 600.0 * uniform(), ay = 20.0 + 440.0 * uniform();
        const double rx = (ax - cx) / f, ry = (ay - cy) / f;
        const double Z = kind == 0 ? 5.0 / (1.0 + 0.1 * rx - 0.2 * ry) : 3.0 + 6.0 * uniform();
        const double X = rx * Z, Y = ry * Z;
        const double X1 = cs * X + sn * Z + T[0], Y1 = Y + T[1], Z1 = -sn * X + cs * Z + T[2];
        double bx = f * X1 / Z1 + cx + 0.3 * (uniform() - 0.5), by = f * Y1 / Z1 + cy + 0.3 * (uniform() - 0.5);
        if (k % 3 == 2) bx = 640.0 * uniform(), by = 480.0 * uniform();
        s.a.push_back(ax), s.a.push_back(ay), s.b.push_back(bx), s.b.push_back(by);
    }
    return s;
}

int failures = 0;
void fail(const char* what) { printf("FAIL: %s\n", what), failures += 1; }

void print9(const char* head, const double* m) {
    printf("%s", head);
    for (int i = 0; i < 9; ++i) printf(" %.17g", m[i]);
    printf("\n");
}

void run(int index, const Scene& s) {
    const int P = (int)(s.a.size() / 2);
    printf("scene %d kind %d %d\n", index, s.kind, P);
    for (int k = 0; k < P; ++k) printf("%.17g %.17g %.17g %.17g\n", s.a[2 * k], s.a[2 * k + 1], s.b[2 * k], s.b[2 * k + 1]);
    // the fit on the two thirds that follow the motion
    std::vector<uint8_t> all(P, 1);
    int n = 0;
    for (int k = 0; k < P; ++k) all[k] = k % 3 != 2, n += all[k];
    double fit[9];
    const bool ok = s.kind == 0 ? gim_mr_fit<0>(s.a.data(), s.b.data(), P, all.data(), n, fit) : gim_mr_fit<1>(s.a.data(), s.b.data(), P, all.data(), n, fit);
    if (!ok) return fail("no fit on a proper scene");
    print9("fit", fit);
    double norm = 0.0;
    for (int i = 0; i < 9; ++i) norm += fit[i] * fit[i];
    if (s.kind == 0 ? fit[8] != 1.0 : !(fabs(sqrt(norm) - 1.0) <= 1e-15)) fail("the fit is not scaled as promised");
    // the loop, from the fit perturbed: four rounds at one pixel
    double start[9], out[9];
    for (int i = 0; i < 9; ++i) start[i] = fit[i] * (1.0 + 2e-3 * (uniform() - 0.5));
    print9("start", start);
    std::vector<uint8_t> mask(P + 2, 0xAB);                                            // a guard byte on either side
    int32_t counts[2];
    const int accepted = gim_mr_refit(s.kind, s.a.data(), s.b.data(), P, start, nullptr, 1.0, 4, out, mask.data() + 1, counts);
    printf("refit %d %d %d", accepted, counts[0], counts[1]);
    print9("", out);
    printf("mask ");
    int good = 0;
    for (int k = 0; k < P; ++k) putchar('0' + mask[1 + k]), good += mask[1 + k] == 1;
    printf("\n");
    if (mask[0] != 0xAB || mask[P + 1] != 0xAB) fail("a guard byte was written");
    if (good != counts[1] || counts[1] < counts[0] || accepted < 0 || accepted > 4) fail("counts, mask and accepted disagree");
    // a model that cannot be refitted: everything zero
    double bad[9] = {0.0, 0.0, 0.0, 0.0, NAN, 0.0, 0.0, 0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass, bad[4] = 0.0) {
        std::fill(mask.begin(), mask.end(), 0xAB);
        const int r = gim_mr_refit(s.kind, s.a.data(), s.b.data(), P, bad, nullptr, 1.0, 4, out, mask.data() + 1, counts);
        bool zero = r == -1 && counts[0] == 0 && counts[1] == 0 && mask[0] == 0xAB && mask[P + 1] == 0xAB;
        for (int i = 0; i < 9; ++i) zero = zero && out[i] == 0.0;
        for (int k = 0; k < P; ++k) zero = zero && mask[1 + k] == 0;
        if (!zero) fail("a skipped pair left something behind");
    }
}

}  // namespace

int main() {
    const int sizes[3] = {300, 64, 13};
    int index = 0;
    for (int kind = 0; kind < 2; ++kind)
        for (int j = 0; j < 3; ++j) run(index++, scene(kind, sizes[j], 0.08 + 0.04 * j));
    printf(failures == 0 ? "OK\n" : "FAIL\n");
    return failures == 0 ? 0 : 1;
}
