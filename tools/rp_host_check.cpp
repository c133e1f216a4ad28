// recoverPose as gim_amd/csrc/recover_pose_solve.h computes it, on the CPU, as plain C++ (no HIP, no Python).
//
//     rp_host_check                 a few seeded two-view scenes plus the degenerate inputs the tests plant; every result is checked
//                                   for what the contract promises (R orthogonal with det +1, |t| = 1, the counts equal to the
//                                   mask's, the winner the first maximum, an invalid E all zero); a checksum is printed
//     rp_host_check FILE            the problems of FILE, one after the other; per problem a line "B best n0 n1 n2 n3", a line with
//                                   R (9) and t (3) in %.17g, and a line with the mask as 0 / 1 characters ("-" for no points).
//                                   FILE: per problem "P has_mask distance_thresh", the nine entries of E, then P lines
//                                   "x0 y0 x1 y1 [mask]" (tests/test_recover_pose_cpu.py writes it and compares with pose.recover_pose_ge)
//
// Meant to be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/rp_host_check.cpp -o rp_host_check
//     ./rp_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "recover_pose_solve.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform() {   // xorshift64*, in [0, 1)
    state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

struct Problem {
    double E[9], dthr = 1e9;
    std::vector<double> x0, x1;
    std::vector<uint8_t> mask;
    bool has_mask = false;
};

struct Result {
    double R[9], t[3];
    int32_t n[4];
    int best;
    std::vector<uint8_t> mask;
};

Result solve(const Problem& p) {
    Result r;
    const int P = (int)(p.x0.size() / 2);
    r.mask.assign(P + 1, 0xAB);                                                       // one guard byte behind the pair
    r.best = gim_rp_recover(p.E, p.x0.data(), p.x1.data(), P, p.has_mask ? p.mask.data() : nullptr, p.dthr, r.R, r.t, r.n, r.mask.data());
    return r;
}

// a turn of `angle` about y with a step T; half of the second view replaced by uniform points
Problem scene(int P, double angle, const double* T, double outliers) {
    Problem p;
    const double cs = cos(angle), sn = sin(angle);
    const double R[9] = {cs, 0.0, sn, 0.0, 1.0, 0.0, -sn, 0.0, cs};
    const double K[9] = {0.0, -T[2], T[1], T[2], 0.0, -T[0], -T[1], T[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) p.E[3 * i + j] = K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j] + K[3 * i + 2] * R[6 + j];
    for (int k = 0; k < P; ++k) {
        const double X = -2.0 + 4.0 * uniform(), Y = -1.5 + 3.0 * uniform(), Z = 2.0 + 8.0 * uniform();
        const double X1 = cs * X + sn * Z + T[0], Y1 = Y + T[1], Z1 = -sn * X + cs * Z + T[2];
        p.x0.push_back(X / Z + 5e-4 * (uniform() - 0.5)), p.x0.push_back(Y / Z + 5e-4 * (uniform() - 0.5));
        if (uniform() < outliers) p.x1.push_back(-1.0 + 2.0 * uniform()), p.x1.push_back(-1.0 + 2.0 * uniform());
        else p.x1.push_back(X1 / Z1), p.x1.push_back(Y1 / Z1);
    }
    return p;
}

int failures = 0;
double worst_orth = 0.0, sum = 0.0;

void fail(const char* what) { printf("FAIL: %s\n", what), failures += 1; }

void check(const Problem& p, const Result& r, bool expect_valid) {
    const int P = (int)(p.x0.size() / 2);
    if (r.mask[P] != 0xAB) fail("the byte behind the pair was written");
    int good = 0;
    for (int k = 0; k < P; ++k) {
        if (r.mask[k] > 1) fail("a mask byte is neither 0 nor 1");
        if (p.has_mask && !p.mask[k] && r.mask[k]) fail("a masked point is good");
        good += r.mask[k];
    }
    if (!expect_valid) {
        bool zero = r.best == -1 && good == 0;
        for (int i = 0; i < 9; ++i) zero = zero && r.R[i] == 0.0;
        for (int i = 0; i < 3; ++i) zero = zero && r.t[i] == 0.0;
        for (int j = 0; j < 4; ++j) zero = zero && r.n[j] == 0;
        if (!zero) fail("an invalid E left something behind");
        return;
    }
    if (r.best < 0 || r.best > 3 || r.best != gim_rp_best(r.n[0], r.n[1], r.n[2], r.n[3])) fail("best is not the first maximum");
    else if (good != r.n[r.best]) fail("the mask does not add up to the winner's count");
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += r.R[3 * k + i] * r.R[3 * k + j];
            d = fabs(d - (i == j ? 1.0 : 0.0));
            if (!(d <= worst_orth)) worst_orth = d;
        }
    const double det = r.R[0] * (r.R[4] * r.R[8] - r.R[5] * r.R[7]) - r.R[1] * (r.R[3] * r.R[8] - r.R[5] * r.R[6]) +
                       r.R[2] * (r.R[3] * r.R[7] - r.R[4] * r.R[6]);
    const double tn = sqrt(r.t[0] * r.t[0] + r.t[1] * r.t[1] + r.t[2] * r.t[2]);
    if (!(fabs(det - 1.0) <= 1e-12)) fail("det R != 1");
    if (!(fabs(tn - 1.0) <= 1e-12)) fail("|t| != 1");
    for (int i = 0; i < 9; ++i) sum += fabs(r.R[i]) * (double)(1 + i);
    for (int j = 0; j < 4; ++j) sum += (double)r.n[j];
}

int self_check() {
    const double T[3][3] = {{0.5, 0.1, 0.05}, {-0.2, 0.9, 0.1}, {0.05, -0.1, 1.0}};
    int scenes = 0, most = 0;
    for (int s = 0; s < 6; ++s) {
        Problem p = scene(s == 5 ? 0 : 1 + 211 * s, 0.05 + 0.05 * s, T[s % 3], 0.5);
        Result r = solve(p);
        check(p, r, true);
        if (r.best >= 0 && r.n[r.best] > most) most = r.n[r.best];
        p.has_mask = true;
        for (size_t k = 0; k < p.x0.size() / 2; ++k) p.mask.push_back(uniform() < 0.7 ? 1 : 0);
        check(p, solve(p), true);
        p.dthr = 5.0;
        check(p, solve(p), true);
        for (double& e : p.E) e *= -1e-6;                                             // the same pose set
        check(p, solve(p), true);
        scenes += 4;
    }
    Problem bad = scene(65, 0.1, T[0], 0.5);
    memset(bad.E, 0, sizeof bad.E);
    check(bad, solve(bad), false);
    bad.E[4] = NAN;
    check(bad, solve(bad), false);
    bad.E[4] = INFINITY;
    check(bad, solve(bad), false);
    memset(bad.E, 0, sizeof bad.E);
    bad.E[1] = 1.0;                                                                   // rank one: still four proper candidates
    check(bad, solve(bad), true);
    printf("%d scene runs, 4 degenerate; most good points %d; largest |R^T R - I| %.3e\n", scenes, most, worst_orth);
    printf("checksum %.12e\n", sum);
    const bool pass = failures == 0 && most > 400 && worst_orth <= 1e-14;
    printf(pass ? "OK\n" : "FAIL\n");
    return pass ? 0 : 1;
}

int run_file(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("cannot open %s\n", path), 2;
    int P, has_mask, b = 0;
    double dthr;
    while (fscanf(f, "%d %d %lf", &P, &has_mask, &dthr) == 3) {
        if (P < 0 || P > (1 << 24)) return fclose(f), printf("bad point count %d\n", P), 2;
        Problem p;
        p.dthr = dthr, p.has_mask = has_mask != 0;
        for (double& e : p.E) {
            char word[64];
            if (fscanf(f, "%63s", word) != 1) return fclose(f), printf("short file\n"), 2;
            e = strcmp(word, "nan") == 0 ? NAN : strtod(word, nullptr);
        }
        for (int k = 0; k < P; ++k) {
            double v[4];
            int m = 1;
            if (fscanf(f, "%lf %lf %lf %lf", v, v + 1, v + 2, v + 3) != 4 || (p.has_mask && fscanf(f, "%d", &m) != 1))
                return fclose(f), printf("short file\n"), 2;
            p.x0.push_back(v[0]), p.x0.push_back(v[1]), p.x1.push_back(v[2]), p.x1.push_back(v[3]);
            p.mask.push_back((uint8_t)(m != 0));
        }
        const Result r = solve(p);
        printf("%d %d %d %d %d %d\n", b++, r.best, r.n[0], r.n[1], r.n[2], r.n[3]);
        for (int i = 0; i < 9; ++i) printf("%.17g ", r.R[i]);
        printf("%.17g %.17g %.17g\n", r.t[0], r.t[1], r.t[2]);
        if (P == 0) printf("-");
        for (int k = 0; k < P; ++k) putchar('0' + r.mask[k]);
        printf("\n");
    }
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) { return argc > 1 ? run_file(argv[1]) : self_check(); }
