// The MAGSAC++ gain of one point and its quantisation (ransac_score.hip), written once for the device and the host.  Plain C++:
// tools/magsac_host_check.cpp compiles it on the CPU and pose.magsac_gain restates it in numpy.  fp64 throughout, no fast-math.
//
// Barath, Noskova, Ivashechkin, Matas: "MAGSAC++, a fast, reliable and accurate robust estimator" (CVPR 2020), the loss rho(r)
// marginalised over the noise scale, for n = 4 degrees of freedom and the 0.99 quantile k = 3.64 that OpenCV's two-view USAC
// uses.  With sigma = max_threshold / k, u = r2 / (2 sigma^2) and u_k = k^2 / 2 the incomplete gamma functions of half-integer
// order reduce to erf, erfc and exp:
//   gamma(5/2, u) = (3 sqrt(pi) / 4) erf(t) - t exp(-u) (3/2 + u),   Gamma(3/2, u) = (sqrt(pi) / 2) erfc(t) + t exp(-u),   t = sqrt(u)
//   N(u) = gamma(5/2, u) + u (Gamma(3/2, u) - G_k) = (3 sqrt(pi)/4) erf(t) - 1.5 t exp(-u) + (sqrt(pi)/2) u erfc(t) - u G_k
//   gain(u) = 1 - N(u) / g_k for u < u_k (r2 finite), 0 otherwise;   G_k = Gamma(3/2, u_k), g_k = gamma(5/2, u_k) = N(u_k)
// gain is 1 at 0, 0 at u_k, continuous and non-increasing in between (N' = Gamma(3/2, u) - G_k >= 0).  A point contributes
// q = llrint(gain * 2^32), an integer of [0, 2^32]; a model's quality is the int64 sum of q over its pair's points.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GIM_MS_HD __host__ __device__ inline
#else
#define GIM_MS_HD inline
#endif

constexpr double GIM_MS_K = 3.64;                          // the 0.99 quantile of chi(4)
constexpr double GIM_MS_UK = 3.64 * 3.64 / 2.0;            // u at r = k sigma
constexpr double GIM_MS_GK = 0.0036572608340910747;        // Gamma(3/2, u_k), upper incomplete
constexpr double GIM_MS_LK = 1.3012265540498873;           // gamma(5/2, u_k), lower incomplete
constexpr double GIM_MS_C_ERF = 1.3293403881791370;        // 3 sqrt(pi) / 4
constexpr double GIM_MS_C_ERFC = 0.88622692545275801;      // sqrt(pi) / 2
constexpr double GIM_MS_UNITS = 4294967296.0;              // 2^32 quantisation units per point

// r2 = scale * u: the squared residual at u = 1, 2 sigma^2 = max_thr2 / u_k
GIM_MS_HD double gim_ms_scale(double max_thr2) { return max_thr2 / GIM_MS_UK; }

GIM_MS_HD double gim_ms_gain(double u) {
    if (!(u >= 0.0 && u < GIM_MS_UK)) return 0.0;          // beyond k sigma, negative, NaN
    const double t = sqrt(u);
    const double n = GIM_MS_C_ERF * erf(t) - 1.5 * t * exp(-u) + GIM_MS_C_ERFC * u * erfc(t) - u * GIM_MS_GK;
    const double g = 1.0 - n / GIM_MS_LK;
    return g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
}

// the quantised gain of a squared residual (a NaN or infinite r2: 0)
GIM_MS_HD int64_t gim_ms_units(double r2, double scale) { return (int64_t)llrint(gim_ms_gain(r2 / scale) * GIM_MS_UNITS); }
