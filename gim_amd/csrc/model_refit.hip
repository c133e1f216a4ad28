// Least-squares refit of a homography or a fundamental matrix on its inliers, and up to eight rounds of refit / re-score local
// optimisation, in one launch for a batch of pairs (gfx950).  fp64 throughout, no fast-math flag on this file, no atomics.
//
// The points are those the RANSAC step kernels already hold on the device (csrc/homography.hip, csrc/fundamental.hip); after the
// RANSAC a pair's refit costs this launch and one copy of the model, the mask and the counts.
//
// Replaces (reference file:line): the re-fit on the inliers inside cv2.findHomography(..., USAC_MAGSAC, ...) of demo.py:197-217 and
// the local optimisation / least-squares polish inside cv2.findFundamentalMat(..., USAC_MAGSAC, ...) of demo.py:514-517 and
// datasets/walk/walk.py:295, as far as they are the published normalised DLT and normalised eight-point algorithms
// (HomographyEstimatorCallback::runKernel and run8Point of OpenCV's modules/calib3d/src/fundam.cpp: A^T A and its eigenvectors).
// MAGSAC's scoring and findHomography's Levenberg-Marquardt polish are not built.  pose.refit_ge is the arithmetic of this file in
// numpy, pose.homography_dlt the host's restatement with LAPACK's SVD.
//
// Arithmetic (the contract of include/gim_hip.h, csrc/model_refit_solve.h): every sum over a pair's inliers has one fixed order
// (block_sum below), so a pair's result depends neither on B nor on its place in the batch.  The divisions and square roots are
// IEEE; the compiler may contract a*b+c into an FMA where numpy rounds twice.
#include "gim_common.h"
#include "model_refit_solve.h"

namespace {

constexpr int MR_THREADS = GIM_MR_LANES;
constexpr int MR_WAVES = MR_THREADS / 64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));   // one point: a 16-byte load

struct mr_shared {
    double red[MR_WAVES][GIM_MR_TRI];   // one row of partial sums per wave
    double tri[GIM_MR_TRI];             // the summed upper triangle of A^T A
    double a[81], v[81];                // the Jacobi iteration's matrix and eigenvectors (lane 0)
    double cur[9], cand[9];             // the current model and the round's candidate
    int cnt[MR_WAVES][2];
    int ok;
};

// The fixed summation order: every lane brings the sum of its own points (l, l + 256, ... ascending); the 64 lanes of a wave are
// combined by the shuffle tree x[l] += x[l + o], o = 32 .. 1, whose lane 0 holds the wave's total; every lane then adds the four
// wave totals in wave order from LDS, so all lanes hold the same bits.  Two barriers; sh.red is free again on return.
template <int K>
__device__ __forceinline__ void block_sum(double (&x)[K], mr_shared& sh, int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x[k] += __shfl_down(x[k], o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh.red[tid >> 6][k] = x[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = ((sh.red[0][k] + sh.red[1][k]) + sh.red[2][k]) + sh.red[3][k];
    __syncthreads();
}

// two integer sums over the workgroup, the same result on every lane
__device__ __forceinline__ void block_count(int& c0, int& c1, mr_shared& sh, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c0 += __shfl_down(c0, o, 64), c1 += __shfl_down(c1, o, 64);
    if ((tid & 63) == 0) sh.cnt[tid >> 6][0] = c0, sh.cnt[tid >> 6][1] = c1;
    __syncthreads();
    c0 = (sh.cnt[0][0] + sh.cnt[1][0]) + (sh.cnt[2][0] + sh.cnt[3][0]);
    c1 = (sh.cnt[0][1] + sh.cnt[1][1]) + (sh.cnt[2][1] + sh.cnt[3][1]);
    __syncthreads();
}

// grid = pairs: one workgroup owns one pair.  A lane owns the points tid, tid + 256, ... of the pair and their bytes of mask_out,
// which hold the current mask in bit 0 throughout (and the candidate's in bit 1 between a round's re-scoring and its decision):
// no lane reads a byte another lane wrote.  Every branch that leaves the loop is taken on a value all lanes hold alike: the result
// of a block_sum / block_count, or a word lane 0 left in LDS before a barrier.
template <int KIND>
__global__ void __launch_bounds__(MR_THREADS) model_refit_kernel(const f64x2_t* __restrict__ pa, const f64x2_t* __restrict__ pb,
                                                                 const int32_t* __restrict__ offsets, const double* __restrict__ models_in,
                                                                 const uint8_t* __restrict__ mask_in, double thr2, int rounds,
                                                                 double* __restrict__ models_out, uint8_t* __restrict__ mask_out,
                                                                 int32_t* __restrict__ counts, int32_t* __restrict__ accepted) {
    __shared__ mr_shared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int base = offsets[b];
    const int n_pts = offsets[b + 1] - base;                  // workgroup-uniform
    if (tid == 0) {
        double m[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = models_in[(int64_t)b * 9 + i];
        sh.ok = gim_mr_model_ok(m) ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) sh.cur[i] = m[i];
    }
    __syncthreads();
    if (sh.ok == 0) {                                         // a skipped pair: everything zero
        for (int p = tid; p < n_pts; p += MR_THREADS) mask_out[(int64_t)base + p] = 0;
        if (tid < 9) models_out[(int64_t)b * 9 + tid] = 0.0;
        if (tid < 2) counts[(int64_t)b * 2 + tid] = 0;
        if (tid == 0) accepted[b] = -1;
        return;
    }
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = sh.cur[i];
    // the starting mask: the caller's, or the model's own under thr2
    int n = 0, unused = 0;
    for (int p = tid; p < n_pts; p += MR_THREADS) {
        const int64_t i = (int64_t)base + p;
        int in;
        if (mask_in != nullptr) {
            in = mask_in[i] != 0 ? 1 : 0;
        } else {
            const f64x2_t a = pa[i], d = pb[i];
            in = gim_tv_inlier(KIND, M, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
        }
        mask_out[i] = (uint8_t)in;
        n += in;
    }
    block_count(n, unused, sh, tid);
    const int n_start = n;
    int acc_rounds = 0;
    for (int r = 0; r < rounds; ++r) {
        if (n < gim_mr_min_points(KIND)) break;
        // step 1 and the first reduction of step 2: the coordinate sums, and how many inlier coordinates are not finite
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        int bad = 0, zero = 0;
        for (int p = tid; p < n_pts; p += MR_THREADS) {
            const int64_t i = (int64_t)base + p;
            if (mask_out[i] != 0) {
                const f64x2_t a = pa[i], d = pb[i];
                bad += (gim_mr_finite(a.x) && gim_mr_finite(a.y) && gim_mr_finite(d.x) && gim_mr_finite(d.y)) ? 0 : 1;
                s4[0] += a.x, s4[1] += a.y, s4[2] += d.x, s4[3] += d.y;
            }
        }
        block_count(bad, zero, sh, tid);
        if (bad != 0) break;
        block_sum<4>(s4, sh, tid);
        gim_mr_norm N;
        gim_mr_centres(s4, n, &N);
        double d2[2] = {0.0, 0.0};
        for (int p = tid; p < n_pts; p += MR_THREADS) {
            const int64_t i = (int64_t)base + p;
            if (mask_out[i] != 0) {
                const f64x2_t a = pa[i], d = pb[i];
                double dd[2];
                gim_mr_dist(N, a.x, a.y, d.x, d.y, dd);
                d2[0] += dd[0], d2[1] += dd[1];
            }
        }
        block_sum<2>(d2, sh, tid);
        if (!gim_mr_scales(d2, n, &N)) break;
        // step 3
        double tri[GIM_MR_TRI];
#pragma unroll
        for (int k = 0; k < GIM_MR_TRI; ++k) tri[k] = 0.0;
        for (int p = tid; p < n_pts; p += MR_THREADS) {
            const int64_t i = (int64_t)base + p;
            if (mask_out[i] != 0) {
                const f64x2_t a = pa[i], d = pb[i];
                gim_mr_accumulate<KIND>(N, a.x, a.y, d.x, d.y, tri);
            }
        }
        block_sum<GIM_MR_TRI>(tri, sh, tid);
        // steps 4 to 6 on one lane; the verdict and the candidate reach the others through LDS
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < GIM_MR_TRI; ++k) sh.tri[k] = tri[k];
            double c[9];
            const bool good = gim_mr_solve(KIND, sh.tri, N, sh.a, sh.v, c);
#pragma unroll
            for (int i = 0; i < 9; ++i) sh.cand[i] = c[i];
            sh.ok = good ? 1 : 0;
        }
        __syncthreads();
        const int good = sh.ok;
        double C[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) C[i] = sh.cand[i];
        __syncthreads();                                      // sh.ok and sh.cand are read before the next round writes them
        if (good == 0) break;
        // step 7
        int nc = 0, ndiff = 0;
        for (int p = tid; p < n_pts; p += MR_THREADS) {
            const int64_t i = (int64_t)base + p;
            const f64x2_t a = pa[i], d = pb[i];
            const int in = gim_tv_inlier(KIND, C, a.x, a.y, d.x, d.y, thr2) ? 1 : 0;
            const int was = mask_out[i];
            mask_out[i] = (uint8_t)(was | (in << 1));
            nc += in, ndiff += in != was ? 1 : 0;
        }
        block_count(nc, ndiff, sh, tid);
        const bool take = nc >= n;
        for (int p = tid; p < n_pts; p += MR_THREADS) {       // the bytes this lane wrote above
            const int64_t i = (int64_t)base + p;
            const int both = mask_out[i];
            mask_out[i] = (uint8_t)(take ? (both >> 1) : (both & 1));
        }
        if (!take) break;
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = C[i];
        n = nc, ++acc_rounds;
        if (ndiff == 0) break;                                // a fixed point
    }
    if (tid < 9) {
        double out = M[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) out = tid == i ? M[i] : out;
        models_out[(int64_t)b * 9 + tid] = out;
    }
    if (tid == 0) {
        counts[(int64_t)b * 2] = n_start, counts[(int64_t)b * 2 + 1] = n;
        accepted[b] = acc_rounds;
    }
}

}  // namespace

extern "C" int gim_model_refit(int kind, const double* a, const double* b, const int32_t* offsets, int B, const double* models_in,
                               const uint8_t* mask_in, double thr2, int rounds, double* models_out, uint8_t* mask_out, int32_t* counts,
                               int32_t* accepted, gim_stream_t stream) {
    GIM_REQUIRE(kind == 0 || kind == 1, "gim_model_refit: kind=%d (0: homography, 1: fundamental)", kind);
    GIM_REQUIRE(rounds >= 1 && rounds <= GIM_MR_MAX_ROUNDS, "gim_model_refit: rounds=%d (1 <= rounds <= 8)", rounds);
    GIM_REQUIRE(B >= 0 && B <= 65535, "gim_model_refit: B=%d (0 <= B <= 65535)", B);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(a && b && offsets && models_in && models_out && mask_out && counts && accepted, "gim_model_refit: NULL pointer");
    GIM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "gim_model_refit: a and b must be 16-byte aligned");
    GIM_REQUIRE((((uintptr_t)models_in | (uintptr_t)models_out) & 7) == 0 && (((uintptr_t)offsets | (uintptr_t)counts | (uintptr_t)accepted) & 3) == 0,
                "gim_model_refit: misaligned models_in, models_out, offsets, counts or accepted");
    if (kind == 0)
        hipLaunchKernelGGL(model_refit_kernel<0>, dim3((unsigned)B), dim3(MR_THREADS), 0, (hipStream_t)stream, (const f64x2_t*)a,
                           (const f64x2_t*)b, offsets, models_in, mask_in, thr2, rounds, models_out, mask_out, counts, accepted);
    else
        hipLaunchKernelGGL(model_refit_kernel<1>, dim3((unsigned)B), dim3(MR_THREADS), 0, (hipStream_t)stream, (const f64x2_t*)a,
                           (const f64x2_t*)b, offsets, models_in, mask_in, thr2, rounds, models_out, mask_out, counts, accepted);
    return gim_check_launch("model_refit_kernel");
}
