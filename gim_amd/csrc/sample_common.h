// Device helpers that the per-pair kernels of RegressionMatcher.sample (gim_weighted_sample in sample.hip, gim_kde in dkm.hip) share
// with the batched sampler (sample_pairs.hip).  The batched path must return the per-pair path's rows bit for bit, so the key of the
// exponential clocks and the summation order of the KDE exist ONCE, here, and every kernel compiles the same expressions.
#pragma once
#include "gim_common.h"

__device__ __forceinline__ unsigned hash32(unsigned x) {  // murmur3 finaliser
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

// key of weight wi at hash index i: the bit pattern of wi / e_i, e_i ~ Exp(1) hashed from (seed, i); 0 where wi <= 0 (or NaN)
__device__ __forceinline__ unsigned ws_key(float wi, unsigned i, unsigned seed) {
    unsigned key = 0u;
    if (wi > 0.f) {
        const unsigned r = hash32(hash32(i ^ (seed * 0x9e3779b9u)) + seed);
        // 23 random bits + half an ulp: every value is exactly representable and strictly inside (0, 1)
        // ((r >> 8) + 0.5 needs 25 bits at the top end and rounds up to 1.0 -> e = 0 -> key = +inf)
        const float u = ((float)(r >> 9) + 0.5f) * (1.0f / 8388608.0f);
        const float e = -logf(u);
        // > 0: bit order = value order.  The floor keeps a subnormal weight drawable: wi / e rounds to 0 for wi = 1.4e-45 and
        // e > 2 (subnormals are kept, the division is IEEE), key 0 is never taken by the compaction, and a caller that counts
        // the weight as positive (balanced_sample: k = n_pos) would get an output whose tail was never written.  Floored keys
        // tie and go by ascending index like every tie
        key = max(__float_as_uint(wi / e), 1u);
    }
    return key;
}

__device__ __forceinline__ float4 round_half4(float4 v) {
    return make_float4((float)(_Float16)v.x, (float)(_Float16)v.y, (float)(_Float16)v.z, (float)(_Float16)v.w);
}

// kde (utils/kde.py:17-26) of the 64 query points of block `blk` among x [n,4]: density[i] = sum_j exp(-|x_i - x_j|^2 / (2 std^2)).
// One block (256 threads) = 64 query points; its 4 waves split the j range (chunks of 64 points, chunk c -> wave c % 4), each staging its
// chunk in its own LDS slice (wave-local: no block barrier in the loop), partial sums combined in a fixed order.  The first
// version ran 256 queries per block with the whole block walking all j: 79 blocks for 20 000 samples -- a quarter of the CUs,
// one wave per SIMD, 1.6 ms per call; exp via v_exp_f32 (relative error ~1e-6 on a sum of 20 000 terms).
// Returns the density of point blk * 64 + lane; it is meaningful in wave 0 for points below n.  Every thread of the block calls it.
__device__ __forceinline__ float kde_block(const float* __restrict__ x, int n, float inv2s2, int half, int blk, float4 (*tile)[64],
                                           float (*part)[64]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blk * 64 + lane;
    float4 xi = i < n ? *(const float4*)(x + (size_t)i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (half) xi = round_half4(xi);
    const float c = -inv2s2 * 1.4426950408889634f;      // exp(-d2 * inv2s2) = exp2(d2 * c)
    float acc = 0.f;
    for (int j0 = wv * 64; j0 < n; j0 += 256) {
        const int j = j0 + lane;
        float4 xj = j < n ? *(const float4*)(x + (size_t)j * 4) : make_float4(1e18f, 1e18f, 1e18f, 1e18f);
        if (half && j < n) xj = round_half4(xj);
        tile[wv][lane] = xj;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-local LDS hand-off
        const int m = min(64, n - j0);
#pragma unroll 8
        for (int k = 0; k < m; ++k) {
            const float4 v = tile[wv][k];
            const float dx = xi.x - v.x, dy = xi.y - v.y, dz = xi.z - v.z, dw = xi.w - v.w;
            acc += __builtin_amdgcn_exp2f(((dx * dx + dy * dy) + (dz * dz + dw * dw)) * c);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // all reads done before the slice is overwritten
    }
    part[wv][lane] = acc;
    __syncthreads();
    return (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}
