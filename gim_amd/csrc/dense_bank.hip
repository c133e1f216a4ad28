// Feature bank of the dense matchers (gim_dkm, gim_roma; gfx950): the two launches that let a pair list run from per-image state.
//
// DenseMatcher.extract() computes everything match_batch derives from ONE image (pyramid levels, projections, black masks); the state
// lives in slabs [slots][bytes per slot], one per tensor kind (gim_amd/dense_bank.py).  DenseMatcher.match_features() needs them as the
// contiguous [2B, ...] batches the decoder reads:
//   gim_dense_gather_pairs   every level of a pair batch in ONE launch: destination entry d of every level receives slot idx[d].  Called
//                            with (slots0 | slots1) for the query batch and with (slots1 | slots0) for the support batch -- the second
//                            call replaces the per-level torch.cat((a[half:], a[:half])) of `_decode`.
//   gim_dense_emit_pairs     the tail of adapters.HlocDenseMatcher.forward + the rescale of dense_sfm.match_dense_pair_list for B pairs in
//                            one launch: `mconf > 0`, pixel coordinates, un-pad, strict in-bounds test, sides switched back, rescale,
//                            rows compacted in input order (block scan, no atomics), count per pair.
//
// Replaces (reference file:line): hloc/matchers/dkm.py:95-150 (the tail, per pair, four boolean-mask compactions = four host syncs)
// and hloc/match_dense.py:242-243 (scale_keypoints); the gather replaces nothing of the reference's arithmetic -- the reference encodes
// both images of every pair again (networks/dkm/models/dkm.py:572-581).
#include "gim_common.h"

namespace {

constexpr int GATHER_CHUNK = 2048;   // 16-byte pieces per workgroup: two unrolled passes of 256 lanes x 4 loads

struct GatherTable {
    const uint4* slab[GIM_DENSE_MAX_LEVELS];
    uint4* dst[GIM_DENSE_MAX_LEVELS];
    int64_t pieces[GIM_DENSE_MAX_LEVELS];      // 16-byte pieces per slot
    int wg_prefix[GIM_DENSE_MAX_LEVELS + 1];   // workgroups (chunks of GATHER_CHUNK pieces) in front of each level
    int n_levels;
};

// grid.x walks the chunks of all levels (the level of a workgroup: the prefix entry its index falls under), grid.y the 2B destination
// entries.  Four independent 16-byte loads are in flight per lane before the first store.  The slot index is uniform over the workgroup
// (a scalar load); an index outside [0, n_slots) skips the block whole: nothing of it is read or written.
__global__ void __launch_bounds__(256) dense_gather_kernel(const GatherTable t, const int32_t* __restrict__ idx, int n_slots) {
    const int d = blockIdx.y;
    const int slot = idx[d];
    if ((unsigned)slot >= (unsigned)n_slots) return;
    int l = 0;
    while (l + 1 < t.n_levels && (int)blockIdx.x >= t.wg_prefix[l + 1]) ++l;
    const int64_t pieces = t.pieces[l];
    const uint4* __restrict__ s = t.slab[l] + (int64_t)slot * pieces;
    uint4* __restrict__ o = t.dst[l] + (int64_t)d * pieces;
    const int64_t lo = (int64_t)((int)blockIdx.x - t.wg_prefix[l]) * GATHER_CHUNK;
    const int64_t hi = lo + GATHER_CHUNK < pieces ? lo + GATHER_CHUNK : pieces;
    int64_t v = lo + threadIdx.x;
    for (; v + 3 * 256 < hi; v += 4 * 256) {
        const uint4 a0 = s[v], a1 = s[v + 256], a2 = s[v + 2 * 256], a3 = s[v + 3 * 256];
        o[v] = a0;
        o[v + 256] = a1;
        o[v + 2 * 256] = a2;
        o[v + 3 * 256] = a3;
    }
    for (; v < hi; v += 256) o[v] = s[v];
}

// One workgroup per pair.  Rows are walked in tiles of 256; a row's place in the output is the number of kept rows in front of it
// (ballot + popcount within a wave, wave totals through LDS, the running base carried in a register every lane holds), so the order
// is the input order whatever the scheduling.  fp32 throughout, the host path's operations in the host path's order; contraction is
// off so that no multiply-add pair is fused where the host rounds twice.
#pragma clang fp contract(off)
__global__ void __launch_bounds__(256) dense_emit_kernel(const float* __restrict__ sparse, const float* __restrict__ mconf,
                                                         const gim_dense_pair_geom* __restrict__ geom, float* __restrict__ kpts0,
                                                         float* __restrict__ kpts1, float* __restrict__ scores, int32_t* __restrict__ count,
                                                         int num, int rescale) {
    __shared__ int wave_n[4];
    const int b = blockIdx.x;
    const gim_dense_pair_geom g = geom[b];
    const float* __restrict__ m = sparse + (size_t)b * num * 4;
    const float* __restrict__ c = mconf + (size_t)b * num;
    float* __restrict__ o0 = kpts0 + (size_t)b * num * 2;
    float* __restrict__ o1 = kpts1 + (size_t)b * num * 2;
    float* __restrict__ os = scores + (size_t)b * num;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;
    for (int r0 = 0; r0 < num; r0 += 256) {
        const int r = r0 + threadIdx.x;
        bool keep = false;
        float ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f, sc = 0.f;
        if (r < num) {
            const float4 v = *(const float4*)(m + (size_t)r * 4);
            sc = c[r];
            // gim_dense_to_pixels, then minus the padding (adapters._unpad_and_mask)
            ax = g.wp0 * (v.x + 1.f) / 2.f - g.pl0;
            ay = g.hp0 * (v.y + 1.f) / 2.f - g.pt0;
            bx = g.wp1 * (v.z + 1.f) / 2.f - g.pl1;
            by = g.hp1 * (v.w + 1.f) / 2.f - g.pt1;
            keep = sc > 0.f && ax > 0.f && ay > 0.f && bx > 0.f && by > 0.f && ax <= g.ow0 - 1.f && bx <= g.ow1 - 1.f &&
                   ay <= g.oh0 - 1.f && by <= g.oh1 - 1.f;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_n[wv] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int n = wave_n[w];
            if (w < wv) off += n;
            total += n;
        }
        if (keep) {
            const int o = off + __popcll(bal & ((1ull << lane) - 1ull));
            // the model's second image is the caller's image0: keypoints0 <- (bx, by), keypoints1 <- (ax, ay)
            float k0x = bx, k0y = by, k1x = ax, k1y = ay;
            if (rescale) {   // match_dense_pair_list: (k + 0.5) * s - 0.5
                k0x = (k0x + 0.5f) * g.sx0 - 0.5f;
                k0y = (k0y + 0.5f) * g.sy0 - 0.5f;
                k1x = (k1x + 0.5f) * g.sx1 - 0.5f;
                k1y = (k1y + 0.5f) * g.sy1 - 0.5f;
            }
            *(float2*)(o0 + (size_t)o * 2) = make_float2(k0x, k0y);
            *(float2*)(o1 + (size_t)o * 2) = make_float2(k1x, k1y);
            os[o] = sc;
        }
        base += total;
        __syncthreads();   // wave_n is rewritten by the next tile
    }
    if (threadIdx.x == 0) count[b] = base;
}

}  // namespace

extern "C" int gim_dense_gather_pairs(const gim_dense_gather_args* a, const int32_t* idx, int n_entries, int n_slots, gim_stream_t stream) {
    GIM_REQUIRE(a != nullptr, "gim_dense_gather_pairs: NULL table");
    GIM_REQUIRE(a->n_levels >= 1 && a->n_levels <= GIM_DENSE_MAX_LEVELS, "gim_dense_gather_pairs: %d levels, 1..%d are built", a->n_levels,
                GIM_DENSE_MAX_LEVELS);
    GIM_REQUIRE(n_entries >= 0 && n_entries <= 65535 && n_slots >= 1, "gim_dense_gather_pairs: n_entries=%d n_slots=%d", n_entries, n_slots);
    if (n_entries == 0) return GIM_OK;
    GIM_REQUIRE(idx != nullptr, "gim_dense_gather_pairs: NULL index array");
    GatherTable t;
    t.n_levels = a->n_levels;
    int64_t wg = 0;
    for (int l = 0; l < GIM_DENSE_MAX_LEVELS; ++l) {
        t.wg_prefix[l] = (int)wg;
        if (l >= a->n_levels) {
            t.slab[l] = nullptr; t.dst[l] = nullptr; t.pieces[l] = 0;
            continue;
        }
        GIM_REQUIRE(a->slab[l] && a->dst[l], "gim_dense_gather_pairs: level %d: NULL slab or destination", l);
        GIM_REQUIRE(a->slot_bytes[l] > 0 && a->slot_bytes[l] % 16 == 0, "gim_dense_gather_pairs: level %d: %lld bytes per slot is not a positive multiple of 16",
                    l, (long long)a->slot_bytes[l]);
        GIM_REQUIRE((((uintptr_t)a->slab[l] | (uintptr_t)a->dst[l]) & 15) == 0, "gim_dense_gather_pairs: level %d: slab and destination must be 16-byte aligned", l);
        t.slab[l] = (const uint4*)a->slab[l];
        t.dst[l] = (uint4*)a->dst[l];
        t.pieces[l] = a->slot_bytes[l] / 16;
        wg += (t.pieces[l] + GATHER_CHUNK - 1) / GATHER_CHUNK;
        GIM_REQUIRE(wg <= 0x7fffffff, "gim_dense_gather_pairs: the levels need more than 2^31 workgroups");
    }
    t.wg_prefix[GIM_DENSE_MAX_LEVELS] = (int)wg;
    hipLaunchKernelGGL(dense_gather_kernel, dim3((unsigned)wg, (unsigned)n_entries), dim3(256), 0, (hipStream_t)stream, t, idx, n_slots);
    return gim_check_launch("dense_gather_kernel");
}

extern "C" int gim_dense_emit_pairs(const float* sparse, const float* mconf, const gim_dense_pair_geom* geom, float* kpts0, float* kpts1,
                                    float* scores, int32_t* count, int B, int num, int rescale, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && num >= 0 && (int64_t)B * num <= 0x7fffffff, "gim_dense_emit_pairs: B=%d num=%d", B, num);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(geom && count, "gim_dense_emit_pairs: NULL geometry table or count");
    GIM_REQUIRE(num == 0 || (sparse && mconf && kpts0 && kpts1 && scores), "gim_dense_emit_pairs: NULL rows");
    GIM_REQUIRE((((uintptr_t)sparse) & 15) == 0 && ((((uintptr_t)kpts0 | (uintptr_t)kpts1)) & 7) == 0 && (((uintptr_t)geom) & 3) == 0,
                "gim_dense_emit_pairs: sparse must be 16-byte, keypoints 8-byte aligned");
    hipLaunchKernelGGL(dense_emit_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, sparse, mconf, geom, kpts0, kpts1, scores,
                       count, num, rescale);
    return gim_check_launch("dense_emit_kernel");
}
