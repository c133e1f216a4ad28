// Feature bank of the gim_loftr engine (gfx950): indexed block copy between slabs of equally sized slots.
//
// LoFTR.extract() computes the backbone maps of an image once; LoFTR.match_features() matches them in any number of pairs
// (gim_amd/loftr/loftr.py, gim_amd/loftr/bank.py).  The maps live in slabs [slots][block_bytes]; the stages that read them
// (transformer, coarse matching, fused fine level) take contiguous [bs, h, w, C] batches.  One kernel moves whole slots both ways:
//   scatter  freshly extracted maps [m][block] -> bank slots dst_idx[i]          (src_idx == NULL)
//   gather   bank slots src_idx[p] -> the pair batch's contiguous buffer [P][block]   (dst_idx == NULL)
// The index arrays are read on the device: the host enqueues the launch without waiting for anything, and a captured graph whose
// static inputs are the gathered buffers replays unchanged when the indices change.
//
// Replaces (reference file:line): nothing of the reference's arithmetic -- networks/loftr/loftr.py:59-72 recomputes the backbone
// for both images of every pair; this is the data movement that lets the engine not do so.
#include "gim_common.h"

namespace {

// grid.y walks the blocks, grid.x the 16-byte pieces of one block (both grid-stride).  Four independent 16-byte loads are in flight
// per lane before the first store.  A block whose source or destination slot is out of range is skipped as a whole: nothing of it
// is read or written.  The slot indices of a block are uniform over the workgroup (scalar loads).
__global__ void __launch_bounds__(256) slot_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                        const int32_t* __restrict__ src_idx, const int32_t* __restrict__ dst_idx,
                                                        int n, int64_t vec_per_block, int src_slots, int dst_slots) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const int si = src_idx ? src_idx[i] : i;
        const int di = dst_idx ? dst_idx[i] : i;
        if ((unsigned)si >= (unsigned)src_slots || (unsigned)di >= (unsigned)dst_slots) continue;
        const uint4* __restrict__ s = src + (int64_t)si * vec_per_block;
        uint4* __restrict__ d = dst + (int64_t)di * vec_per_block;
        int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
        for (; v + 3 * step < vec_per_block; v += 4 * step) {
            const uint4 a0 = s[v], a1 = s[v + step], a2 = s[v + 2 * step], a3 = s[v + 3 * step];
            d[v] = a0;
            d[v + step] = a1;
            d[v + 2 * step] = a2;
            d[v + 3 * step] = a3;
        }
        for (; v < vec_per_block; v += step) d[v] = s[v];
    }
}

}  // namespace

extern "C" int gim_slot_copy(const void* src, void* dst, const int32_t* src_idx, const int32_t* dst_idx, int n, int64_t block_bytes,
                             int src_slots, int dst_slots, gim_stream_t stream) {
    GIM_REQUIRE(n >= 0 && src_slots >= 0 && dst_slots >= 0, "gim_slot_copy: n=%d src_slots=%d dst_slots=%d", n, src_slots, dst_slots);
    if (n == 0) return GIM_OK;
    GIM_REQUIRE(src && dst, "gim_slot_copy: NULL slab");
    GIM_REQUIRE(block_bytes > 0 && block_bytes % 16 == 0, "gim_slot_copy: block_bytes=%lld is not a positive multiple of 16", (long long)block_bytes);
    GIM_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "gim_slot_copy: slabs must be 16-byte aligned");
    // identity on a side: block i is slot i there
    GIM_REQUIRE(src_idx || n <= src_slots, "gim_slot_copy: identity source needs n=%d <= src_slots=%d", n, src_slots);
    GIM_REQUIRE(dst_idx || n <= dst_slots, "gim_slot_copy: identity destination needs n=%d <= dst_slots=%d", n, dst_slots);
    const int64_t vpb = block_bytes / 16;
    // grid from the total bytes: 4 KiB (one unrolled pass) per lane group of a block, at most ~4096 workgroups; the rest is strided
    int64_t gx = (vpb + 4 * 256 - 1) / (4 * 256);
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    int64_t gy = 4096 / gx;
    gy = gy < 1 ? 1 : (gy > n ? n : gy);
    hipLaunchKernelGGL(slot_copy_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (uint4*)dst,
                       src_idx, dst_idx, n, vpb, src_slots, dst_slots);
    return gim_check_launch("slot_copy_kernel");
}
