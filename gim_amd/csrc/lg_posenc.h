// The one statement of LightGlue's keypoint encoding (lightglue.py:21-33,47-61), shared by the per-pair kernel (lightglue.hip:
// lg_posenc_kernel) and the keypoint bank's insertion kernel (lg_bank.hip: lg_bank_put_kernel): a bank slot's encoding must be the
// bits the per-pair kernel writes for the same fp32 keypoint, size and Wr.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// frequency f of one keypoint: proj = Wr[f] . normalised keypoint; c = cos(proj), s = sin(proj).  kpt -> (x, y), (w, h) the image size
__device__ __forceinline__ void lg_posenc_freq(const float* __restrict__ kpt, float w, float h, const float* __restrict__ Wr, int f,
                                               float& c, float& s) {
    const float scale = fmaxf(w, h) / 2.f;
    const float x = (kpt[0] - w / 2.f) / scale;
    const float y = (kpt[1] - h / 2.f) / scale;
    const float p = x * Wr[f * 2 + 0] + y * Wr[f * 2 + 1];
    c = cosf(p);
    s = sinf(p);
}
