// Keypoint bank of the gim_lightglue engine (gfx950): SuperPoint features of an image are stored once and matched in any number of
// pairs (gim_amd/lightglue/bank.py, gim_amd/lightglue/pairs.py) -- the sparse counterpart of feature_bank.hip.
//
// Replaces (reference file:line): nothing of the reference's arithmetic.  hloc/match_features.py:124-160, 244-255 reads both images'
// features from disk for every pair, uploads them, and the matcher recomputes both positional encodings (lightglue.py:414-430); an
// exhaustive list over n images names every image n - 1 times.  Here an image costs one insertion, and a batch of pairs one gather.
//
// Bank layout, `slots` images of K keypoints (all arrays dense, slot-major):
//   kpts [slots][K][2]    fp32   (x, y) as the detector returned them
//   desc [slots][K][256]  fp32 or IEEE fp16 (the storage dtype; hloc's feature files are fp16 already)
//   enc  [slots][K][64]   fp32   cos | sin table of lg_posenc for the image's size and the matcher's Wr: a function of the image alone
//
//   lg_bank_put      rows of n images -> their slots (descriptor rounding to the storage dtype, keypoints, encoding)
//   lg_gather_pairs  slots idx0[b], idx1[b] of B pairs -> the stacked [2 B K] row block LightGlue.forward builds per call: the fp32
//                    residual stream, its compute-dtype copy (CAT[:, :256]) and the encoding table, image-0 rows first
//   lg_emit_hloc     an lg_assign result -> hloc's match-file datasets (matches0 int16, matching_scores0 fp16) for the whole batch
// Every kernel gives a keypoint row to 32 lanes (8 descriptor elements each: 16-byte loads and stores throughout); slot indices are
// read on the device and a row whose slot is out of range is not read.
#include "gim_common.h"
#include "lg_posenc.h"

namespace {

inline unsigned nblocks(size_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

typedef long long gim_i64x2_t __attribute__((ext_vector_type(2)));

// desc == NULL: descriptors untouched; bank_kpts == NULL: keypoints untouched; Wr == NULL: encoding untouched
template <bool ST16>
__global__ void __launch_bounds__(256) lg_bank_put_kernel(const float* __restrict__ kpts, const float* __restrict__ desc,
                                                          const float* __restrict__ size_wh, const float* __restrict__ Wr,
                                                          const int32_t* __restrict__ slots, float* __restrict__ bank_kpts,
                                                          void* __restrict__ bank_desc, float* __restrict__ bank_enc, int n, int K,
                                                          int n_slots) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * K * 32) return;
    const int c = (int)(idx & 31);
    const size_t r = idx >> 5;
    const int i = (int)(r / K), k = (int)(r % K);
    const int slot = slots[i];
    if ((unsigned)slot >= (unsigned)n_slots) return;
    const size_t dr = (size_t)slot * K + k;
    if (desc != nullptr) {
        const float4 a = *(const float4*)(desc + r * 256 + c * 8), b = *(const float4*)(desc + r * 256 + c * 8 + 4);
        if (ST16) {
            *(uint4*)((unsigned short*)bank_desc + dr * 256 + c * 8) =
                make_uint4(cvt_pk_f16(a.x, a.y), cvt_pk_f16(a.z, a.w), cvt_pk_f16(b.x, b.y), cvt_pk_f16(b.z, b.w));
        } else {
            float* d = (float*)bank_desc + dr * 256 + c * 8;
            *(float4*)d = a;
            *(float4*)(d + 4) = b;
        }
    }
    if (bank_kpts != nullptr && c == 0) *(float2*)(bank_kpts + dr * 2) = *(const float2*)(kpts + r * 2);
    if (Wr != nullptr) {
        float cs, sn;
        lg_posenc_freq(kpts + r * 2, size_wh[i * 2 + 0], size_wh[i * 2 + 1], Wr, c, cs, sn);
        bank_enc[dr * 64 + c] = cs;
        bank_enc[dr * 64 + 32 + c] = sn;
    }
}

// cat_kind: 0 = no 16-bit copy (fp32 compute: x32 IS CAT[:, :256]), GIM_BF16 / GIM_F16 = the copy's kind (wave-uniform).
// A pair whose slot is out of range gets zero rows.
template <bool ST16>
__global__ void __launch_bounds__(256) lg_gather_pairs_kernel(const void* __restrict__ bank_desc, const float* __restrict__ bank_enc,
                                                              const int32_t* __restrict__ idx0, const int32_t* __restrict__ idx1,
                                                              float* __restrict__ x32, void* __restrict__ cat, float* __restrict__ enc,
                                                              int B, int K, int n_slots, int cat_kind, int ld_x32, int ld_cat,
                                                              const int32_t* __restrict__ counts, int32_t* __restrict__ len0,
                                                              int32_t* __restrict__ len1) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t half = (size_t)B * K;
    if (idx >= 2 * half * 32) return;
    const int c = (int)(idx & 31);
    const size_t r = idx >> 5;
    const bool side1 = r >= half;
    const size_t rr = side1 ? r - half : r;
    const int b = (int)(rr / K), k = (int)(rr % K);
    const int slot = side1 ? idx1[b] : idx0[b];
    bool ok = (unsigned)slot < (unsigned)n_slots;
    if (counts != nullptr) {   // ragged bank: the image has counts[slot] keypoints; what the slab holds behind them is never read
        const int n = ok ? min(max(counts[slot], 0), K) : 0;
        if (k == 0 && c == 0) (side1 ? len1 : len0)[b] = n;
        ok = ok && k < n;
    }
    const size_t sr = (size_t)(ok ? slot : 0) * K + k;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (ok) {
        if (ST16) {
            const uint4 u = *(const uint4*)((const unsigned short*)bank_desc + sr * 256 + c * 8);
            lo = make_float4(f16_lo(u.x), f16_hi(u.x), f16_lo(u.y), f16_hi(u.y));
            hi = make_float4(f16_lo(u.z), f16_hi(u.z), f16_lo(u.w), f16_hi(u.w));
        } else {
            const float* s = (const float*)bank_desc + sr * 256 + c * 8;
            lo = *(const float4*)s;
            hi = *(const float4*)(s + 4);
        }
    }
    float* xo = x32 + r * ld_x32 + c * 8;
    *(float4*)xo = lo;
    *(float4*)(xo + 4) = hi;
    if (cat_kind != 0) {   // the rounding of cast_rows on the same fp32 values
        const bool bf = cat_kind == GIM_BF16;
        *(uint4*)((unsigned short*)cat + r * ld_cat + c * 8) =
            make_uint4(cvt_pk_16(lo.x, lo.y, bf), cvt_pk_16(lo.z, lo.w, bf), cvt_pk_16(hi.x, hi.y, bf), cvt_pk_16(hi.z, hi.w, bf));
    }
    if (c < 16) *(float4*)(enc + r * 64 + c * 4) = ok ? *(const float4*)(bank_enc + sr * 64 + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// 8 elements per lane: 4 x 16 bytes of int64 and 2 x 16 bytes of fp32 in, 16 bytes of int16 and 16 bytes of fp16 out
__global__ void __launch_bounds__(256) lg_emit_hloc_kernel(const long long* __restrict__ m0, const float* __restrict__ s0,
                                                           short* __restrict__ om, unsigned short* __restrict__ os, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    if (i + 8 <= n) {
        const gim_i64x2_t* mp = (const gim_i64x2_t*)(m0 + i);
        const gim_i64x2_t a = mp[0], b = mp[1], c = mp[2], d = mp[3];
        const float4 p = *(const float4*)(s0 + i), q = *(const float4*)(s0 + i + 4);
        auto pk = [](long long x, long long y) { return ((unsigned)x & 0xffffu) | ((unsigned)y << 16); };   // .short(): the low 16 bits
        *(uint4*)(om + i) = make_uint4(pk(a[0], a[1]), pk(b[0], b[1]), pk(c[0], c[1]), pk(d[0], d[1]));
        *(uint4*)(os + i) = make_uint4(cvt_pk_f16(p.x, p.y), cvt_pk_f16(p.z, p.w), cvt_pk_f16(q.x, q.y), cvt_pk_f16(q.z, q.w));
    } else {
        for (size_t j = i; j < n; ++j) {
            om[j] = (short)m0[j];
            os[j] = __builtin_bit_cast(unsigned short, (_Float16)s0[j]);   // .half(): round to nearest even
        }
    }
}

inline bool storage_ok(int storage) { return storage == GIM_F32 || storage == GIM_F16; }

}  // namespace

extern "C" int gim_lg_bank_put(const float* kpts, const float* desc, const float* size_wh, const float* Wr, const int32_t* slots,
                               float* bank_kpts, void* bank_desc, float* bank_enc, int n, int K, int n_slots, int storage,
                               gim_stream_t stream) {
    GIM_REQUIRE(n >= 0 && K > 0 && n_slots > 0, "lg_bank_put: n=%d K=%d n_slots=%d", n, K, n_slots);
    GIM_REQUIRE(storage_ok(storage), "lg_bank_put: storage dtype tag %d (GIM_F32 or GIM_F16)", storage);
    if (n == 0) return GIM_OK;
    GIM_REQUIRE(kpts && slots, "lg_bank_put: NULL keypoints / slots");
    GIM_REQUIRE(!desc || bank_desc, "lg_bank_put: descriptors without a bank slab");
    GIM_REQUIRE(!Wr || (size_wh && bank_enc), "lg_bank_put: Wr without image sizes / an encoding slab");
    GIM_REQUIRE((((uintptr_t)desc | (uintptr_t)bank_desc) & 15) == 0 && (((uintptr_t)kpts | (uintptr_t)bank_kpts) & 7) == 0,
                "lg_bank_put: descriptors must be 16-byte aligned, keypoints 8-byte aligned");
    GIM_REQUIRE((int64_t)n * K <= (int64_t)1 << 26, "lg_bank_put: n*K=%lld rows in one call", (long long)n * K);
    const size_t t = (size_t)n * K * 32;
    if (storage == GIM_F16)
        hipLaunchKernelGGL(lg_bank_put_kernel<true>, dim3(nblocks(t, 256)), dim3(256), 0, (hipStream_t)stream, kpts, desc, size_wh, Wr,
                           slots, bank_kpts, bank_desc, bank_enc, n, K, n_slots);
    else
        hipLaunchKernelGGL(lg_bank_put_kernel<false>, dim3(nblocks(t, 256)), dim3(256), 0, (hipStream_t)stream, kpts, desc, size_wh, Wr,
                           slots, bank_kpts, bank_desc, bank_enc, n, K, n_slots);
    return gim_check_launch("lg_bank_put");
}

static int lg_gather(const void* bank_desc, const float* bank_enc, const int32_t* idx0, const int32_t* idx1, const int32_t* counts,
                     float* x32, void* cat, float* enc, int32_t* len0, int32_t* len1, int B, int K, int n_slots, int storage, int dtype,
                     int ld_x32, int ld_cat, gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K > 0 && n_slots > 0, "lg_gather_pairs: B=%d K=%d n_slots=%d", B, K, n_slots);
    GIM_REQUIRE(storage_ok(storage), "lg_gather_pairs: storage dtype tag %d (GIM_F32 or GIM_F16)", storage);
    if (B == 0) return GIM_OK;
    GIM_REQUIRE(bank_desc && bank_enc && idx0 && idx1 && x32 && enc, "lg_gather_pairs: NULL argument");
    // fp32 compute: the residual stream IS the GEMM operand (x32 aliases CAT[:, :256]) -- written once, no 16-bit copy
    GIM_REQUIRE((dtype == GIM_F32) == (cat == nullptr), "lg_gather_pairs: cat must be NULL in fp32 mode and only then");
    GIM_REQUIRE(ld_x32 >= 256 && ld_x32 % 4 == 0 && (cat == nullptr || (ld_cat >= 256 && ld_cat % 8 == 0)),
                "lg_gather_pairs: ld_x32=%d ld_cat=%d must keep 16-byte rows", ld_x32, ld_cat);
    GIM_REQUIRE((((uintptr_t)bank_desc | (uintptr_t)bank_enc | (uintptr_t)x32 | (uintptr_t)cat | (uintptr_t)enc) & 15) == 0,
                "lg_gather_pairs: buffers must be 16-byte aligned");
    GIM_REQUIRE((int64_t)2 * B * K <= (int64_t)1 << 26, "lg_gather_pairs: 2*B*K=%lld rows in one call", (long long)2 * B * K);
    const size_t t = (size_t)2 * B * K * 32;
    const int kind = dtype == GIM_F32 ? 0 : dtype;
    if (storage == GIM_F16)
        hipLaunchKernelGGL(lg_gather_pairs_kernel<true>, dim3(nblocks(t, 256)), dim3(256), 0, (hipStream_t)stream, bank_desc, bank_enc, idx0,
                           idx1, x32, cat, enc, B, K, n_slots, kind, ld_x32, ld_cat, counts, len0, len1);
    else
        hipLaunchKernelGGL(lg_gather_pairs_kernel<false>, dim3(nblocks(t, 256)), dim3(256), 0, (hipStream_t)stream, bank_desc, bank_enc, idx0,
                           idx1, x32, cat, enc, B, K, n_slots, kind, ld_x32, ld_cat, counts, len0, len1);
    return gim_check_launch("lg_gather_pairs");
}

extern "C" int gim_lg_gather_pairs(const void* bank_desc, const float* bank_enc, const int32_t* idx0, const int32_t* idx1, float* x32,
                                   void* cat, float* enc, int B, int K, int n_slots, int storage, int dtype, int ld_x32, int ld_cat,
                                   gim_stream_t stream) {
    GIM_TAG_ANY(dtype, gim_lg_gather_pairs);   // the compute dtype; one object serves every kind, nothing to route
    return lg_gather(bank_desc, bank_enc, idx0, idx1, nullptr, x32, cat, enc, nullptr, nullptr, B, K, n_slots, storage, dtype, ld_x32,
                     ld_cat, stream);
}

extern "C" int gim_lg_gather_pairs_ragged(const void* bank_desc, const float* bank_enc, const int32_t* idx0, const int32_t* idx1,
                                          const int32_t* counts, float* x32, void* cat, float* enc, int32_t* len0, int32_t* len1, int B,
                                          int K, int n_slots, int storage, int dtype, int ld_x32, int ld_cat, gim_stream_t stream) {
    GIM_TAG_ANY(dtype, gim_lg_gather_pairs_ragged);
    GIM_REQUIRE(B == 0 || (counts && len0 && len1), "lg_gather_pairs_ragged: NULL count / length table");
    return lg_gather(bank_desc, bank_enc, idx0, idx1, counts, x32, cat, enc, len0, len1, B, K, n_slots, storage, dtype, ld_x32, ld_cat,
                     stream);
}

extern "C" int gim_lg_emit_hloc(const int64_t* matches0, const float* mscores0, int16_t* matches0_i16, void* mscores0_f16, int B, int K,
                                gim_stream_t stream) {
    GIM_REQUIRE(B >= 0 && K >= 0, "lg_emit_hloc: B=%d K=%d", B, K);
    GIM_REQUIRE(K <= 32767, "lg_emit_hloc: K=%d keypoints do not fit hloc's int16 matches0 (at most 32767)", K);
    if (B == 0 || K == 0) return GIM_OK;
    GIM_REQUIRE(matches0 && mscores0 && matches0_i16 && mscores0_f16, "lg_emit_hloc: NULL argument");
    GIM_REQUIRE((((uintptr_t)matches0 | (uintptr_t)mscores0 | (uintptr_t)matches0_i16 | (uintptr_t)mscores0_f16) & 15) == 0,
                "lg_emit_hloc: buffers must be 16-byte aligned");
    const size_t n = (size_t)B * K;
    hipLaunchKernelGGL(lg_emit_hloc_kernel, dim3(nblocks((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)matches0,
                       mscores0, (short*)matches0_i16, (unsigned short*)mscores0_f16, n);
    return gim_check_launch("lg_emit_hloc");
}
