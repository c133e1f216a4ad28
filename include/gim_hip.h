/* libgimhip -- C ABI of the MI355X (gfx950) gim_loftr hot path.
 *
 * The reference (xuelunshen/gim) is 100 % Python and has no FFI of its own; its hot path is the
 * `forward` of `networks/loftr/loftr.py:43-91` built from stock torch ops.  Each entry point below
 * replaces one group of those torch ops (reference file:line cited per function) and is what the
 * Python host shell `gim_amd/loftr/` binds through `ctypes` (see INTEGRATION.md for the stub a
 * reference maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted;
 *   - every call is asynchronous on `stream` (pass torch.cuda.current_stream().cuda_stream);
 *   - the library never allocates user-visible memory: outputs / workspaces are caller-allocated;
 *   - return 0 on success, negative GIM_ERR_* otherwise; message via gim_last_error() (thread local);
 *   - `dtype` arguments: GIM_F32 (exact-parity mode, fp32 MFMA), GIM_BF16 (throughput mode, 8 significand bits, fp32 range)
 *     or -- on the gim_loftr entry points (conv, layout / pos-enc / LayerNorm glue, linear attention, coarse matching, fine
 *     gather) -- GIM_F16 (throughput mode, IEEE fp16 operands: 11 significand bits at the same MFMA rate, |x| < 65504; a
 *     quarter of bf16's index flips against the fp32 reference).  A call is of ONE 16-bit kind; the one
 *     mixed form is gim_conv2d_bn_act with dtype GIM_F16 and out_dtype GIM_BF16 (no residual / upsample operand): the bf16
 *     mode's first convolution reads the image as fp16;
 *   - activations are NHWC ("pixel rows"): row m = ((b*H + y)*W + x), `ld*` = row stride in ELEMENTS.
 */
#ifndef GIM_HIP_H
#define GIM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gim_stream_t; /* hipStream_t */

/* The dtype tag.  ONE convention for every entry point that handles 16-bit operands: the name declared here takes the tag (a `dtype` /
 * `out_dtype` / `feat_dtype` argument or struct field) and the library routes the call to its bf16 or its IEEE-fp16 build of the kernel;
 * no per-dtype symbol is part of this ABI.  The fused kernels (gim_bneck64_fused*, gim_bneck_tail*, gim_token_mlp*, gim_fine_fused*)
 * work on ONE 16-bit kind -- tensors and packed weights alike -- named by their `dtype`: GIM_BF16 or GIM_F16; any other tag returns
 * GIM_ERR_INVALID before a pointer is looked at or the device is touched.  The entry points that take their tag(s) as `int` arguments
 * and accept GIM_F32 too refuse, in the same place and the same way, a tag that is none of the three and -- with two tags -- a call that
 * names BOTH 16-bit kinds (a 16-bit tag next to GIM_F32 is the mixed-precision form, e.g. gim_sdpa with fp16 operands and an fp32
 * output).  gim_stem7x7 alone takes the two 16-bit kinds side by side (fp16 image -> bf16 activations) and refuses GIM_F32. */
enum { GIM_F32 = 0, GIM_BF16 = 1, GIM_F16 = 2 };
enum { GIM_ACT_NONE = 0, GIM_ACT_RELU = 1, GIM_ACT_LEAKY = 2, GIM_ACT_ELU1 = 3 /* elu(x)+1 */, GIM_ACT_GELU = 4 /* exact erf GELU */ };
enum { GIM_OK = 0, GIM_ERR_INVALID = -1, GIM_ERR_LAUNCH = -2, GIM_ERR_UNSUPPORTED = -3 };

/* 110 (round 5): the fp16 range-guard word is an ARGUMENT of the entry points that use it (`health` of gim_bneck64_fused*,
 * gim_bneck_tail*, gim_conv_args.health; gim_set_range_guard() is gone), and gim_coarse_match's `count` is int32[2 + N] (count[1] = health
 * word, per-pair counts from count[2]) -- a caller bound to version 100 must be rebuilt.
 * 111: struct gim_token_emit grew the kv_part / kv_nchunk / kv_tile0 / kv_len arrays (fused KV state), q_weights (local queries), project_only and pe_*; zero them for
 * the old behaviour;
 * new entries gim_linear_attention_finalize, gim_linear_attention_ws_bytes_chunks.
 * 112 (round 6): gim_coarse_args.precand_per_row appended (zero it for the old behaviour); the library reads no environment variable.
 * 113 (round 6): gim_conv_args.split16 appended (zero it for the old behaviour).
 * 114: health bit 8 -- a split16 launch handed a `health` word reports an operand that left the IEEE-fp16 range (gim_conv_args.split16);
 * fp32-operand launches with split16 = 0 and a 16-bit output take exact fp32 products (version 113 sent some of them to the split loop).
 * 115: the fused kernels take a `dtype` tag (in front of `health`, else of `stream`; gim_token_mlp_emit: in front of `emit`) like every other
 * entry point, and the `*_f16` twins (gim_stem7x7_f16, gim_bneck64_fused*_f16, gim_bneck_tail*_f16, gim_token_mlp*_f16, gim_fine_fused*_f16)
 * left this header: call the plain name with GIM_F16 -- a caller bound to version 114 must be rebuilt. */
int gim_version(void);
/* fp16 range guard.  `health` (NULL: no check): a device word into which the fp16 flavour of the kernels that store un-normalised
 * residual streams (gim_bneck64_fused*, gim_bneck_tail*, gim_conv2d_bn_act with a residual operand) OR 4 when a converted value exceeds
 * the IEEE-fp16 range -- ReLUs downstream turn the resulting NaNs into zeros, so the outputs alone do not show it.  A plain argument:
 * no process-wide state, a captured graph keeps the word it was captured with.  gim_amd passes count[1] of gim_coarse_match. */
const char* gim_last_error(void);
/* compile-time facts the host packer needs: K-tile bytes (128) and the N padding granule (64). */
int gim_ktile_bytes(void);
int gim_npad_granule(void);

/* --------------------------------------------------------------------------------------------
 * Layout conversion: [B,C,H,W] fp32 (the reference's boundary layout, loftr.py:59) ->
 * NHWC rows [B*H*W, ld] of `dtype`, channels >= C zero-filled up to `cpad`.
 * `b_off`: first output image index (color0 -> 0, color1 -> bs: replaces torch.cat, loftr.py:60). */
int gim_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int cpad, int ld,
                     int b_off, int dtype, gim_stream_t stream);
/* The same boundary conversion for the split-operand first convolution (16-bit dtypes only): every channel c becomes the pair
 * hi = rn16(x), lo = rn16(x - hi), stored as channels [hi(0..C) | lo(0..C) | hi(0..C) | zeros up to ld]; with weights packed as
 * [w_hi | w_hi | w_lo] (gim_amd/packing.py::pack_conv_split) the 16-bit MFMA evaluates x*w to 2^-22 instead of 2^-11: the input
 * of backbone/resnet.py:306 (conv1 7x7 on the image) is where half of the 16-bit modes' deviation from the fp32 reference arises. */
int gim_nchw_to_nhwc_split(const float* src, void* dst, int B, int C, int H, int W, int ld, int b_off, int dtype,
                           gim_stream_t stream);
/* (ld >= 3 C: the layout above.  2 C <= ld < 3 C: [hi(0..C) | lo(0..C) | zeros] -- one 16-byte piece per RGB pixel, the input of gim_stem7x7.) */

/* --------------------------------------------------------------------------------------------
 * The first convolution of the backbone as its own kernel: conv1 7x7 / stride 2 / pad 3, 3 -> 64, + bn1 (folded) + relu
 * (backbone/resnet.py:306).  x [B,H,W,8] 16-bit pixels (one 16-byte piece each: gim_nchw_to_nhwc with cpad 8 for split = 0,
 * gim_nchw_to_nhwc_split with ld 8 for split = 1), w = the LDS image of the filter bank (gim_stem7x7_weight_bytes(split) bytes,
 * gim_amd/packing.py::pack_stem7x7: split = 1 carries every filter as a hi + lo pair), bias [64] fp32, y [B,Ho,Wo,64] of out_dtype
 * (bf16 / fp16; Ho = (H - 1) / 2 + 1).  dtype = the operands' 16-bit kind.  The implicit-GEMM entry computes the same layer
 * (split: on 16 channels per pixel) and remains the fp32 mode's path. */
int64_t gim_stem7x7_weight_bytes(int split);
int gim_stem7x7(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int split, int dtype, int out_dtype,
                gim_stream_t stream);
/* inverse, for exposing feature maps in the reference layout (tests / lazy outputs) */
int gim_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int ld, int dtype,
                     gim_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution with fused epilogue (MFMA):
 *     y[m, n] = act( sum_k A[m,k] * w[n,k] + bias[n] + res[m or m % res_mod, n] )
 * Replaces Conv2d+BatchNorm2d(eval)+ReLU/LeakyReLU(+residual add) of
 * `networks/loftr/backbone/resnet.py:109-126,230-233,316-327` and, with a 1x1 "pixel = row" view,
 * every bias-free nn.Linear of `submodules/transformer.py:47-55` (+ elu+1 of attentions.py:31-32).
 * A[m,k] is gathered on the fly: k -> (dy,dx,c) through `ktab` (one int per 16-byte K group:
 * c | dx<<16 | dy<<24, dy=255 marks K padding), pixel (b, ho*stride-pad+dy, wo*stride-pad+dx).
 * Weights `w` are packed [npad][kpad] in `dtype` with BN already folded in (host side). */
typedef struct gim_conv_args {
    const void* x;      /* input rows, dtype */
    const void* w;      /* packed weights [npad][kpad], dtype */
    const int32_t* ktab;/* [(kpad*elemsize/128 + 2) * 8]: two trailing slabs of 0xFF000000 */
    const float* bias;  /* [npad] or NULL */
    const void* res;    /* residual rows or NULL */
    void* y;            /* output rows */
    int64_t x_bytes;    /* size of the x allocation in bytes (buffer-descriptor bound, < 4 GiB) */
    int B, H, W;        /* input images / spatial size */
    int Ho, Wo;         /* output spatial size */
    int stride, pad;
    int ldx, ldy, ldres;/* row strides in elements */
    int N;              /* valid output channels stored (multiple of 4, <= npad) */
    int npad, kpad;
    int act;            /* GIM_ACT_* */
    int act_cols;       /* 0: activation on every column; >0 (multiple of 128): only on columns < act_cols
                           (fused [q|k|v] projection: elu+1 on q,k but not on v) */
    int res_mod;        /* 0: res row = m;  >0: res row = m % res_mod (broadcast over images) */
    int dtype;          /* dtype of x and w */
    int out_dtype;      /* dtype of y */
    int res_dtype;      /* dtype of res */
    int use_lds_dma;    /* 1: buffer_load ... lds staging (default); 0: register staging; 2: 3x3 halo kernel (w / ktab / kpad =
                           the halo packing, res_mod = channels stored per input row); 3: as 1, and the 256 x 256 tile takes the launch
                           whatever its size (its selection is a size heuristic: the parity tests reach it on small shapes this way) */
    const void* ups;    /* NULL, or a half-resolution tensor [B, ups_h, ups_w, ups_ld] (dtype = out_dtype, 16-bit) whose bilinear x2
                           upsampling (align_corners=True) is added to the conv output in fp32, in front of the ONE 16-bit rounding (round 6:
                           as 48 more K of the MFMA per 32-pixel pass; act must be GIM_ACT_NONE): the FPN's
                           `x2_out + F.interpolate(x3_out, scale_factor=2.)` (backbone/resnet.py:321-327) without a second pass
                           over y.  Output rows = (image, Y < 2 ups_h, X < 2 ups_w); needs (2 ups_w) % 32 == 0 and a launch the 256 x 256 tile takes
                           (1x1 conv, bf16, no residual, npad % 256 == 0, >= 4 K slabs, >= 512 tiles): gim_conv_ups_supported() */
    int ups_h, ups_w, ups_ld;
    int32_t* health;    /* or NULL.  fp16 range guard (see the top of this file): checked where a residual operand is added (fp16 flavour).  Split launches
                           (split16 = 1, version 114): bit 8 when an operand left the fp16 range (see split16) */
    int split16;        /* fp32 operands only (ABI 113).  0: products on v_mfma_f32_32x32x2_f32 (exact fp32 products).  1: every fp32 operand value is
                           split in registers into an IEEE-fp16 pair hi + lo and x w is evaluated as hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16
                           with fp32 accumulation (weights scaled by 2^12 for the split, accumulators scaled back): 2^-22 relative per product at
                           3/8 of the matrix-pipe time.  Range: |x| < 65520 and |w| < 65520 / 4096 = 15.996 (hi = rn16 of the value must be finite).
                           Beyond it hi and lo become +-inf and every accumulator of that pixel row (or channel column) NaN -- which a ReLU
                           epilogue turns into 0 -- so the launch ORs 8 into `health` (version 114; checked once per tile in the epilogue,
                           before residual and activation).  Accuracy floor: hi + lo carries an activation to about 2^-22 of its value only while
                           lo is a normal fp16 (|x| >= 2^-3); below, lo is subnormal and the error is up to 2^-25 absolute (the weights, scaled by
                           2^12 first, keep 2^-37).  A layer whose activations ALL lie near 1e-5 is good to ~1e-3 of its output scale, near 1e-7
                           to ~4e-2: a documented limit of the mode (tests/test_gpu_split16_range.py pins the bands).  Any value may be
                           given with split16 = 0 (exact fp32 products). */
    int pad_;
} gim_conv_args;
int gim_conv_ups_supported(const gim_conv_args* a);   /* 1 if gim_conv2d_bn_act would take a->ups (set or not) for this launch */
int gim_conv2d_bn_act(const gim_conv_args* a, gim_stream_t stream);
/* The 3x3 halo launch of gim_conv2d_bn_act (use_lds_dma = 2: 16-bit, stride 1, pad 1, halo packing) over a device-side list of
 * 8 x 32-pixel output patches (added within ABI revision 114).  tiles[0 .. min(*n_tiles, tiles_cap)): int32 patch indices
 * (image * ceil(H / 8) + ty) * ceil(W / 32) + tx, ascending for L2 locality; *n_tiles is read ON THE DEVICE (no host sync, the grid
 * does not depend on it; 0 writes nothing).  Listed patches get exactly what the dense launch writes; pixels of every other patch
 * keep whatever y held.  Entries outside the map are clamped into it. */
int gim_conv3x3_halo_tiles(const gim_conv_args* a, const int* tiles, const int* n_tiles, int tiles_cap, gim_stream_t stream);
/* The upsample-carrying launch of gim_conv2d_bn_act (a 1x1 conv with a->ups: the FPN's lateral conv + bilinear x2 + add) over a device-side
 * list of 8 x 32-pixel patches of its output map [images, 2 ups_h, 2 ups_w] (added within ABI revision 115: no existing structure or
 * prototype changed with it).  The list is that of gim_conv3x3_halo_tiles: int32 patch indices (image * (2 ups_h / 8) + ty) * (2 ups_w / 32)
 * + tx, ascending, *n_tiles read ON THE DEVICE and clipped to tiles_cap, entries outside the map clamped into it.  Listed patches get exactly
 * the bits the dense launch writes; pixels of every other patch keep whatever y held.
 * gim_conv_ups_tiles_supported(): 1 if the launch is one this entry takes -- the conditions of gim_conv_ups_supported() without its
 * tile-count floor (the list decides the count), a 16-bit dtype, the 1x1 conv stated flat (B = H = Ho = 1, W = Wo = the pixel count,
 * stride 1, pad 0) and an output map of whole patches: (2 ups_h) % 8 == 0, (2 ups_w) % 32 == 0. */
int gim_conv_ups_tiles_supported(const gim_conv_args* a);
int gim_conv2d_ups_tiles(const gim_conv_args* a, const int* tiles, const int* n_tiles, int tiles_cap, gim_stream_t stream);
/* The plain 3 x 3 / stride 1 / pad 1 launch of gim_conv2d_bn_act on its 256 x 256 tile over a device-side list of 8 x 32-pixel patches of its
 * output map [B, H, W] (added within ABI revision 115: no existing structure or prototype changed with it).  The list is that of
 * gim_conv3x3_halo_tiles: int32 patch indices (image * (H / 8) + ty) * (W / 32) + tx, ascending, *n_tiles read ON THE DEVICE and clipped to
 * tiles_cap, entries outside the map clamped into it.  Same K loop, weight packing and K order as the dense launch on that tile: listed
 * patches get exactly the bits it writes; pixels of every other patch keep whatever y held.
 * gim_conv2d_tiles_supported(): 1 if the launch is one this entry takes -- a 16-bit dtype in and out, stride 1, pad 1, Ho = H, Wo = W (k = 3),
 * no residual, no `ups`, no split16, no act_cols, use_lds_dma 1 or 3, H % 8 == 0, W % 32 == 0, npad % 256 == 0, at most 32 768 patches.
 * gim_conv2d_big_tile(): 1 if gim_conv2d_bn_act runs the DENSE launch of these 16-bit args on that 256 x 256 tile as well (enough tiles and
 * K slabs, or use_lds_dma = 3) -- only then are the two bit-identical. */
int gim_conv2d_tiles_supported(const gim_conv_args* a);
int gim_conv2d_big_tile(const gim_conv_args* a);
int gim_conv2d_tiles(const gim_conv_args* a, const int* tiles, const int* n_tiles, int tiles_cap, gim_stream_t stream);

/* y[m,:] += bilinear_upsample_2x(x)[m,:], align_corners=True (resnet.py:321,325: F.interpolate +
 * the `x2_out+x3_out_2x` add).  x: [B,h,w,C] rows (ldx), y: [B,2h,2w,C] rows (ldy), in place. */
int gim_upsample2x_add(const void* x, void* y, int B, int h, int w, int C, int ldx, int ldy,
                       int dtype, gim_stream_t stream);

/* out_f32[m,:] = x[m,:] + pe[m % hw, :]   (loftr.py:74-75 pos_encoding + 'n c h w -> n (h w) c';
 * NHWC rows make the rearrange free).  Also writes a `dtype` copy (GEMM operand) if out_t != NULL. */
int gim_posenc_add(const void* x, const float* pe, float* out_f32, void* out_t, int rows, int hw,
                   int C, int ldx, int ld_f32, int ld_t, int dtype, gim_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * LinearAttention (submodules/attentions.py:20-47), q/k already elu+1'd by the projection epilogue.
 *   step 1  gim_linear_attention_kv:  KV[b,h,:,:] = sum_s K[b,s,h,:]^T (V[b,s,h,:]/S),  Ksum[b,h,:]
 *   step 2  gim_linear_attention_apply: out[b,l,h,:] = (Q KV) / (Q.Ksum + eps) * S
 * k,v: [nb*S, ld] rows, q: [nb*L, ld] rows; `kv_ws` >= gim_linear_attention_ws_bytes(...) bytes.
 * kv_mask [nb*S] / q_mask [nb*L] (uint8, NULL = no mask): padded positions, attentions.py:35-39
 * (K, V rows with mask 0 do not contribute; Q rows with mask 0 give a zero message).
 * Arithmetic of step 1 at the coarse level (D = 32, H = 8): 16-bit operands -- exact products on the 16-bit MFMA, fp32 sums, 1/S applied
 * to the sums; fp32 operands -- fp32 MFMA on K and V/S.  Partial sums of row chunks are combined in a fixed order (run-to-run deterministic).
 * The partials are those of 256-row chunks whatever workgroup shape the launch takes: a sequence's state does not depend on the batch it
 * travels in, bit for bit.
 * gim_linear_attention_finalize (version 111): the last step alone -- state = sum of `nchunk` partial states per sequence and head that somebody
 * else wrote (gim_token_mlp_emit's fused KV state: one partial per 64-row tile) into a workspace of gim_linear_attention_ws_bytes_chunks bytes:
 * [state: nb x H x (D D + D) fp32][partials: nb x H x nchunk x (D D + D) fp32]. */
int64_t gim_linear_attention_ws_bytes(int nb, int S, int H, int D);
int64_t gim_linear_attention_ws_bytes_chunks(int nb, int H, int D, int nchunk);
int gim_linear_attention_finalize(float* kv_ws, int nb, int H, int D, int nchunk, gim_stream_t stream);
int gim_linear_attention_kv(const void* k, const void* v, const uint8_t* kv_mask, float* kv_ws, int nb,
                            int S, int H, int D, int ldk, int ldv, int dtype, gim_stream_t stream);
int gim_linear_attention_apply(const void* q, const uint8_t* q_mask, const float* kv_ws, void* out,
                               int nb, int L, int S, int H, int D, int ldq, int ldo, int dtype,
                               int out_dtype, gim_stream_t stream);

/* Same LinearAttention for SHORT sequences (the fine level's 25-token windows, transformer on [M,25,128],
 * loftr.py:88): one wave per sequence fuses both steps, no workspace.  Requires H == 8, D in {16, 32}. */
int gim_linear_attention_short(const void* q, const void* k, const void* v, const uint8_t* q_mask,
                               const uint8_t* kv_mask, void* out, int nb, int L, int S, int H, int D,
                               int ldq, int ldk, int ldv, int ldo, int dtype, int out_dtype,
                               gim_stream_t stream);

/* LayerNorm (+ optional residual):  v = LN(x[m,:]) * gamma + beta ; if res: v += res[m,:]
 * (transformer.py:52,56,58).  x is `x_dtype` (fp32, or bf16 pre-norm activations in the throughput mode).
 * Writes fp32 (out_f32, may be NULL) and/or `dtype` copy (out_t). */
int gim_layernorm_residual(const void* x, const float* gamma, const float* beta, const float* res,
                           float* out_f32, void* out_t, int rows, int C, int ldx, int ldres,
                           int ld_f32, int ld_t, int x_dtype, int dtype, float eps, gim_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Coarse matching (utils/coarse_matching.py:88-259): dual-softmax + threshold + border + mutual-NN
 * + ordered compaction, fused so that the [N,L,S] confidence matrix is never written.
 * feat0 [N*L, C] / feat1 [N*S, C] fp32 rows (row stride C).  Outputs in torch.where order
 * (ascending b, then i): b_ids/i_ids/j_ids int64, mconf fp32, mkpts0_c/mkpts1_c fp32 [cap,2].
 * `count` (device int32[2 + N], ZERO IT ONCE when allocating): count[0] = M, count[2+b] = matches of pair b, count[1] = health word:
 * bit 0 (rewritten by every call) = a NaN / inf similarity reached the statistics -- the inputs or weights were not finite, or an
 * overflow survived the ReLUs in between; bit 1 (sticky, never cleared here) = gim_fine_fused_dev saw a non-finite fine-level
 * output on this buffer: a host that replays a captured graph on the same buffer learns it with the NEXT call's count read-back;
 * bit 2 (sticky) = the fp16 range guard: a kernel that stores an un-normalised residual stream converted a value beyond 65504
 * that was handed this word as its `health` argument; bit 8 (sticky, version 114) = the split range guard: a gim_conv2d_bn_act launch with
 * split16 = 1 that was handed this word met an fp32 operand beyond the fp16 range of its hi / lo split (gim_conv_args.split16).  The reference has no such word (fp32 has the range);
 * gim_amd/loftr/loftr.py reads it with the match count (coarse_matching.py:193's sync) and re-runs the batch in bf16.
 * scale0/scale1: NULL or fp32 [N,2] per-pair (w,h) scales (coarse_matching.py:237-245). */
typedef struct gim_coarse_args {
    const void* feat0;    /* [N, L, ldf] rows of C features, fp32 or bf16 (feat_dtype) */
    const void* feat1;    /* [N, S, ldf] */
    const float* scale0;
    const float* scale1;
    const uint8_t* mask0; /* NULL or [N, L] padding mask of image0's coarse cells (coarse_matching.py:116-117) */
    const uint8_t* mask1; /* NULL or [N, S]; with masks the border rule is mask_border_with_padding (:29-44) */
    void* ws;             /* >= gim_coarse_match_ws_bytes() */
    int64_t* b_ids;
    int64_t* i_ids;
    int64_t* j_ids;
    float* mconf;
    float* mkpts0_c;
    float* mkpts1_c;
    int32_t* count;
    int N, L, S, C;
    int h0c, w0c, h1c, w1c;
    int cap;              /* capacity of the output arrays (N * min(L,S) always suffices) */
    float temperature;    /* dsmax_temperature (0.1) */
    float thr;            /* 0.2 */
    int border_rm;        /* 2 */
    float scale;          /* hw0_i[0] / hw0_c[0] */
    int feat_dtype;       /* GIM_F32 (0, default) or GIM_BF16: bf16 features run the similarity on the bf16 MFMA -- exact
                           * products, fp32 accumulation, i.e. the fp32 result for bf16-valued inputs up to summation order */
    int ldf;              /* row stride of feat0 / feat1 in elements; 0 = C (contiguous) */
    int precand_per_row;  /* 0 = default (16 pre-candidate slots per row, what gim_coarse_match_ws_bytes sizes); 1..16 = fewer; -1 = none: the
                           * device-side overflow flag then routes every call to the two-pass recompute (tests; replaces an environment hook) */
} gim_coarse_args;
int64_t gim_coarse_match_ws_bytes(int N, int L, int S);
int gim_coarse_match(const gim_coarse_args* a, gim_stream_t stream);
/* materialise conf_matrix [N,L,S] fp32 (data['conf_matrix'], coarse_matching.py:144) on demand;
 * needs the workspace of the preceding gim_coarse_match call (row/column softmax statistics). */
int gim_coarse_conf_matrix(const gim_coarse_args* a, float* conf, gim_stream_t stream);

/* Tail of a ResNet Bottleneck (planes 64) fused with the head of the next block (resnet.py:109-126), one kernel:
 *     x' = relu(bn3(conv3(relu(bn2(conv2_3x3(t1))))) + identity);   t1' = relu(bn1'(conv1'(x')))   (optional)
 * Tensors and weights are of `dtype` (GIM_BF16 / GIM_F16), called "bf16" below.
 * t1: [B,H,W,64] bf16 (the block's conv1 output), res: [B,H,W,256] bf16 identity / downsample branch, x_out: [B,H,W,256],
 * t1_next: [B,H,W,n_next] or NULL (n_next = 64: the next block of the layer; 128: the next layer's first conv1; 0: none).
 * Weights bf16 with eval-BN folded in (biases fp32): w2 [64][576] with K = (ky, kx, c);
 * w3 [256][64] and w1n [n_next][256] with K permuted to the MFMA accumulator layout (gim_amd/packing.py::pack_bneck) -- the three
 * products are chained through registers.  H % 8 == 0, W % 32 == 0. */
int gim_bneck64_fused(const void* t1, const void* res, void* x_out, void* t1_next, const void* w2, const void* w3,
                      const void* w1n, const float* b2, const float* b3, const float* b1n, int B, int H, int W,
                      int n_next, int dtype, int32_t* health, gim_stream_t stream);
/* First block of layer 1 (resnet.py:120-124: identity = bn(conv1x1(x)), 64 -> 256, stride 1): the downsample convolution runs INSIDE
 * the kernel as extra K of conv3 -- x' = relu([W3 | Wds] [t2 ; x] + b3 + bds) -- so neither its launch nor the 256-channel identity
 * tensor exist.  x_in: [B,H,W,64] the block's input; wds [256][64] bf16 (BN folded, K in channel order); b3ds = b3 + bds; n_next = 64. */
int gim_bneck64_fused_ds(const void* t1, const void* x_in, void* x_out, void* t1_next, const void* w2, const void* w3,
                         const void* wds, const void* w1n, const float* b2, const float* b3ds, const float* b1n, int B, int H, int W,
                         int dtype, int32_t* health, gim_stream_t stream);

/* The same fusion one layer up (planes 128: layer 2), without the 3x3 -- x' = relu(bn3(conv3_1x1(t2)) + identity), t1' =
 * act(bn1'(conv1'_1x1(x'))) of the NEXT block (resnet.py:117-124, 109-111) -- so that x' [M,512], the widest tensor of the block, is
 * written once and not read back.  t2: [M,128] (the block's conv2 output), res: [M,512], x_out: [M,512], t1_next: [M,n_next], n_next
 * in {128, 256}; M = pixel rows, a multiple of 256 (both convolutions are 1x1: no spatial structure).  w3 [512][128] K in channel
 * order, w1n [8][n_next][64]: per 64-channel chunk of x', K in accumulator order (gim_amd/packing.py::pack_bneck_tail); the 256+ KiB
 * of weights stream through LDS two chunks ahead of the MFMAs.  act_next: GIM_ACT_RELU / GIM_ACT_NONE. */
int gim_bneck_tail128(const void* t2, const void* res, void* x_out, void* t1_next, const void* w3, const void* w1n,
                      const float* b3, const float* b1n, int M, int n_next, int act_next, int dtype, int32_t* health,
                      gim_stream_t stream);
/* First block of layer 2 with its `downsample` branch INSIDE the kernel (round 5; resnet.py:120-124: identity = bn(conv1x1, stride 2 (x))):
 *     x' = relu([W3 | Wds] [t2 ; x_in(b, 2y, 2x)] + b3 + bds);   t1' = act(bn1'(conv1'(x')))
 * -- neither the downsample launch nor its 512-channel output exist.  t2 [B,Ho,Wo,128] (conv2 output, stride 2), x_in [B,Hin,Win,256] the
 * block's input (Hin >= 2 Ho - 1, Win >= 2 Wo - 1), x_out [B,Ho,Wo,512], t1_next [B,Ho,Wo,128]; B Ho Wo a multiple of 256.
 * w3ds [512][128 + 256] (K: t2's channels, then x_in's, both in channel order, BN folded), w1n [16][128][32] (32-channel chunks of x', K in
 * accumulator order), b3ds = b3 + bds (gim_amd/packing.py::pack_bneck_tail(..., ds=True)). */
int gim_bneck_tail128_ds(const void* t2, const void* x_in, void* x_out, void* t1_next, const void* w3ds, const void* w1n,
                         const float* b3ds, const float* b1n, int B, int Ho, int Wo, int Hin, int Win, int n_next, int act_next,
                         int dtype, int32_t* health, gim_stream_t stream);
/* Planes 256 (layer 3): t2 [M,256], res / x_out [M,1024], t1_next [M,256] (n_next = 256); w3 [1024][256], w1n [32][256][32] (chunks of
 * 32 channels).  x_out may be NULL: the last block's output is read by nothing but the fused 1x1 convolution -- the FPN's
 * layer3_outconv (resnet.py:316), act_next = GIM_ACT_NONE, zero bias -- so it is never written. */
int gim_bneck_tail256(const void* t2, const void* res, void* x_out, void* t1_next, const void* w3, const void* w1n,
                      const float* b3, const float* b1n, int M, int n_next, int act_next, int dtype, int32_t* health,
                      gim_stream_t stream);

/* Token-wise tail of a LoFTREncoderLayer in ONE kernel (16-bit operand modes, d_model 256; transformer.py:52-58; "bf16" below = the
 * 16-bit kind named by `dtype`, GIM_BF16 / GIM_F16):
 *     x += norm2(mlp.2(relu(mlp.0(cat[x, norm1(merge(msg))]))))
 * msg: [R][ldm] bf16 attention output; xb: [R][ldxb] bf16 operand copy of x (read, then overwritten with the new x);
 * x32: [R][ldx32] fp32 residual stream (read-modify-write).  `weights`: gim_token_mlp_weight_bytes() bytes of bf16 in the
 * per-wave fragment order of gim_amd/packing.py::pack_token_mlp; ln_params: [norm1.weight | norm1.bias | norm2.weight |
 * norm2.bias] fp32.  64 rows per workgroup; none of the intermediate row buffers exists in memory.
 * kv != NULL fuses the apply step of the linear attention (attentions.py:44-45) in front: `msg` then holds the elu+1 QUERY rows,
 * kv the [nb][8][32*32 + 32] fp32 state written by gim_linear_attention_kv (nb = R / L sequences of L rows, L % 64 == 0), S the
 * source length, q_mask an optional [R] padding mask. */
int64_t gim_token_mlp_weight_bytes(void);
int gim_token_mlp(const void* msg, void* xb, float* x32, const void* weights, const float* ln_params, const float* kv,
                  const uint8_t* q_mask, int R, int C, int L, int S, int ldm, int ldxb, int ldx32, float ln_eps,
                  int dtype, gim_stream_t stream);

/* gim_token_mlp + projection blocks of the NEW x, computed on the tile while it is still in LDS: the q / k / v projections of
 * the following LoFTREncoderLayer (transformer.py:42-44; in a cross layer also the k / v of the same layer's second call), each
 * a bias-free [256 x 256] Linear with elu(.)+1 on q and k (attentions.py:31-32):   out[b][m, 0:256] = act[b](x_new[m] W_b^T)
 * for the rows m of 64-row tiles whose first row lies in [row_lo[b], row_hi[b]).  weights: nblk x 128 KiB of 16-bit values in the
 * per-wave fragment order of gim_amd/packing.py::pack_token_emit. */
#define GIM_TOKEN_EMIT_MAX 6
typedef struct gim_token_emit {
    int nblk;
    const void* weights;
    void* out[GIM_TOKEN_EMIT_MAX];      /* row 0 of the block's output columns, 16-bit, 16-byte aligned */
    int ld[GIM_TOKEN_EMIT_MAX];         /* row stride in elements (multiple of 8) */
    int act[GIM_TOKEN_EMIT_MAX];        /* GIM_ACT_NONE or GIM_ACT_ELU1 */
    int row_lo[GIM_TOKEN_EMIT_MAX], row_hi[GIM_TOKEN_EMIT_MAX];
    /* Fused KV state (version 111).  kv_part[b] != NULL: blocks b (k, elu + 1) and b + 1 (v; same row range, whole 64-row tiles) are NOT
     * written; each tile stores the partial state K^T V / kv_len, K^T 1 of its 64 rows (attentions.py:38-43) at
     * kv_part[b][sequence][8 heads][kv_nchunk[b]][32 * 32 + 32] fp32, tile index = kv_tile0[b] + (tile's first row - row_lo[b]) / 64 counted
     * over the consuming call's source rows (sequence = index / kv_nchunk, chunk = index % kv_nchunk).  kv_part is the partial area of a
     * gim_linear_attention_kv workspace (gim_linear_attention_part) and gim_linear_attention_finalize turns it into the state.  out[] /
     * ld[] of the two blocks are ignored. */
    float* kv_part[GIM_TOKEN_EMIT_MAX];
    int kv_nchunk[GIM_TOKEN_EMIT_MAX], kv_tile0[GIM_TOKEN_EMIT_MAX];
    float kv_len[GIM_TOKEN_EMIT_MAX];
    /* Local queries (version 111).  q_weights != NULL (needs kv != NULL): `msg` is not read; the elu + 1 query rows of the fused attention
     * apply are projected inside the kernel from xb, q = elu(xb Wq^T) + 1 (transformer.py:42, attentions.py:31).  128 KiB of 16-bit values in
     * the order of ONE block of packing.py::pack_token_emit([Wq]).  nblk may be 0 then. */
    const void* q_weights;
    /* Projection only (version 111).  != 0: nothing of the layer runs -- msg, x32, weights, ln_params, kv may be NULL -- the blocks are
     * projections of the 16-bit rows `xb` as they are (the first layer's k / v pair as partial KV states: replaces its projection GEMM). */
    int project_only;
    /* ... with the positional encoding in front (loftr.py:74-75; pe != NULL, project_only only): the rows are pe_feat[m] (16-bit, stride pe_ld)
     * + pe[m % pe_hw] (fp32 [pe_hw][256]) in gim_posenc_add's arithmetic; the kernel writes them to x32 (fp32) and xb (16-bit) before it projects. */
    const void* pe_feat;
    const float* pe;
    int pe_ld, pe_hw;
} gim_token_emit;
int gim_token_mlp_emit(const void* msg, void* xb, float* x32, const void* weights, const float* ln_params, const float* kv,
                       const uint8_t* q_mask, int R, int C, int L, int S, int ldm, int ldxb, int ldx32, float ln_eps,
                       int dtype, const gim_token_emit* emit, gim_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Fine level.  gim_fine_gather = F.unfold(k=W,stride,pad=W/2) + [b_ids,i_ids] pick
 * (submodules/fine_preprocess.py:40-47) without materialising the unfold: windows of image0 go to
 * rows [0, M*WW), windows of image1 to rows [M*WW, 2*M*WW).
 * feat_f0: [bs, hf0, wf0, C] rows, feat_f1: [bs, hf1, wf1, C] rows (row stride ldf) in `dtype`. */
int gim_fine_gather(const void* feat_f0, const void* feat_f1, const int64_t* b_ids,
                    const int64_t* i_ids, const int64_t* j_ids, float* out_f32, void* out_t, int M,
                    int hf0, int wf0, int hf1, int wf1, int C, int ldf, int w0c, int w1c, int stride,
                    int W, int ld_f32, int ld_t, int dtype, gim_stream_t stream);
/* FineMatching.forward + get_fine_match (utils/fine_matching.py:43-74): centre-row correlation,
 * softmax over WW, DSNT expectation + std, final coordinates.
 * f0/f1: fp32 [M*WW, C] rows.  scale1: NULL or fp32 [bs,2] (applied iff has_scale0, line 68). */
int gim_fine_match(const float* f0, const float* f1, const float* mkpts1_c, const int64_t* b_ids,
                   const float* scale1, float* expec_f, float* mkpts1_f, int M, int WW, int C, int ld,
                   float scale, int has_scale0, gim_stream_t stream);
/* The whole fine level in ONE kernel (16-bit operand modes, d_model 128, 5x5 windows, layer_names ['self','cross']; "bf16" below = the
 * 16-bit kind named by `dtype`, GIM_BF16 / GIM_F16):
 * window gather (fine_preprocess.py:40-47) + LocalFeatureTransformer (transformer.py:35-58,80-101, LinearAttention
 * attentions.py:20-47) + FineMatching (fine_matching.py:43-74); 2 matches per workgroup, activations never leave the CU.
 * feat_f0/feat_f1: NHWC bf16 fine maps (row stride ldf).  `weights`: gim_fine_fused_weight_bytes() bytes, bf16, per layer
 * [Wq | Wk | Wv | Wmerge | mlp.0 rows 0..127 | mlp.0 rows 128..255 | mlp.2 cols 0..127 | mlp.2 cols 128..255], each block
 * [128 out][K] re-ordered to MFMA fragment order [wave = out/32][k16 step][lane = (k/8 % 2)*32 + out%32][8] (host side:
 * gim_amd/packing.py::pack_fine_fused).  ln_params: per layer [norm1.weight | norm1.bias | norm2.weight | norm2.bias] fp32.
 * dbg_fine0/dbg_fine1: NULL or fp32 [M, 25, 128] dumps of the transformer output (tests). */
int64_t gim_fine_fused_weight_bytes(void);
int gim_fine_fused(const void* feat_f0, const void* feat_f1, const int64_t* b_ids, const int64_t* i_ids,
                   const int64_t* j_ids, const float* mkpts1_c, const float* scale1, const void* weights,
                   const float* ln_params, float* expec_f, float* mkpts1_f, float* dbg_fine0, float* dbg_fine1,
                   int M, int hf0, int wf0, int hf1, int wf1, int C, int ldf, int w0c, int w1c, int stride, int W,
                   float scale, float ln_eps, int has_scale0, int dtype, gim_stream_t stream);
/* The same launch without the host knowing the match count: it covers M_cap = the capacity of the match lists and processes the first
 * min(M_cap, *count_dev) of them (count_dev = gim_coarse_match's count[0]); expec_f / mkpts1_f hold M_cap rows.  The reference
 * synchronises on the count (torch.where, coarse_matching.py:193) before the fine level; here the read-back overlaps this kernel. */
int gim_fine_fused_dev(const void* feat_f0, const void* feat_f1, const int64_t* b_ids, const int64_t* i_ids,
                       const int64_t* j_ids, const float* mkpts1_c, const float* scale1, const void* weights,
                       const float* ln_params, float* expec_f, float* mkpts1_f, int M_cap, const int* count_dev,
                       int hf0, int wf0, int hf1, int wf1, int C, int ldf, int w0c, int w1c, int stride, int W,
                       float scale, float ln_eps, int has_scale0, int dtype, gim_stream_t stream);


/* ======================================================================================================
 * gim_lightglue path: SuperPoint detector glue + LightGlue matcher.
 * The convolutions and Linear layers of both networks run on gim_conv2d_bn_act above.
 * ====================================================================================================== */

/* nn.MaxPool2d(2, 2) on NHWC rows -- replaces superpoint.py:216,219,222 (`self.pool`). */
int gim_maxpool2x2(const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy, int dtype,
                   gim_stream_t stream);

/* Detector head tail -- replaces superpoint.py:231-236: softmax over the 65 logits of each 8x8 cell
 * (rows [B*h*w][ld], ld >= 65), dustbin dropped, depth-to-space -> scores [B, 8h, 8w] fp32. */
int gim_sp_scores(const void* logits, float* scores, int B, int h, int w, int ld, int dtype,
                  gim_stream_t stream);

/* simple_nms + border removal -- replaces superpoint.py:61-80 (radius, 2 refinement rounds) and :247-258
 * (scores within `border` px of the canvas edge = -1; the reference always uses the canvas size, :207).
 * out [B,H,W] fp32: score at kept maxima, 0 elsewhere, -1 on the border. */
int64_t gim_sp_nms_ws_bytes(int B, int H, int W);
int gim_sp_nms(const float* scores, float* out, void* ws, int B, int H, int W, int radius, int border,
               gim_stream_t stream);

/* Keypoint extraction -- replaces superpoint.py:260-300,308: candidates `score > thr`, top-k by score in
 * descending order (`torch.topk(sorted=True)`; fewer than k candidates: all of them in torch.where order),
 * kpts [B,k,2] = (x, y) as float (without the +0.5 of :346), kscores [B,k], nvalid [B] = min(#candidates, k)
 * (entries >= nvalid are zero; the caller pads them like pad_and_stack).  B <= 64, k <= 4096, thr >= 0. */
int64_t gim_sp_topk_ws_bytes(int B, int H, int W);
int gim_sp_topk(const float* nms_scores, void* ws, float* kpts, float* kscores, int32_t* nvalid, int B,
                int H, int W, int k, float thr, gim_stream_t stream);

/* Descriptor sampling -- replaces superpoint.py:241 (per-pixel F.normalize of the dense map, fused),
 * :120-137 (legacy_sampling: bilinear grid_sample, align_corners=True) and the final F.normalize.
 * dense rows [B*h*w][ld] (raw convDb output), kpts [B,K,2]; out_f32 / out_t rows [B*K][C], C = 256. */
int gim_sp_sample_desc(const void* dense, const float* kpts, float* out_f32, void* out_t, int B, int K,
                       int h, int w, int C, int ld, int ld_f32, int ld_t, int cell, int dtype,
                       gim_stream_t stream);

/* normalize_keypoints + LearnableFourierPositionalEncoding -- replaces lightglue.py:21-33,47-61.
 * kpts [B,K,2], size_wh [B,2] = (w, h), Wr [32,2]; enc [B*K][64] = cos(proj)[32] | sin(proj)[32]
 * (the reference's [2,B,1,K,64] tensor is this table with every entry repeated twice). */
int gim_lg_posenc(const float* kpts, const float* size_wh, const float* Wr, float* enc, int B, int K,
                  gim_stream_t stream);

/* apply_cached_rotary_emb -- replaces lightglue.py:36-44,150-151: in place on columns [0, ncols) of x
 * (ncols % 64 == 0; heads of 64, the same table for every head). */
int gim_lg_rotary(void* x, const float* enc, int rows, int ncols, int ld, int dtype, gim_stream_t stream);

/* V -> V^T per sequence for gim_sdpa: dst[nb][C][Sp], key index contiguous, zero for key >= S (Sp = S
 * rounded up to a multiple of 64). */
int gim_lg_transpose(const void* src, void* dst, int nb, int S, int Sp, int C, int ld, int dtype,
                     gim_stream_t stream);

/* softmax(q k^T / sqrt(D)) v -- replaces Attention.forward (lightglue.py:104-118) and the bidirectional
 * cross attention of CrossBlock.forward (:196-207; the two directions are two calls).
 * q rows [nb*L][ldq], k rows [nb*S][ldk] (head h at columns h*D), vt from gim_lg_transpose, out rows
 * [nb*L][ldo].  Sequence s attends to the keys/values of sequence (s + kv_shift) % nb (self: 0;
 * cross with image0/image1 stacked as [2B]: kv_shift = B).  D = 64.  dtype f32: exact-fp32 MFMA. */
int gim_sdpa(const void* q, const void* k, const void* vt, void* out, int nb, int H, int L, int S, int Sp,
             int D, int ldq, int ldk, int ldo, int kv_shift, int dtype, int out_dtype, gim_stream_t stream);

/* LayerNorm (+ GELU) -- replaces ffn[1], ffn[2] of SelfBlock / CrossBlock (lightglue.py:135-139). */
int gim_layernorm_act(const float* x, const float* gamma, const float* beta, void* out, int rows, int C,
                      int ldx, int ldo, int act, int out_dtype, float eps, gim_stream_t stream);

/* fp32 rows -> dtype rows (residual stream -> GEMM operand copy). */
int gim_cast_rows(const float* src, void* dst, int rows, int C, int ld_src, int ld_dst, int dtype,
                  gim_stream_t stream);

/* MatchAssignment + sigmoid_log_double_softmax + filter_matches, fused -- replaces lightglue.py:226-300. */
typedef struct gim_lg_assign_args {
    const float* desc0;   /* [B*M][ld_desc] final descriptors (matchability input) */
    const float* desc1;   /* [B*N][ld_desc] */
    const float* md0;     /* [B][M][C] final_proj(desc0), unscaled */
    const float* md1;     /* [B][N][C] */
    const float* match_w; /* matchability.weight [C] */
    const float* match_b; /* matchability.bias [1] */
    void* ws;             /* >= gim_lg_assign_ws_bytes() */
    int64_t* matches0;    /* [B][M], -1 = unmatched */
    int64_t* matches1;    /* [B][N] */
    float* mscores0;      /* [B][M] */
    float* mscores1;      /* [B][N] */
    int32_t* pos;         /* [B][M] position of row i in its pair's match list, -1 = unmatched */
    int32_t* count;       /* [B] matches per pair */
    int B, M, N, C;
    int ld_desc;
    float threshold;      /* filter_threshold (0.1) */
} gim_lg_assign_args;
int64_t gim_lg_assign_ws_bytes(int B, int M, int N, int C);
int gim_lg_assign(const gim_lg_assign_args* a, gim_stream_t stream);
/* `pred["log_assignment"]` [B][M+1][N+1] on demand (lightglue.py:226-238). */
int gim_lg_log_assignment(const gim_lg_assign_args* a, float* out, gim_stream_t stream);
/* `matches` / `scores` lists (lightglue.py:497-506) packed over the batch in torch.where order, and the
 * caller-side adapter of trainer/lightning.py:176-183 / demo.py:503-510 (mkpts = keypoints * scale,
 * m_bids); mkpts0 == NULL skips the adapter outputs. */
int gim_lg_emit_matches(const int64_t* matches0, const float* mscores0, const int32_t* pos,
                        const int32_t* count, const float* kpts0, const float* kpts1, const float* scale0,
                        const float* scale1, int64_t* matches, float* scores, float* mkpts0, float* mkpts1,
                        int64_t* m_bids, int B, int M, int N, gim_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Output hand-out.  gim_copy_segments: up to GIM_MAX_COPY_SEGS independent device byte ranges moved (src == NULL: zero
 * filled) in ONE launch -- the private copies of b_ids / i_ids / j_ids / m_bids / mkpts0_c / mkpts1_c / mconf and the
 * all-false gt_mask that `data` receives after coarse matching (coarse_matching.py:236-259: tensor construction only).
 * gim_pack_matches: reporting rows [pair_id, x0, y0, x1, y1, conf] (24 B per match; the packed form of the per-pair rows of
 * trainer/lightning.py:258-270); pair_id = pair_ids[m_bids[m]] (device int64, one per batch element) or, with
 * pair_ids == NULL, pid_base + m_bids[m]. */
enum { GIM_MAX_COPY_SEGS = 12 };
typedef struct gim_copy_segs {
    const void* src[12];
    void* dst[12];
    int64_t bytes[12];
    int n;
} gim_copy_segs;
int gim_copy_segments(const gim_copy_segs* segs, gim_stream_t stream);
int gim_pack_matches(const int64_t* m_bids, const float* mkpts0, const float* mkpts1, const float* mconf,
                     const int64_t* pair_ids, int64_t pid_base, float* out, int M, gim_stream_t stream);
/* The patches of the 1/2-resolution fine maps [2 bs, H, W, .] (images of side 0, then of side 1) that the fine level of the first
 * min(count[0], cap) matches can read, for gim_conv3x3_halo_tiles (added within ABI revision 114).  A patch is listed when it
 * holds a pixel of [stride cy - 3, stride cy + 3] x [stride cx - 3, stride cx + 3] clipped to the map, (cy, cx) = the match's coarse cell
 * (i_ids / w0c on side 0, j_ids / w1c on side 1): the 5 x 5 fine window (fine_preprocess.py:40-47) plus the one-pixel reach of a 3 x 3
 * convolution.  tiles: ascending int32 patch indices ((side * bs + b) * ceil(H / 8) + ty) * ceil(W / 32) + tx, n_tiles[0] their number;
 * tiles_cap >= the patch total.  One workgroup, the count is read on the device; at most gim_fine_tile_list_max_flags() patches. */
int gim_fine_tile_list_max_flags(void);
int gim_fine_tile_list(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                       int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int tiles_cap, gim_stream_t stream);
/* gim_fine_tile_list and, from the same launch, a second list of the same form for the reach grown by one pixel (added within ABI
 * revision 115): tiles4 / n_tiles4 list the patches that hold a pixel of [stride cy - 4, stride cy + 4] x [stride cx - 4, stride cx + 4]
 * clipped to the map -- what the INPUT of the last-but-one 3 x 3 convolution must hold, for gim_conv2d_ups_tiles.  tiles / n_tiles get
 * exactly what gim_fine_tile_list writes; both lists have tiles_cap entries. */
int gim_fine_tile_lists(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                        int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int* tiles4, int* n_tiles4, int tiles_cap,
                        gim_stream_t stream);
/* gim_fine_tile_lists and, from the same launch, three patch lists of the 1/4-resolution maps [2 bs, H / 2, W / 2] (added within ABI
 * revision 115; H % 16 == 0, W % 64 == 0).  S = every pixel of the 1/4-resolution map that the lateral launch gim_conv2d_ups_tiles stages as
 * an upsample source for a patch of tiles4: per 32-pixel pass (row Y, first column X0) rows y0 = (int)(sy Y), y0 + (y0 < h - 1) and columns
 * xa .. min(xa + 23, w - 1), xa = (int)(sx X0), fp32, sy = (float)(h - 1) / (float)(H - 1), sx likewise -- weight-0 sources included.
 * tilesq = int32 [3][tilesq_cap]: the ascending lists of 8 x 32 patches ((side * bs + b) * (h / 8) + ty) * (w / 32) + tx that hold a pixel of
 * S dilated by 2 (list A), by 1 (list B) and of S itself (list C), dilations clipped to the map; n_tilesq = int32 [3] their counts.  The
 * half- and quarter-level patches together must not exceed gim_fine_tile_list_max_flags(). */
int gim_fine_tile_lists4(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                         int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int* tiles4, int* n_tiles4, int tiles_cap,
                         int* tilesq, int* n_tilesq, int tilesq_cap, gim_stream_t stream);
/* gim_fine_tile_lists4 for the pairs [b_lo, b_hi) alone, 0 <= b_lo <= b_hi <= bs (added within ABI revision 115): a match whose b_ids value
 * lies outside the range marks nothing; patch indices, list order and buffer sizes stay those of the whole batch, so the lists of disjoint
 * ranges are disjoint and their sorted union is the list of the union of the ranges.  b_lo = 0, b_hi = bs writes what gim_fine_tile_lists4
 * writes; an empty range writes the five counts (0) and no list entry.  For launch chains that each own the images of a pair range. */
int gim_fine_tile_lists4_range(const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, const int* count, int cap, int bs,
                               int w0c, int w1c, int stride, int H, int W, int* tiles, int* n_tiles, int* tiles4, int* n_tiles4, int tiles_cap,
                               int* tilesq, int* n_tilesq, int tilesq_cap, int b_lo, int b_hi, gim_stream_t stream);

/* ======================================================================================================
 * gim_dkm path (kernels D1-D9).  Convolutions / 1x1 projections / the cosine-kernel and
 * posterior-mean products run on gim_conv2d_bn_act (runtime "weights" = row buffers in [N][K] layout).
 * ====================================================================================================== */

/* torchvision resnet50 `maxpool` (kernel 3, stride 2, padding 1) on NHWC rows -- encoders.py:51. */
int gim_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy, int dtype,
                     gim_stream_t stream);
/* F.interpolate(mode='bilinear', align_corners=False) on NHWC rows -- dkm.py:420-425,468-479,518-529,668-701. */
int gim_resize_bilinear(const void* x, void* y, int B, int h, int w, int Ho, int Wo, int C, int ldx, int ldy,
                        int dtype, int out_dtype, gim_stream_t stream);
/* The same resize for the NCHW fp32 input images, written as NHWC rows with cpad channels (images b_off..)
 * -- dkm.py:668-669,700-701. */
int gim_resize_image(const float* x, void* y, int B, int C, int h, int w, int Ho, int Wo, int cpad, int b_off,
                     int out_dtype, gim_stream_t stream);
/* F.grid_sample(bilinear, zeros padding, align_corners=False): feat [B,h,w,C] at grid [B,Ho,Wo,2] (x, y)
 * -- dkm.py:89.  Any finite grid value is allowed (targets far outside the map give zeros); h, w <= 65536. */
int gim_grid_sample(const void* feat, const float* grid_xy, void* out, int B, int h, int w, int Ho, int Wo, int C,
                    int ldf, int ldo, int dtype, gim_stream_t stream);
/* disp_emb(flow - query_coords): 1x1 conv 2 -> E on the displacement field -- dkm.py:91-101. wgt [E][2]. */
int gim_dkm_disp_emb(const float* flow, const float* wgt, const float* bias, void* out, int B, int h, int w, int E,
                     int ldo, int out_dtype, gim_stream_t stream);
/* local_correlation(x, y, local_radius=r, flow) -- utils/local_correlation.py:5-40: out[b,y,x,k], k = (2r+1)^2
 * bilinear window taps of f1 around the flow target, dotted with f0, / sqrt(C).  r <= 7. */
int gim_local_corr(const void* f0, const void* f1, const float* flow, void* out, int B, int h, int w, int C, int r,
                   int ld0, int ld1, int ldo, int dtype, int out_dtype, gim_stream_t stream);
/* ConvRefiner.create_block, first half (dw=True): depthwise 5x5 conv (Cout = mult * Cin) + eval BatchNorm + ReLU
 * -- dkm.py:58-73.  wgt [25][cpad], scale / shift [cpad] fp32 (conv bias and BN folded), zero padded. */
int gim_dwconv5x5_bn_relu(const void* x, const float* wgt, const float* scale, const float* shift, void* y, int B,
                          int H, int W, int Cin, int Cout, int cpad, int ldx, int ldy, int dtype, gim_stream_t stream);
/* The whole ConvRefiner block of DKM / RoMa (dkm.py:58-73, create_block: depthwise 5x5 + BatchNorm + ReLU + 1x1 convolution with bias) in ONE launch,
 * 16-bit operands, for the refiners whose channel count fits one channel chunk: cs = 144 stored channels (the scale-2 refiner) or 24 / 32 (scale 1).
 * The depthwise output goes to an LDS tile and is the B operand of the 1x1's MFMAs; the intermediate tensor is never written.  x [B,H,W,ldx],
 * y [B,H,W,ldy] rows of cs stored channels; wgt [25][cs], scale / shift [cs] fp32 (BatchNorm folded, as gim_dwconv5x5_bn_relu); pw_w [NP][KP] 16-bit
 * (rows = output channels padded to NP = 160 / 32, K = input channels padded to KP = 144 / 32, zero padding); pw_b [NP] fp32.  dtype GIM_BF16 / GIM_F16. */
int gim_dwconv5x5_pw(const void* x, const float* wgt, const float* scale, const float* shift, const void* pw_w, const float* pw_b, void* y,
                     int B, int H, int W, int cs, int ldx, int ldy, int dtype, gim_stream_t stream);
/* CosKernel pieces -- dkm.py:135-144: row L2 norms, and K = exp((dot / (nx ny + eps) - 1) / T) in place on the
 * dot-product matrix (diag_add = sigma_noise on the diagonal, dkm.py:352). */
int gim_row_norms(const void* x, float* out, int rows, int C, int ld, int dtype, gim_stream_t stream);
int gim_cos_kernel_finish(float* k, const float* nx, const float* ny, int B, int n, int m, int ld, float T, float eps,
                          float diag_add, gim_stream_t stream);
/* (K_yy + sigma I)^-1 f of GP.forward -- dkm.py:352-359 -- as a blocked fp64 Cholesky solve (the reference inverts
 * with LU in fp32).  K [B][n][ldk] fp32 with sigma on the diagonal, F [B][n][nrhs] fp32;
 * Xt [B][nrhs][npad] fp32 = (K^-1 F)^T zero padded: the [N][K] operand layout of gim_conv2d_bn_act.  B <= 16.
 * A batch entry whose factorisation meets a pivot that is not positive (matrix not positive definite, NaN or overflowed entries) comes
 * back as quiet NaN in EVERY element of Xt[b], padding included; the other entries are unaffected.  No status is returned for it: the
 * call does not wait for the device. */
int64_t gim_gp_solve_ws_bytes(int B, int n, int nrhs);
int gim_gp_solve(const float* K, const float* F, float* Xt, void* ws, int B, int n, int ldk, int nrhs, int npad,
                 gim_stream_t stream);
/* The same posterior evaluated ENTIRELY in fp64 from fp32 feature rows (the dense matchers' parity mode): cosine-kernel entries,
 * Cholesky and both products on the fp64 MFMA.  X (queries) / Y (supports): [B][n][ldx] fp32, d features per row; F [n][nrhs] fp32
 * (shared by all B directions); mu [B][n][ld_mu] fp32 = K_xy (K_yy + sigma I)^-1 F with K = exp((cos - 1) / T), cos = x.y / (|x||y| + eps)
 * (dkm.py:135-144, 340-370; roma.py:94-136).  The system's condition number (~2e4) turns the 1e-7 rounding of fp32 kernel entries
 * into ~1e-4 of mu; this entry point removes that term from the engine's side.  B <= 16.  As with gim_gp_solve, a direction whose
 * K_yy + sigma I fails to factor (NaN or overflowed support features) has every element of mu[b] (n x nrhs) written as quiet NaN. */
int64_t gim_gp_posterior_f64_ws_bytes(int B, int n, int d, int nrhs);
int gim_gp_posterior_f64(const float* X, const float* Y, const float* F, float* mu, void* ws, int B, int n, int d, int ldx,
                         int nrhs, int ld_mu, float T, float eps, float sigma, gim_stream_t stream);
/* CAB -- dkm.py:160-168: global average pool of NHWC rows into out[b][c_off + c]; out = sigmoid(g) * x2 + x1. */
int gim_global_avgpool(const void* x, float* out, int B, int HW, int C, int ld, int ldo, int c_off, int dtype,
                       gim_stream_t stream);
int gim_cab_scale_add(const float* g, const void* x1, const void* x2, void* out, int B, int HW, int C, int ldg, int ld1,
                      int ld2, int ldo, int dtype, gim_stream_t stream);
/* Decoder.forward flow / certainty update -- dkm.py:505-514, roma.py:318-331.  cert_init bit 0: certainty = delta
 * (instead of +=); bit 1: d rows = [dx, dy, delta certainty] (RoMa, roma.py:579) instead of [delta certainty, dx, dy]. */
int gim_dkm_flow_update(float* flow, float* cert, const void* d, int64_t npix, int ldd, float sx, float sy,
                        int cert_init, int dtype, gim_stream_t stream);
/* get_placeholder_flow -- dkm.py:437-448. */
int gim_dkm_grid_coords(float* flow, int B, int h, int w, gim_stream_t stream);
/* match() tail of one symmetric pair -- dkm.py:693-741: flow / certainty / low-res certainty maps [H,W,.] of the two
 * directions (0 = query -> support) -> warp [H,2W,4], certainty [H,2W]; black masks from gim_dkm_black_mask (:726-729). */
int gim_dkm_match_post(const float* flow0, const float* flow1, const float* cert0, const float* cert1, const float* low0,
                       const float* low1, const uint8_t* black0, const uint8_t* black1, float* warp, float* certainty,
                       int H, int W, gim_stream_t stream);
int gim_dkm_black_mask(const float* im, uint8_t* mask, int h, int w, int Ho, int Wo, gim_stream_t stream);
/* kde(x, std) -- utils/kde.py:17-26: density[i] = sum_j exp(-cdist(x_i, x_j)^2 / (2 std^2)), x [n,4] fp32 (the
 * reference materialises the n x n distance matrix: 1.6 GB at n = 20000). */
int gim_kde(const float* x, float* density, int n, float std, gim_stream_t stream);  /* std < 0: |std| on fp16-rounded x (roma.py:1018-1023) */
/* cls_to_flow_refine + the certainty channel of TransformerDecoder's output -- roma.py:1092-1121, 1013-1014: logits rows
 * [npix][ld] fp32 = ncls (= res^2) anchor classes then the certainty logit -> flow [npix,2], cert [npix]. */
int gim_cls_to_flow(const float* logits, float* flow, float* cert, int npix, int ncls, int ld, gim_stream_t stream);
/* torch.multinomial(w, k, replacement=False) of RegressionMatcher.sample -- dkm.py:603-605,617-619: k distinct indices
 * drawn with probability proportional to w (exponential clocks + radix-select top-k), as an unordered set; reproducible
 * from `seed`.  Needs at least k positive weights. */
/* Caller-side dense adapter -- trainer/lightning.py:141-144 / demo.py:438-443: normalised [n,4] matches -> pixel
 * coordinates in the two images, kpts = size * (x + 1) / 2. */
int gim_dense_to_pixels(const float* matches, float* kpts0, float* kpts1, int n, float w0, float h0, float w1, float h1,
                        gim_stream_t stream);
int64_t gim_weighted_sample_ws_bytes(int n);
int gim_weighted_sample(const float* w, int64_t* out, void* ws, int n, int k, uint32_t seed, gim_stream_t stream);

/* ======================================================================================================
 * gim_semseg path: the CSAIL ADE20K-150 segmenter of gim's SfM / video paths (networks/mit_semseg, ResnetDilated + PPMDeepsup).
 * Its convolutions (dilated 3x3s included: the K-group table stores dy*d, dx*d) run on gim_conv2d_bn_act; these three are the rest.
 * ====================================================================================================== */

/* nn.AdaptiveAvgPool2d(s) of conv5 for s = 1, 2, 3, 6 in one launch -- models.py:446-451, 472-477.  x [B,H,W] rows of ldx (C channels,
 * `dtype`); out fp32 [B][50][C]: bins of s = 1, 2, 3, 6 from offsets 0, 1, 5, 14, row-major.  Bin i of s spans [floor(i H / s),
 * ceil((i + 1) H / s)) (bins overlap when H < s).  C % 4 == 0. */
int gim_ppm_pool(const void* x, float* out, int B, int H, int W, int C, int ldx, int dtype, gim_stream_t stream);
/* F.interpolate(bilinear, align_corners=False) of the four branch outputs (after 1x1 conv + BN + ReLU) from s x s to h x w, written into
 * channels c_off + i * Cb .. of y (rows [B*h*w][ldy], `dtype`): the concat buffer of conv_last, no torch.cat -- models.py:471-478.
 * br fp32 [B][50][Cb] in gim_ppm_pool's bin order. */
int gim_ppm_upsample_concat(const float* br, void* y, int B, int h, int w, int Cb, int ldy, int c_off, int dtype, gim_stream_t stream);
/* Inference tail of PPMDeepsup.forward + segment()'s torch.max -- models.py:482-486, hloc/utils/__init__.py:42-49: logits fp32 rows
 * [B*h*w][ld] (C <= 256 classes) upsampled bilinearly (align_corners=False) to H x W per output pixel, arg-max over the classes (the
 * lowest index wins a tie) -> cls uint8 [B][H][W]; prob (NULL: not written) fp32 [B][H][W] = the maximum softmax probability.  The
 * full-resolution C-channel tensor is never written.  flag (NULL: no check): a device word ORed with 1 when a logit is not finite. */
int gim_seg_head_argmax(const float* logits, uint8_t* cls, float* prob, int* flag, int B, int h, int w, int C, int ld, int H, int W,
                        gim_stream_t stream);

/* ======================================================================================================
 * Feature bank (gim_loftr): the backbone maps of an image are extracted once and matched in many pairs (added within ABI
 * revision 114).  The reference recomputes them per pair (networks/loftr/loftr.py:59-72).
 * ====================================================================================================== */

/* Indexed block copy between two slabs of equally sized slots, ONE launch: for i in [0, n) the block_bytes bytes (a positive multiple
 * of 16; both slabs 16-byte aligned) at src + src_idx[i] * block_bytes go to dst + dst_idx[i] * block_bytes, as 16-byte vector loads
 * and stores.  src_idx / dst_idx: DEVICE int32 arrays read by the kernel (the host does not wait for them), NULL = identity (i), which
 * needs n <= that side's slot count.  src_slots / dst_slots: slot counts of the slabs; a block whose source or destination index is
 * outside [0, slots) is skipped as a whole -- nothing is read or written out of bounds.  Destination indices must be distinct and the
 * slabs must not overlap.  Serves both directions: scatter of extracted maps into bank slots (src_idx NULL) and gather of a pair batch's
 * slots into the contiguous [bs, h, w, C] buffers the stages read (dst_idx NULL). */
int gim_slot_copy(const void* src, void* dst, const int32_t* src_idx, const int32_t* dst_idx, int n, int64_t block_bytes, int src_slots,
                  int dst_slots, gim_stream_t stream);

/* ======================================================================================================
 * Keypoint bank (gim_lightglue): the SuperPoint features of an image are stored once and matched in many pairs (added within
 * ABI revision 115: no existing structure or prototype changed with it).  The reference reloads both images' features and
 * recomputes both positional encodings for every pair (hloc/match_features.py:124-160, lightglue.py:414-430).
 * Bank arrays, `n_slots` images of K keypoints, dense and slot-major: kpts fp32 [n_slots][K][2], desc [n_slots][K][256] in the
 * `storage` dtype (GIM_F32 or GIM_F16 = IEEE fp16), enc fp32 [n_slots][K][64] (the table of gim_lg_posenc).  Slot indices are
 * DEVICE int32 arrays read by the kernels; an index outside [0, n_slots) is never used as an address.
 * ====================================================================================================== */

/* Inserts n images: image i goes to slot slots[i] (an out-of-range slot skips the image).  kpts [n][K][2] fp32, desc [n][K][256]
 * fp32 (16-byte aligned), size_wh [n][2] = (w, h), Wr [32][2].  Writes the slot's keypoints, its descriptors rounded to the storage
 * dtype (round to nearest even, as .half()) and its encoding -- bit for bit what gim_lg_posenc writes for the same fp32 keypoints,
 * size and Wr (one shared device function), so it is never computed again per pair.  Parts can be left out: desc == NULL leaves the
 * descriptors, bank_kpts == NULL the keypoints, Wr == NULL the encoding (size_wh, bank_enc unused) untouched -- a changed Wr rebuilds
 * the encodings of resident images with desc == bank_kpts == NULL.  Slots must be distinct. */
int gim_lg_bank_put(const float* kpts, const float* desc, const float* size_wh, const float* Wr, const int32_t* slots,
                    float* bank_kpts, void* bank_desc, float* bank_enc, int n, int K, int n_slots, int storage,
                    gim_stream_t stream);

/* The stacked row block of B pairs in ONE launch: rows [0, B*K) are the images idx0[b], rows [B*K, 2*B*K) the images idx1[b] (the
 * layout LightGlue.forward builds with two gim_lg_posenc launches, a concatenation, two copies and a gim_cast_rows).  x32 rows
 * [2*B*K][ld_x32] fp32 = the descriptors (fp16 storage: converted exactly), cat rows [2*B*K][ld_cat] = the same values in the compute
 * dtype `dtype` (GIM_BF16 / GIM_F16; the rounding of gim_cast_rows), enc [2*B*K][64] = the slots' encodings.  dtype GIM_F32: x32 is
 * the GEMM operand itself (it aliases CAT[:, :256], ld_x32 = 512) and cat must be NULL -- the row is written once.  A pair whose slot is
 * out of range gets zero rows.  16-byte loads and stores; all buffers 16-byte aligned. */
int gim_lg_gather_pairs(const void* bank_desc, const float* bank_enc, const int32_t* idx0, const int32_t* idx1, float* x32,
                        void* cat, float* enc, int B, int K, int n_slots, int storage, int dtype, int ld_x32, int ld_cat,
                        gim_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Ragged batches (added within ABI revision 115: no existing structure or prototype changed with them).  A batch keeps the padded row
 * layout -- sequence / pair b owns rows [b*K, (b+1)*K) on each side, K the capacity -- and device int32 length tables say how many of
 * those rows exist.  Contract: pair b gets what the uniform entry point gives for that pair alone at its own sizes (the reference's
 * LightGlue.forward at batch 1 takes any (m, n): lightglue.py:405-430); rows that do not exist are never read into a result.
 * The row-wise kernels (linears, gim_lg_rotary, gim_layernorm_act, gim_cast_rows) need no lengths.
 * ------------------------------------------------------------------------------------------------------ */

/* gim_lg_transpose with a length table: sequence s has len[s] <= S keys, dst columns >= len[s] are ZERO (a masked key has probability
 * exactly 0, and 0 x NaN is NaN: nothing of the padding may reach gim_sdpa_varlen's second MFMA).  Serves lightglue.py:112-118. */
int gim_lg_transpose_varlen(const void* src, void* dst, const int32_t* len, int nb, int S, int Sp, int C, int ld, int dtype,
                            gim_stream_t stream);

/* gim_sdpa (Attention.forward, lightglue.py:104-118, 196-207) over sequences of their own lengths: L and S stay the row strides of a
 * sequence, sequence s has len_q[s] <= L queries and attends to keys [0, len_k[kvseq]) of sequence kvseq = (s + kv_shift) % nb.  Valid
 * rows are gim_sdpa's at L = len_q[s], S = len_k[kvseq] bit for bit (the same tile walk); out rows [len_q[s], L) are written as zeros,
 * and so is the whole sequence when len_k[kvseq] == 0.  vt from gim_lg_transpose_varlen with the key lengths.  dtype_qkv / dtype_out are
 * gim_sdpa's dtype / out_dtype tags under the same rule: each GIM_F32 / GIM_BF16 / GIM_F16, one 16-bit kind per call. */
int gim_sdpa_varlen(const void* q, const void* k, const void* vt, void* out, const int32_t* len_q, const int32_t* len_k, int nb, int H,
                    int L, int S, int Sp, int D, int ldq, int ldk, int ldo, int kv_shift, int dtype_qkv, int dtype_out, gim_stream_t stream);

/* gim_lg_assign (lightglue.py:226-300) where pair b has len0[b] <= M rows and len1[b] <= N columns: the softmax statistics, the
 * arg-maxima and the mutual check see those only (tiles wholly outside are skipped); matches0 = -1, score 0 for i >= len0[b], likewise
 * side 1; pos / count and with them gim_lg_emit_matches keep torch.where order over the rows that exist.  An empty side: all -1, zero
 * scores, count 0.  gim_lg_log_assignment has no ragged form. */
int gim_lg_assign_ragged(const gim_lg_assign_args* a, const int32_t* len0, const int32_t* len1, gim_stream_t stream);

/* gim_lg_gather_pairs for a bank whose image in slot s has counts[s] <= K keypoints (counts int32 [n_slots]): rows at or beyond the
 * image's count are ZERO in x32, cat and enc whatever the slab holds there, and len0[b] = counts[idx0[b]], len1[b] = counts[idx1[b]]
 * (0 for a slot out of range) are written for the kernels above. */
int gim_lg_gather_pairs_ragged(const void* bank_desc, const float* bank_enc, const int32_t* idx0, const int32_t* idx1,
                               const int32_t* counts, float* x32, void* cat, float* enc, int32_t* len0, int32_t* len1, int B, int K,
                               int n_slots, int storage, int dtype, int ld_x32, int ld_cat, gim_stream_t stream);

/* hloc's sparse match-file datasets (hloc/match_features.py:150-160) of a whole batch from a gim_lg_assign result: matches0 int64
 * [B][K] -> int16 (the low 16 bits, as .short()), mscores0 fp32 [B][K] -> IEEE fp16 (round to nearest even, as .half()).  K > 32767
 * does not fit the int16 format and is refused before the launch.  All buffers 16-byte aligned. */
int gim_lg_emit_hloc(const int64_t* matches0, const float* mscores0, int16_t* matches0_i16, void* mscores0_f16, int B, int K,
                     gim_stream_t stream);

/* ======================================================================================================
 * root_sift baseline: descriptor matching (added within ABI revision 114: no existing structure or prototype
 * changed with it).
 * ====================================================================================================== */

/* RootSIFT normalisation, similarity, mutual nearest neighbour and Lowe's ratio test of root_sift_inference --
 * trainer/lightning.py:215-226, 230 (the same lines again in video_preprocessor.py:379-390) -- without the [n0, n1] similarity
 * matrix: desc0 [n0][D], desc1 [n1][D] fp32 row-major, 16-byte aligned, D a multiple of 16 in [16, 256] (SIFT 128, SuperPoint 256).
 * rootsift = 1: rows become sqrt(d / sum d) first (:215; copies in ws, the inputs are not modified).  Products are exact fp32.
 * match0 int32 [n0] = the index into desc1 or -1; score0 fp32 [n0] = the row maximum of the similarity (`mconf`; 0 for a row without
 * a comparable value); count = device int32 word, the number of rows with match0 >= 0.  ratio (0.8 at both reference call sites) <= 0
 * switches the ratio test off (plain mutual nearest neighbour).  A row that ties its maximum in several columns reports the lowest
 * such column, then tests mutuality (the reference picks a mutual one among them); NaN similarities (zero-sum row under rootsift)
 * never match; n1 == 1 has no second neighbour, so a positive ratio rejects every row; n0 == 0 or n1 == 0 writes count = 0 only.
 * ws: gim_nn_match_ws_bytes(n0, n1, D, rootsift) bytes, 16-byte aligned -- O((n0 + n1) D), nothing of size n0 x n1 exists. */
int64_t gim_nn_match_ws_bytes(int n0, int n1, int D, int rootsift);
int gim_nn_match(const float* desc0, const float* desc1, int n0, int n1, int D, int rootsift, float ratio, int32_t* match0,
                 float* score0, int32_t* count, void* ws, gim_stream_t stream);

/* ---- descriptor bank: the same matcher over a pair list (added within ABI revision 115: no existing structure or prototype changed
 * with it).  Bank arrays, `n_slots` images of at most `max_rows` descriptors, slot-major: bank_desc fp32 [n_slots][max_rows][D]
 * (16-byte aligned; slot s owns rows s * max_rows .. s * max_rows + bank_n[s] - 1), bank_n int32 [n_slots] on the DEVICE.  The
 * descriptors are stored as the sweep reads them (normalised once), so an image is never normalised again per pair. ---- */

/* Inserts one image: desc [n][D] fp32 DEVICE rows (16-byte aligned; NULL allowed when n == 0: an image without keypoints) into slot
 * `slot`, and bank_n[slot] = n, in ONE launch.  rootsift = 1 stores sqrt(d / sum d) per row -- the device function gim_nn_match's
 * normalisation calls, so the stored rows are bit-equal to the copies that call keeps in its workspace; rootsift = 0 is a plain copy.
 * slot outside [0, n_slots), n outside [0, max_rows] and a bad D are refused before the launch. */
int gim_nn_bank_put(const float* desc, int n, int D, int rootsift, int slot, float* bank_desc, int32_t* bank_n, int n_slots,
                    int max_rows, gim_stream_t stream);

/* HOST-only planning of a batch of P pairs (idx0[p], idx1[p]) of slots; every pointer is HOST memory and no device is touched.
 * n [n_slots] = the caller's mirror of bank_n.  Writes row_off [P + 1] / col_off [P + 1] = prefix sums of n[idx0[p]] / n[idx1[p]],
 * *nsplit = the column split of the batch (chosen from the TOTAL number of 128-row blocks: about 512 workgroups, at most 16; a pair
 * uses min(*nsplit, its column tiles)), *n_work = the number of work items, and, when work != NULL, the work table
 * work [n_work][4] = (pair, row block, first column tile, one past the last column tile) in pair, row block, split order
 * (work_cap = its capacity in items; too small is an error, work == NULL only counts).  A pair with n0 == 0 or n1 == 0 has no work
 * items.  A slot index outside [0, n_slots), a negative count and sums that do not fit int32 are refused. */
int gim_nn_match_pairs_plan(const int32_t* idx0, const int32_t* idx1, const int32_t* n, int P, int n_slots, int32_t* row_off,
                            int32_t* col_off, int32_t* work, int work_cap, int32_t* n_work, int32_t* nsplit);

/* gim_nn_match for P pairs of slots in at most three launches whatever P is (reset, sweep over the work table, final), no host
 * synchronisation.  idx0, idx1 [P], row_off, col_off [P + 1], work [n_work][4]: DEVICE copies of what gim_nn_match_pairs_plan made
 * (rows0 = row_off[P], rows1 = col_off[P], nsplit as planned); the kernels re-check every entry against n_slots, max_rows, bank_n and
 * the offsets and skip an item that does not fit, so nothing is read or written out of bounds.  The sweep is gim_nn_match's tile, the
 * same k-ordered exact-fp32 chain: every similarity, and so match0 / score0 / count, has the bits the single-pair call gives that
 * pair.  Ragged outputs: match0 int32 [rows0], score0 fp32 [rows0] (pair p owns row_off[p] .. row_off[p + 1] - 1), count int32 [P].
 * hloc != 0: the final kernel also writes hloc's match-file datasets in the same pass, matches0_i16 int16 [rows0] and
 * scores_f16 IEEE fp16 [rows0] = (1 + score0) / 2 on matched rows, 0 elsewhere (round to nearest even); max_rows > 32767 does not
 * fit int16 and is refused.  The same slot may appear on both sides and in many pairs; slots are only read.  Rules for n1 == 0,
 * n1 == 1 and ratio <= 0 as in gim_nn_match; a pair with n0 == 0 owns no rows.  P == 0 returns without a launch.
 * ws: gim_nn_match_pairs_ws_bytes(rows0, rows1) bytes, 16-byte aligned -- O(rows0 + rows1), never n0 x n1. */
int64_t gim_nn_match_pairs_ws_bytes(int rows0, int rows1);
int gim_nn_match_pairs(const float* bank_desc, const int32_t* bank_n, const int32_t* idx0, const int32_t* idx1, const int32_t* row_off,
                       const int32_t* col_off, const int32_t* work, int P, int n_work, int nsplit, int rows0, int rows1, int n_slots,
                       int max_rows, int D, float ratio, int32_t* match0, float* score0, int32_t* count, int hloc,
                       int16_t* matches0_i16, void* scores_f16, void* ws, gim_stream_t stream);

/* ======================================================================================================
 * RANSAC hypothesis scoring for the pose half of the ZEB loop (added within ABI revision 114).  Sampling, the minimal
 * solvers, the iteration bound and recoverPose stay on the host (gim_amd/pose.py); this is the inlier count that was 90 % of its step.
 * ====================================================================================================== */

/* Inlier counts of K candidate 3x3 models per pair over that pair's points, B pairs in ONE launch.  All pointers are DEVICE memory.
 * models fp64 [B][K][3][3] row-major; valid uint8 [B][K] or NULL (all valid); x0, x1 fp64 [Ptot][2] (16-byte aligned), the points of
 * the pairs concatenated; offsets int32 [B + 1], non-decreasing: pair b owns the points offsets[b] .. offsets[b + 1] (the kernel
 * trusts them -- the caller checks 0 <= offsets[b] <= offsets[b + 1] <= Ptot).  fp64 throughout:
 *   err = (x1^T M x0)^2 / max(|M x0|_xy^2 + |M^T x1|_xy^2, 1e-300)   with x = (x, y, 1),   inlier when err <= thr2
 * (pose.sampson_error; EMEstimatorCallback::computeError).  counts int32 [B][K] is FULLY written by the call (no memset by the
 * caller): 0 for a model with valid == 0, 0 for a model with a NaN entry (its comparison is false), the pair's point count for an
 * all-zero valid model (0 / 1e-300 = 0, as numpy), 0 for a pair without points.  Only integer sums cross threads: the result does not
 * depend on the launch shape.  B == 0 or K == 0 returns without touching anything.  B <= 65535. */
int gim_ransac_score(const double* models, const uint8_t* valid, const double* x0, const double* x1, const int32_t* offsets, int B,
                     int K, double thr2, int32_t* counts, gim_stream_t stream);
/* The inlier mask of ONE model per pair with the same arithmetic: models fp64 [B][3][3]; mask uint8 [Ptot], 1 where err <= thr2;
 * every point of [offsets[0], offsets[B]) is written.  B == 0 returns without touching anything. */
int gim_ransac_mask(const double* models, const double* x0, const double* x1, const int32_t* offsets, int B, double thr2,
                    uint8_t* mask, gim_stream_t stream);

/* ======================================================================================================
 * Dense SfM: the dense matches of a pair list aggregated into keypoints and keypoint-indexed matches on the device (added
 * within ABI revision 115: no existing structure or prototype changed with it).  The reference does this on the host, one
 * match at a time (hloc/match_dense.py:43-130, 298-419: assign_keypoints, aggregate_matches, assign_matches, kpids_to_matches0).
 *
 * Geometry: patch = max(cell_size, max_error) (an integer), vote = int(max_error), r = patch / vote an integer in 1..8,
 * max_error <= patch / 2 (so 2 <= r), h = (r + 1) / 2, nb = 2 h + 1 bins per axis and cell (r + 1 when r is even).  Per axis and in
 * IEEE fp32 with round-half-to-even, a point x has cell c = rint((x + 0.5) / patch) and bin b = rint((x + 0.5) / vote), b - r c + h
 * in [0, nb); bin index = by * nb + bx.  Every call takes (max_error, patch) and refuses another geometry before it launches.
 * State, all DEVICE memory, indexed by image slot:
 *   geom int32 [n_slots][4] = (W, H, first cell, 0): slot s owns the Gh * Gw cells from its first cell on, raster order (cy * Gw + cx),
 *     Gw = W / patch + 2, Gh = H / patch + 2 (integer division); total_cells = the cells of all slots;
 *   votes uint64 [total_cells][nb * nb] and cell_n int32 [total_cells] (votes per cell), zeroed by the caller before the first vote;
 *   the pool of stored matches kpts0, kpts1 fp32 [pool_rows][2] (pixel coordinates, 8-byte aligned), scores fp32 [pool_rows];
 *   a batch of P pairs: offsets int32 [P + 1] rising pool rows (pair p owns offsets[p] .. offsets[p + 1] - 1), slot0, slot1 int32 [P];
 *   row_lo = offsets[0], row_hi = offsets[P] as the HOST knows them (the launch shape; one lane per row of [row_lo, row_hi)).
 * A match counts iff both slots are usable, its score is finite and in [0, 65536), and both points lie in [-0.5, W - 0.5] x
 * [-0.5, H - 0.5] of their image.  The kernels re-check every slot, cell, bin, id and row against n_slots, total_cells and the offsets
 * and never turn one that does not fit into an address.
 * ====================================================================================================== */

/* nb * nb for (max_error, patch), or 0 for a geometry the calls below refuse (the reason is in gim_last_error). */
int gim_agg_bins(float max_error, int patch);

/* Votes of the batch: every counting match adds llrint(score * 2^32) to its bin's 64-bit sum and 1 to its cell's count, on both sides
 * (ordinary integer atomicAdd: only integer sums cross threads, so the sums do not depend on the launch shape or on the order of the
 * pairs).  dropped int32 [P] is FULLY written: the matches of pair p that did not count. */
int gim_agg_vote(const float* kpts0, const float* kpts1, const float* scores, const int32_t* offsets, const int32_t* slot0,
                 const int32_t* slot1, const int32_t* geom, uint64_t* votes, int32_t* cell_n, int32_t* dropped, int P, int row_lo,
                 int row_hi, int pool_rows, int n_slots, int64_t total_cells, float max_error, int patch, gim_stream_t stream);

/* Per cell (one lane each) the bin with the largest sum; the lowest bin index wins an exact tie.  cell_bin int32 [total_cells] = that bin,
 * -1 for a cell without votes; cell_key int64 [total_cells] = 0 for a cell without votes, else min(sum, 2^63 - 2) + 1: a stable
 * descending sort of a slot's keys is (score descending, raster cell index) with the cells without votes last. */
int gim_agg_finalize(const uint64_t* votes, const int32_t* cell_n, int64_t total_cells, float max_error, int patch, int64_t* cell_key,
                     int32_t* cell_bin, gim_stream_t stream);

/* The final keypoints of all slots from the cells the host selected: sel int32 [n_sel] = cell indices (into [0, total_cells)), the
 * selected cells of slot s at kp_off[s] .. kp_off[s + 1] - 1 in id order (kp_off int32 [n_slots + 1]), sel_slot int32 [n_sel] = the
 * slot of each entry.  Writes id_grid int32 [total_cells] (FULLY: the id of the cell's keypoint within its image, -1 = none),
 * keypoints fp32 [n_sel][2] = b * vote - 0.5, score fp64 [n_sel] = the integer sum * 2^-32, cells int32 [n_sel][2] = (cx, cy).  An
 * entry that does not fit its slot or names a cell without votes writes keypoint (0, 0), score 0, cell (-1, -1) and no id. */
int gim_agg_keypoints(const uint64_t* votes, const int32_t* cell_bin, const int32_t* geom, const int32_t* sel, const int32_t* sel_slot,
                      const int32_t* kp_off, int n_sel, int n_slots, int64_t total_cells, float max_error, int patch, int32_t* id_grid,
                      float* keypoints, double* score, int32_t* cells, gim_stream_t stream);

/* Keypoint-indexed one-to-one matches of a batch of pairs in two launches.  Per counting match and side the keypoint id is, with
 * nearest == 0, the id of the point's own cell (assign_keypoints(update=True)), else that of the nearest final keypoint among the 3 x 3
 * cells around it whose fp64 distance (correctly rounded sqrt) is <= max_error, the lowest id on a tie, -1 when there is none
 * (assign_keypoints(update=False): the KDTree query; max_error <= patch / 2 keeps every candidate within one cell).  Among the matches
 * with both ids a match stays iff it has the best score of its id on BOTH sides (the lowest match index wins equal scores):
 * (score bits << 32) | ~index is maximised per id with 64-bit atomicMax, a second pass keeps the holders of both maxima.
 * koff0, koff1 int32 [P + 1]: prefix sums of the keypoint counts of the pairs' first / second images (rows0 = koff0[P],
 * rows1 = koff1[P]).  FULLY written: matches0 int32 [rows0] (pair p owns koff0[p] .. koff0[p + 1] - 1; -1 = unmatched), scores_f16
 * IEEE fp16 [rows0] (the score rounded to nearest even; 0 = unmatched), row_len int32 [P] = max matched id0 + 1: hloc's matches0 of
 * pair p is its row cut to row_len[p].  ws: gim_agg_assign_ws_bytes(row_hi - row_lo, rows0, rows1) bytes, 8-byte aligned. */
int64_t gim_agg_assign_ws_bytes(int n_rows, int rows0, int rows1);
int gim_agg_assign(const float* kpts0, const float* kpts1, const float* scores, const int32_t* offsets, const int32_t* slot0,
                   const int32_t* slot1, const int32_t* geom, const int32_t* id_grid, const float* keypoints, const int32_t* kp_off,
                   const int32_t* koff0, const int32_t* koff1, int P, int row_lo, int row_hi, int pool_rows, int n_slots,
                   int64_t total_cells, int n_kp, int rows0, int rows1, float max_error, int patch, int nearest, int32_t* matches0,
                   void* scores_f16, int32_t* row_len, void* ws, gim_stream_t stream);

/* ======================================================================================================
 * Feature bank of the dense matchers (gim_dkm, gim_roma): everything match_batch computes from one image is stored once and
 * matched in many pairs (added within ABI revision 115: no existing structure or prototype changed with it).  The reference
 * encodes both images of every pair (networks/dkm/models/dkm.py:572-581, networks/roma/roma.py:668-678).
 * ====================================================================================================== */

#define GIM_DENSE_MAX_LEVELS 8
/* The level table of one gather: level l copies slot_bytes[l] bytes per entry from slab[l] (slots of slot_bytes[l] bytes) to dst[l]
 * (n_entries blocks of slot_bytes[l] bytes).  Entries past n_levels are ignored. */
typedef struct gim_dense_gather_args {
    const void* slab[GIM_DENSE_MAX_LEVELS];
    void* dst[GIM_DENSE_MAX_LEVELS];
    int64_t slot_bytes[GIM_DENSE_MAX_LEVELS];
    int n_levels;
    int pad_;
} gim_dense_gather_args;
/* A whole pyramid of a pair batch in ONE launch: for every level l < n_levels and every entry d < n_entries, block d of dst[l]
 * receives slot idx[d] of slab[l], as 16-byte vector loads and stores.  idx: DEVICE int32 [n_entries], read by the kernel (the host
 * waits for nothing); an index outside [0, n_slots) skips its blocks whole -- nothing is read or written for it.  Every slab has
 * n_slots slots; slabs and destinations are 16-byte aligned and do not overlap, slot_bytes are positive multiples of 16, 1 <=
 * n_levels <= GIM_DENSE_MAX_LEVELS, n_entries <= 65535: anything else returns GIM_ERR_INVALID before the launch. */
int gim_dense_gather_pairs(const gim_dense_gather_args* args, const int32_t* idx, int n_entries, int n_slots, gim_stream_t stream);

/* Geometry of one pair for gim_dense_emit_pairs, all fp32 (sizes are integers below 2^24).  Side 0 / 1 = the model's first / second
 * image, which are the caller's image1 / image0 (hloc/matchers/dkm.py:44-55 matches the pair swapped). */
typedef struct gim_dense_pair_geom {
    float wp0, hp0, wp1, hp1;   /* padded sizes: what the model saw */
    float pl0, pt0, pl1, pt1;   /* left / top padding of get_padding_size */
    float ow0, oh0, ow1, oh1;   /* sizes before padding */
    float sx0, sy0, sx1, sy1;   /* rescale of the OUTPUT keypoints0 / keypoints1 (the caller's image0 / image1) */
} gim_dense_pair_geom;
/* The tail of the hloc dense plugin for B pairs in ONE launch -- hloc/matchers/dkm.py:95-150 + hloc/match_dense.py:242-243.  sparse
 * [B][num][4] normalised matches and mconf [B][num] of RegressionMatcher.sample.  Row r of pair b is kept iff mconf > 0 and its pixel
 * coordinates k = size_padded * (x + 1) / 2 - pad (gim_dense_to_pixels, then the un-padding) satisfy 0 < k <= original size - 1 on
 * both axes of both sides.  Kept rows are written IN INPUT ORDER to the front of keypoints0 [B][num][2] (side 1: the caller's image0),
 * keypoints1 [B][num][2] (side 0) and scores [B][num]; count int32 [B] = kept rows per pair; rows past count are not written.
 * rescale != 0: every output coordinate becomes (k + 0.5) * s - 0.5.  fp32, the operations of the per-pair host path in its order,
 * nothing contracted: the rows equal that path's bit for bit.  One workgroup per pair with a block scan; no atomics. */
int gim_dense_emit_pairs(const float* sparse, const float* mconf, const gim_dense_pair_geom* geom, float* keypoints0, float* keypoints1,
                         float* scores, int32_t* count, int B, int num, int rescale, gim_stream_t stream);

/* RegressionMatcher.sample (dkm.py:583-620, roma.py:680-714; sample_mode 'threshold_balanced') for B pairs in one fixed launch
 * sequence, with no host read: what gim_amd.dense.balanced_sample does per pair with gim_weighted_sample, gim_kde and torch.sort.
 * matches [B][n][4] and certainty [B][n] are the maps of `match`, flattened (n = H * 2W); seeds: HOST uint32 [B][2], the seeds of a
 * pair's two draws (passed to the kernels by value).  Per pair b:
 *   w = certainty > thresh ? 1 : certainty;  n_pos = #(w > 0);  if n_pos == 0: w += 1e-8 and n_pos = n;
 *   first draw:  k1 = min(4 * num, n, n_pos) rows without replacement with probability ~ w (the keys of gim_weighted_sample from
 *                seeds[b][0] and the flat index), kept in ASCENDING FLAT INDEX;
 *   density = kde(rows, std 0.1) (kde_half: on fp16-rounded coordinates), p = density < 10 ? 1e-7 : 1 / (density + 1);
 *   second draw: k2 = min(num, k1) of those rows with probability ~ p (keys from seeds[b][1] and the row's rank), in ascending rank.
 * sparse [B][num][4] / mconf [B][num] (the un-thresholded certainty) hold the k2 rows, ZERO behind them; count int32 [B] = k2.  Every
 * element of the three outputs is written.  The rows are those of the per-pair path for the same seeds, bit for bit and in its order.
 * Keys tied with a draw's threshold key are taken by ascending index, however many there are (the per-pair path falls back to
 * arrival order behind 4096 ties; there the two paths may differ).
 * 1 <= B <= GIM_SAMPLE_MAX_PAIRS, n > 0, num > 0, no NULL pointer, sparse 16-byte aligned: anything else returns GIM_ERR_INVALID
 * before a launch.
 * Workspace (gim_balanced_sample_pairs_ws_bytes, 256-byte aligned base), consecutive regions, each rounded up to 256 bytes, with
 * np = n rounded up to 4, K1 = min(4 * num, n), nb1 = ceil(n / 2048), nb2 = ceil(K1 / 2048):
 *   keys1   uint32 [B][np]     first-draw keys (0: weight <= 0), as gim_weighted_sample leaves them
 *   rows    float  [B][K1][4]  first-draw rows, k1[b] valid
 *   rowcert float  [B][K1]     their certainties
 *   density float  [B][K1]     their KDE densities
 *   keys2   uint32 [B][K1]     second-draw keys
 *   blocks1 int32  [B][nb1][2] scan scratch of the first draw
 *   blocks2 int32  [B][nb2][2] scan scratch of the second draw
 *   hist    uint32 [B][4096]   radix-select histogram
 *   state   int32  [B][16]     n_pos (as counted, before the n_pos == 0 replacement), k1, k2, then scratch */
#define GIM_SAMPLE_MAX_PAIRS 16
int64_t gim_balanced_sample_pairs_ws_bytes(int B, int n, int num);
int gim_balanced_sample_pairs(const float* matches, const float* certainty, const uint32_t* seeds, float* sparse, float* mconf,
                              int32_t* count, void* ws, int B, int n, int num, float thresh, int kde_half, gim_stream_t stream);

/* ======================================================================================================
 * Homography RANSAC step and perspective warp: the last two steps of the reference's demo (added within ABI revision 115: no
 * existing structure or prototype changed with it).  The reference calls cv2.findHomography(mkpts1, mkpts0, ...) and
 * cv2.warpPerspective(img1, H, size of img0) (demo.py:180-227, 230-266).  Sampling, the iteration bound and the final re-fit
 * stay on the host (gim_amd/pose.py); the minimal solve, the sample checks and the scoring are one launch per step.
 * ====================================================================================================== */

/* K four-point hypotheses per pair, solved AND scored in ONE launch, B pairs.  All pointers are DEVICE memory.  src, dst fp64
 * [Ptot][2] (16-byte aligned), the points of the pairs concatenated; offsets int32 [B + 1], non-decreasing: pair b owns the points
 * offsets[b] .. offsets[b + 1] (trusted, as in gim_ransac_score: the caller checks them); idx int32 [B][K][4]: the sample's four
 * point indices RELATIVE to the pair's offset.  fp64 throughout, no fast-math.  The model is dst ~ H src:
 *   * each side's four points are shifted to zero mean and scaled to mean distance sqrt(2);
 *   * the eight equations (x, y, 1, 0, 0, 0, -u x, -u y | u), (0, 0, 0, x, y, 1, -v x, -v y | v) of the normalised correspondences
 *     (x, y) -> (u, v), point-major, are solved for h11 .. h32 with h33 = 1 by Gaussian elimination with partial pivoting on the
 *     8 x 9 augmented system (the first row of the largest magnitude wins a tie);
 *   * H is de-normalised (T_dst^-1 H T_src) and scaled so that h33 = 1 (HomographyEstimatorCallback::runKernel of OpenCV 4.x,
 *     modules/calib3d/src/fundam.cpp, also normalises, de-normalises and scales to h33 = 1; it scales each axis by its mean absolute
 *     deviation and takes the smallest eigenvector of the 9 x 9 normal matrix, this takes Hartley's scaling and the direct solve: no
 *     eigen-decomposition, the same model on exact data).
 * valid[b][k] = 0, counts[b][k] = 0 and an all-zero model are written when
 *   * an index is outside [0, the pair's point count) or the sample repeats an index;
 *   * the four points of a side coincide (no scale);
 *   * any three of the four points of either side are collinear: the doubled area of the triangle, in normalised coordinates,
 *     is below 1e-9 in magnitude (the haveCollinearPoints rule of fundam.cpp, stated on areas);
 *   * the sample fails the orientation test of HomographyEstimatorCallback::checkSubset (fundam.cpp): over the triples (0,1,2),
 *     (1,2,3), (0,2,3), (0,1,3) the sign of the oriented area on the src side differs from the dst side for some but not all four
 *     (none differing, or all four: a reflection, pass -- as OpenCV decides it);
 *   * a pivot of the normalised system is below 1e-12 in magnitude;
 *   * the de-normalised model has an entry that is not finite after the division by h33.
 * Otherwise valid = 1, models fp64 [B][K][3][3] row-major holds H, and counts int32 [B][K] the number of the pair's points with
 *   err = |dst - proj(H src)|^2 <= thr2     (HomographyEstimatorCallback::computeError: the forward transfer error; IEEE division),
 * where a point with w = h31 x + h32 y + h33 == 0 or an error that is not finite is an outlier.  models, valid and counts are FULLY
 * written (no memset by the caller; no atomics: one workgroup owns one hypothesis).  B == 0 or K == 0 returns without touching
 * anything.  B <= 65535. */
int gim_homography_step(const double* src, const double* dst, const int32_t* offsets, int B, const int32_t* idx, int K, double thr2,
                        double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream);
/* The inlier mask of ONE model per pair with the same error: models fp64 [B][3][3]; mask uint8 [Ptot], 1 where err <= thr2 (an
 * all-zero model has w == 0 everywhere: no inlier); every point of [offsets[0], offsets[B]) is written.  B == 0 returns without
 * touching anything. */
int gim_homography_mask(const double* models, const double* src, const double* dst, const int32_t* offsets, int B, double thr2,
                        uint8_t* mask, gim_stream_t stream);

/* Perspective warp, cv2.warpPerspective(src, H, (Wd, Hd)) with INTER_LINEAR and BORDER_CONSTANT 0.  src / dst: DEVICE memory,
 * channels-first contiguous [B][C][Hs][Ws] / [B][C][Hd][Wd] of uint8 (dtype 0) or fp32 (dtype 1; pixel kinds of this call alone,
 * not the GIM_F32 / GIM_BF16 / GIM_F16 tags; another value is refused), 1 <= C <= 4; Hmat fp64 [B][3][3]
 * DEVICE memory, row-major: H maps src pixels to dst pixels.  The destination pixel (x, y), integer pixel centres, reads
 *   (u, v) = proj(H^-1 (x, y, 1))   in fp64, H^-1 taken as the adjugate of H (the projection does not see the factor 1 / det),
 *   dst = sum over the four neighbours (x0 + i, y0 + j), x0 = floor(u), y0 = floor(v), of weight_ij * src, a neighbour outside the
 *   source contributing 0; the weights (1 - ax | ax)(1 - ay | ay) are formed in fp64, rounded once to fp32, and blended in fp32
 *   (four products, three additions).  The result is a continuous function of (u, v).  w == 0 or a coordinate that is not finite: 0.
 * uint8 stores rint (to nearest even) of the fp32 value, saturated.  cv2 interpolates with 5-bit fixed-point weights (INTER_BITS); this
 * is the exact-weight operator and is compared against its own formula, not against cv2's bytes.  The caller rejects a singular
 * H (det == 0) or one with an entry that is not finite before the call (ops.warp_perspective, on the host); the kernel does not
 * check again: such an H gives an image without meaning, never an access outside src or dst.  B == 0 or an empty destination returns without touching anything. */
int gim_warp_perspective(const void* src, int dtype, int B, int C, int Hs, int Ws, const double* Hmat, void* dst, int Hd, int Wd,
                         gim_stream_t stream);

/* ======================================================================================================
 * Fundamental-matrix RANSAC step: the seven-point minimal solve and the scoring of its models in one launch (added within ABI
 * revision 115: no existing structure or prototype changed with it).  The reference calls cv2.findFundamentalMat(mkpts0, mkpts1,
 * ...) (demo.py:514-517).  Sampling and the iteration bound stay on the host (gim_amd/pose.py); the final mask is gim_ransac_mask,
 * the same Sampson error.  The five-point solver (a 10 x 10 non-symmetric eigenproblem) is gim_essential_step, below.
 * ====================================================================================================== */

/* K seven-point samples per pair, solved AND scored in ONE launch, B pairs; a sample gives up to three models.  All pointers are
 * DEVICE memory.  x0, x1 fp64 [Ptot][2] (16-byte aligned), the points of the pairs concatenated; offsets int32 [B + 1],
 * non-decreasing: pair b owns the points offsets[b] .. offsets[b + 1] (trusted, as in gim_ransac_score: the caller checks them); idx
 * int32 [B][K][7]: the sample's seven point indices RELATIVE to the pair's offset.  fp64 throughout, no fast-math.  The model is
 * x1^T F x0 = 0 (pose.seven_point_ge is this arithmetic in batched numpy, csrc/fundamental_solve.h the code):
 *   * normalisation: each side's seven points are shifted to zero mean (sum in index order, divided by 7) and scaled to mean distance
 *     sqrt(2); a side whose mean distance is below 1e-12 (seven coincident points) or not finite is invalid;
 *   * null space: the 7 x 9 rows (u x, u y, u, v x, v y, v, x, y, 1) of the normalised correspondences (x, y) -> (u, v) (the column
 *     order of pose._epipolar_rows) are reduced by Gauss-Jordan elimination with FULL pivoting: step k takes the largest |a| over the
 *     rows k .. 6 and all columns (the lowest row, then the lowest column, wins a tie), swaps that row into place, divides it by the
 *     pivot and eliminates the pivot column from the six other rows.  A zero pivot, or a seventh pivot below 1e-12 times the first,
 *     is a rank-deficient sample (collinear points, a planar scene).  The two free columns f1 < f2 give the basis: F1 has 1 in
 *     column f1, 0 in f2 and minus the reduced row's entry of column f1 in each pivot column; F2 likewise for f2;
 *   * cubic: det(a F1 + (1 - a) F2) = c0 + c1 a + c2 a^2 + c3 a^3 is interpolated at a = 0, 1, -1, 2 (determinants by cofactors of
 *     the first row).  A sample with max |c| < 1e-12 is invalid: every matrix of the pencil is singular (three matches that share a
 *     point on one side do that) and the cubic is rounding noise, which pose.seven_point's relative rule does not see.  A sample
 *     with |c3| <= 1e-14 (max |c| + 1e-300) is invalid (pose.seven_point's rule);
 *   * roots: with b = c / c3 and a = t - b2 / 3 the depressed cubic is t^3 + p t + q; D = (q/2)^2 + (p/3)^3 > 0 gives one real root
 *     by Cardano (u the cube root without cancellation, v = -p / (3 u)), D <= 0 three by the trigonometric form
 *     t_k = 2 sqrt(-p/3) cos(acos(-(q/2) / sqrt(-p/3)^3) / 3 - 2 pi k / 3); every root gets two Newton steps on
 *     a^3 + b2 a^2 + b1 a + b0 and the roots are ordered ascending into the slots 0, 1, 2.  A sample with |D| within 1e-9 of
 *     (q/2)^2 + |p/3|^3 is ambiguous between one root and three; it is solved as D decides;
 *   * output: each root gives T1^T (a F1 + (1 - a) F2) T0, scaled to unit Frobenius norm; a norm that is zero or not finite is
 *     invalid.
 * An index outside [0, the pair's point count) or a repeated index invalidates the whole sample and never becomes an address.
 * models fp64 [B][K][3][3][3] row-major, valid uint8 [B][K][3] and counts int32 [B][K][3] are FULLY written (no memset by the caller;
 * no atomics: one workgroup owns one sample): an invalid or unused slot holds a zero matrix, valid 0 and count 0; a valid one the
 * number of the pair's points with
 *   err = (x1^T F x0)^2 / max(|F x0|_xy^2 + |F^T x1|_xy^2, 1e-300) <= thr2     (the arithmetic and operation order of gim_ransac_score).
 * B == 0 or K == 0 returns without touching anything.  Refused before a launch: a NULL pointer, x0 / x1 not 16-byte aligned, models
 * not 8-byte or an int32 array not 4-byte aligned, B > 65535, B * K * 27 > INT32_MAX. */
int gim_fundamental_step(const double* x0, const double* x1, const int32_t* offsets, int B, const int32_t* idx, int K, double thr2,
                         double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream);

/* ======================================================================================================
 * Essential-matrix RANSAC step: the five-point minimal solve and the scoring of its models in one launch (added within ABI
 * revision 115: no existing structure or prototype changed with it).  The reference calls cv2.findEssentialMat(kpts0, kpts1,
 * np.eye(3), threshold, prob, method=cv2.RANSAC) (tools/metrics.py:88-89).  The iteration bound stays on the host
 * (gim_amd/pose.py); sampling has gim_ransac_sample and recoverPose gim_recover_pose, below; the final mask is gim_ransac_mask, the
 * same Sampson error.
 * ====================================================================================================== */

/* K five-point samples per pair, solved AND scored in ONE launch, B pairs; a sample gives up to ten models.  All pointers are
 * DEVICE memory.  x0, x1 fp64 [Ptot][2] (16-byte aligned), the points of the pairs concatenated, in normalised camera coordinates
 * (they are used as they are: no Hartley normalisation, as in pose.five_point); offsets int32 [B + 1], non-decreasing: pair b owns
 * the points offsets[b] .. offsets[b + 1] (trusted, as in gim_ransac_score: the caller checks them); idx int32 [B][K][5]: the sample's
 * five point indices RELATIVE to the pair's offset.  fp64 throughout, real arithmetic only, no fast-math, every loop bounded.  The
 * model is x1^T E x0 = 0 (pose.five_point_ge is this arithmetic in numpy, csrc/essential_solve.h the code):
 *   1. null space: the 5 x 9 rows (u x, u y, u, v x, v y, v, x, y, 1) of the correspondences (x, y) -> (u, v) (the column order of
 *      pose._epipolar_rows) are reduced by Gauss-Jordan elimination with FULL pivoting, as in gim_fundamental_step.  A coordinate
 *      that is not finite, a zero pivot, or a fifth pivot below 1e-12 times the first (a repeated correspondence, coincident points)
 *      refuses the sample.  The four free columns f0 < f1 < f2 < f3 give the basis X, Y, Z, W: 1 in its own free column, 0 in the
 *      other free columns, minus the reduced row's entry of its free column in each pivot column;
 *   2. constraints: det E = 0 and the nine entries of 2 E E^T E - tr(E E^T) E on E = x X + y Y + z Z + W, as coefficients over the
 *      20 monomials of pose._MONO, rows in the order pose.five_point stacks them.  E E^T (six polynomials of degree 2) and the 2 x 2
 *      minors are sums of products of two entries, each product accumulated over the 16 coefficient pairs in row-major order; a
 *      row is the sum of its (degree 2) x (entry) products, each accumulated over the 40 coefficient pairs in row-major order;
 *      a row of the second kind is doubled before tr(E E^T) e_ij is subtracted;
 *   3. reduction: Gauss-Jordan with PARTIAL pivoting (the first row of the largest magnitude) on the 10 x 10 block of the cubic
 *      monomials gives [I | B].  A pivot below 1e-12 times the largest |entry| of the 10 x 20 matrix, or an entry that is not
 *      finite, refuses the sample;
 *   4. eigenvalues: the 10 x 10 action matrix of multiplication by x on (x2, xy, xz, y2, yz, z2, x, y, z, 1) -- rows 0 .. 5 are
 *      -B's, rows 6 .. 9 pick x2, xy, xz, x -- is brought to Hessenberg form by Householder reflections (EISPACK orthes) and its
 *      eigenvalues found by the real Francis double-shift QR iteration (EISPACK hqr, eigenvalues only; deflation tests
 *      |h| <= 2^-52 s): at most 30 sweeps per eigenvalue, exceptional shifts at sweeps 10 and 20.  A 2 x 2 block with a negative
 *      discriminant is a complex pair and gives no model; if a sweep count runs out, the eigenvalues not yet found give none.  The
 *      real eigenvalues, ascending, fill the slots 0, 1, ...;
 *   5. models: per real eigenvalue x the null vector v of (action matrix - x I) by Gauss-Jordan elimination with full pivoting
 *      (nine steps, the free column is 1); a zero pivot or |v[9]| <= 1e-14 max |v| refuses the slot (pose.five_point's rule);
 *      (x, y, z) = v[6..8] / v[9]; E = ((x X + y Y) + z Z) + W over its Frobenius norm; a norm that is zero or not finite
 *      refuses the slot.
 * An index outside [0, the pair's point count) or a repeated index invalidates the whole sample and never becomes an address.
 * models fp64 [B][K][10][3][3] row-major, valid uint8 [B][K][10] and counts int32 [B][K][10] are FULLY written (no memset by the
 * caller; no atomics: one workgroup owns one sample): an invalid or unused slot holds a zero matrix, valid 0 and count 0; a valid
 * one the number of the pair's points with
 *   err = (x1^T E x0)^2 / max(|E x0|_xy^2 + |E^T x1|_xy^2, 1e-300) <= thr2     (the arithmetic and operation order of gim_ransac_score).
 * B == 0 or K == 0 returns without touching anything.  Refused before a launch: a NULL pointer, x0 / x1 not 16-byte aligned, models
 * not 8-byte or an int32 array not 4-byte aligned, B > 65535, B * K * 90 > INT32_MAX. */
int gim_essential_step(const double* x0, const double* x1, const int32_t* offsets, int B, const int32_t* idx, int K, double thr2,
                       double* models, uint8_t* valid, int32_t* counts, gim_stream_t stream);

/* ======================================================================================================
 * RANSAC on the device: the sampler and the reduction of a step to its record samples (added within ABI revision 115: no
 * existing structure or prototype changed with it).  Together with one of the three step entry points above they make a RANSAC
 * step three launches whose only host traffic is 3 B integers up and the records down; the reference draws its samples and keeps
 * its best model inside OpenCV (RANSACPointSetRegistrator::run, cv::RNG), on the host.  Integer arithmetic only in both.
 * ====================================================================================================== */

/* The sample indices of one step of B pairs in ONE launch.  All pointers are DEVICE memory.  offsets int32 [B + 1], non-decreasing
 * (trusted, as in gim_ransac_score): pair b has P_b = offsets[b + 1] - offsets[b] points; first int64 [B] (8-byte aligned): the
 * ordinal of the pair's first sample of this step; count int32 [B]: the samples the pair uses this step; m in {4, 5, 7}.  Slot s
 * of pair b holds sample number n = first[b] + s of the pair's run, a function of (seed, n, P_b, m) alone (csrc/ransac_sample.h is
 * the code, pose.device_samples the numpy restatement):
 *   words    Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, key (seed & 0xffffffff,
 *            seed >> 32), counter (n & 0xffffffff, n >> 32, blk, 0); r[0..7] = the four words of blk 0, then those of blk 1;
 *   indices  Floyd's algorithm, exactly m draws, no retry: for i = 0 .. m-1: j = P_b - m + i, t = (r[i] * (j + 1)) >> 32;
 *            idx[i] = t unless t occurs in idx[0 .. i-1], then idx[i] = j.  m distinct indices of [0, P_b); the set is uniform over
 *            the m-subsets up to the multiply-shift bias, at most (j + 1) / 2^32 relative per draw; the order inside a sample is not
 *            uniform.
 * idx int32 [B][K][m] is FULLY written: slot s >= count[b], and every slot of a pair with P_b < m, holds -1 in all m places (the
 * step entry points treat -1 as padding).  One lane per sample, plain per-lane stores, no atomics.  B == 0 or K == 0 returns
 * without touching anything.  Refused before a launch: m outside {4, 5, 7}, a NULL pointer, first not 8-byte or an int32 array not
 * 4-byte aligned, B > 65535, B * K * m > INT32_MAX. */
int gim_ransac_sample(const int32_t* offsets, int B, const int64_t* first, const int32_t* count, int K, int m, uint64_t seed,
                      int32_t* idx, gim_stream_t stream);

/* The samples of a step that set a new strict maximum of the inlier count, per pair, in sample order: the only ones the RANSAC
 * bookkeeping acts on.  All pointers are DEVICE memory.  counts int32 [B][K][k], k in {1, 3, 10}: the counts output of
 * gim_homography_step / gim_fundamental_step / gim_essential_step; nb int32 [B]: the samples in use this step (clamped to [0, K]);
 * floor_ int32 [B]: the count to beat, max(best so far, m - 1).  For s < nb[b]: c_s = the largest of the sample's k counts, j_s the
 * lowest slot that holds it (numpy's argmax); s is a record iff c_s > max(floor_[b], c_0 .. c_{s-1}).
 * rec int32 [B][1 + 3 K]: rec[b][0] = the number of records n_rec, then the triples (s, j_s, c_s) in ascending s; the words
 * beyond the last triple are NOT written.  One workgroup per pair, prefix maximum and ordered compaction through wave shuffles and
 * LDS, no atomics: the output does not depend on the launch shape.  (pose.step_records is the numpy restatement.)
 * B == 0 returns without touching anything; K == 0 writes n_rec = 0.  Refused before a launch: k outside {1, 3, 10}, a NULL
 * pointer, an array not 4-byte aligned, B > 65535, B * K * k or B * (1 + 3 K) > INT32_MAX. */
int gim_ransac_records(const int32_t* counts, const int32_t* nb, const int32_t* floor_, int B, int K, int k, int32_t* rec,
                       gim_stream_t stream);

/* ======================================================================================================
 * recoverPose on the device (added within ABI revision 115: no existing structure or prototype changed with it).  The reference
 * calls cv2.recoverPose(E, kpts0, kpts1, np.eye(3), 1e9, mask=mask) on the host after its RANSAC (tools/metrics.py:96-101); here
 * the points are those the step entry points above already hold and the input mask is gim_ransac_mask's output.
 * ====================================================================================================== */

/* cv::recoverPose for B pairs in ONE launch.  All pointers are DEVICE memory.  E fp64 [B][3][3] row-major (x1^T E x0 = 0); x0, x1
 * fp64 [Ptot][2] (16-byte aligned) and offsets int32 [B + 1] as in gim_essential_step (trusted); mask_in uint8 [Ptot] or NULL: a
 * point with a zero byte is good under no candidate.  fp64 throughout, real arithmetic only, no fast-math, every loop bounded
 * (pose.recover_pose_ge is this arithmetic in numpy, csrc/recover_pose_solve.h the code):
 *   1. decomposition: e = E / max |E_ij|; the eigenvectors of e^T e by cyclic Jacobi (8 sweeps over the planes (0,1), (0,2), (1,2),
 *      Rutishauser's rotation, a zero off-diagonal entry is skipped), ordered by eigenvalue, largest first; v0 normalised, v1
 *      orthogonalised against v0 and normalised, v2 = v0 x v1; u0 = e v0 / |e v0|, u1 = e v1 orthogonalised against u0 and
 *      normalised (when it vanishes, a rank-one E: u0 x the axis of u0's smallest |entry|), u2 = u0 x u1: det U = det V = +1, the
 *      signs cv::decomposeEssentialMat forces.  With W = [[0,1,0],[-1,0,0],[0,0,1]]: R1 = U W V^T, R2 = U W^T V^T, t = u2; the
 *      candidates, in order: (R1, t), (R2, t), (R1, -t), (R2, -t).  The SVD is not unique: R1 and R2 may be exchanged and t negated
 *      relative to LAPACK's, the SET of four candidates is the same;
 *   2. per point and candidate: the 4 x 4 DLT matrix of cv::triangulatePoints with P0 = [I | 0], P1 = [R | t], rows
 *      x P0[2] - P0[0], y P0[2] - P0[1], u P1[2] - P1[0], v P1[2] - P1[1]; its null vector Q: the eigenvector of the smallest
 *      eigenvalue of A^T A by cyclic Jacobi (8 sweeps over the six planes in row-major order; the first smallest diagonal entry);
 *      w = Q[3] where |Q[3]| > 1e-300, else 1e-300; X = Q[:3] / w; z0 = X[2]; z1 = (R[2] . X) + t[2];
 *      good iff mask_in allows the point and 0 < z0 < distance_thresh and 0 < z1 < distance_thresh;
 *   3. n_good int32 [B][4]: the good points per candidate (integer sums through wave shuffles and LDS, no atomics: the result does
 *      not depend on the launch shape); best int32 [B]: the first maximum in candidate order; R fp64 [B][3][3], t fp64 [B][3]: the
 *      winner's; mask_out uint8 [Ptot]: 1 where the point is good under the winner, else 0.
 * Everything is FULLY written for every pair (no memset by the caller).  An E[b] with an entry that is not finite, or all zero:
 * n_good = 0, best = -1, R = 0, t = 0, the pair's mask_out 0.  A pair without points: n_good = 0, best = 0, R and t of the first
 * candidate.  B == 0 returns without touching anything.  Refused before a launch: a NULL pointer other than mask_in, x0 / x1 not
 * 16-byte aligned, E / R / t not 8-byte or an int32 array not 4-byte aligned, B > 65535. */
int gim_recover_pose(const double* E, const double* x0, const double* x1, const int32_t* offsets, int B, const uint8_t* mask_in,
                     double distance_thresh, double* R, double* t, int32_t* n_good, int32_t* best, uint8_t* mask_out,
                     gim_stream_t stream);

/* ======================================================================================================
 * Least-squares refit of H and F on their inliers, and local optimisation (added within ABI revision 115: no existing structure or
 * prototype changed with it).  The reference filters matches with cv2.findHomography(..., USAC_MAGSAC, ...) (demo.py:197-217) and
 * cv2.findFundamentalMat(..., USAC_MAGSAC, ...) (demo.py:514-517, datasets/walk/walk.py:295); both end with a least-squares fit on
 * the inliers (HomographyEstimatorCallback::runKernel, run8Point: A^T A and its eigenvectors).  Here the points are those the step
 * entry points above already hold.  MAGSAC's scoring and findHomography's Levenberg-Marquardt polish are not built.
 * ====================================================================================================== */

/* Refit of one model per pair for B pairs in ONE launch, one workgroup of 256 lanes per pair.  All pointers are DEVICE memory.
 * kind 0: homographies, b ~ H a (normalised DLT, the forward transfer error of gim_homography_mask); kind 1: fundamental matrices,
 * b^T F a = 0 (normalised eight-point algorithm with rank 2 enforced, the Sampson error of gim_ransac_mask).  a, b fp64 [Ptot][2]
 * (16-byte aligned) and offsets int32 [B + 1] as in gim_homography_step / gim_fundamental_step (trusted); models_in fp64 [B][3][3]
 * row-major; mask_in uint8 [Ptot] (a non-zero byte: an inlier; it must not overlap mask_out) or NULL: the starting mask is
 * models_in's own under thr2; 1 <= rounds <= 8.  fp64 throughout, real arithmetic only, no fast-math, no atomics, every loop
 * bounded (pose.refit_ge is this arithmetic in numpy, csrc/model_refit_solve.h the code).  The current model starts as models_in[b],
 * the current mask as the starting mask; up to `rounds` times:
 *   1. fewer current inliers than 4 (kind 0) or 8 (kind 1), or an inlier coordinate that is not finite: stop;
 *   2. Hartley's normalisation of both sides over the inliers: centre = sum / n, then scale = sqrt(2) / (sum of the distances to the
 *      centre / n); a mean distance that is zero or not finite: stop;
 *   3. the 45 upper-triangle entries of A^T A: kind 0 two rows per inlier, (x, y, 1, 0, 0, 0, -u x, -u y, -u) and (0, 0, 0, x, y,
 *      1, -v x, -v y, -v); kind 1 one row, (u x, u y, u, v x, v y, v, x, y, 1), with (x, y) / (u, v) the normalised point of a / b.
 *      Every sum over the inliers (here and in 2) has ONE order: lane l adds its points l, l + 256, ... ascending, the 64 lanes of a
 *      wave are combined by the tree x[l] += x[l + o], o = 32, 16, .., 1, the four wave totals are added in wave order -- a pair's
 *      result depends neither on B nor on its place in the batch;
 *   4. the eigenvector of the smallest eigenvalue (the first smallest diagonal entry) by cyclic Jacobi, 8 sweeps over the 36 planes
 *      in row-major order, Rutishauser's rotation, a zero off-diagonal entry skipped;
 *   5. kind 1: f - (f v2) v2^T with v2 the unit eigenvector of the smallest eigenvalue of f^T f (the 3 x 3 Jacobi iteration of
 *      gim_recover_pose): the smallest singular value set to zero;
 *   6. de-normalised with T = [s, 0, -s cx; 0, s, -s cy; 0, 0, 1]: kind 0 Tb^-1 h Ta scaled to h33 = 1, kind 1 Tb^T f Ta scaled to
 *      unit Frobenius norm; a result that is not finite, a zero norm or h33 == 0: stop;
 *   7. the candidate's mask over every point of the pair, with the error and the comparison of gim_homography_mask (kind 0) or
 *      gim_ransac_mask (kind 1), and its count.  The candidate replaces the current model and mask iff its count is not below the
 *      current count; a rejected candidate stops the loop; a candidate whose mask equals the current mask byte for byte is accepted
 *      and then stops the loop (a fixed point).
 * models_out fp64 [B][3][3]: the last accepted candidate, or models_in[b] when none was; mask_out uint8 [Ptot]: the current mask
 * at the end, 0 / 1; counts int32 [B][2]: the inliers of the starting mask and of mask_out; accepted int32 [B]: the candidates
 * accepted.  Everything is FULLY written for every pair (no memset by the caller), nothing outside [offsets[0], offsets[B]) of
 * mask_out.  A models_in[b] with an entry that is not finite, or all zero: the pair is skipped -- models_out = 0, its mask_out 0,
 * counts 0, accepted = -1.  B == 0 returns without touching anything.  Refused before a launch: kind outside {0, 1}, rounds outside
 * 1 .. 8, a NULL pointer other than mask_in, a / b not 16-byte aligned, models_in / models_out not 8-byte or an int32 array not
 * 4-byte aligned, B > 65535. */
int gim_model_refit(int kind, const double* a, const double* b, const int32_t* offsets, int B, const double* models_in,
                    const uint8_t* mask_in, double thr2, int rounds, double* models_out, uint8_t* mask_out, int32_t* counts,
                    int32_t* accepted, gim_stream_t stream);

/* ======================================================================================================
 * Video pseudo-labels (added within ABI revision 115: no existing structure or prototype changed with them).  A label is an fp32
 * [n][4] array of matches (x0, y0, x1, y1) between two frames.  The reference links the labels of frames a->b and b->c into a->c
 * through the pixels they share in b (datasets/walk/walk.py:29 create_table, :217-247 link, with Python dicts and sets on DataLoader
 * workers) and writes a label at the end of a labelling step (video_preprocessor.py:513-555).  csrc/label_key.h is the arithmetic,
 * gim_amd/video_labels.py (link_tables, label_pack_np) its numpy restatement.
 * ====================================================================================================== */

/* bytes of gim_label_link's workspace: two int32 tables of max_keys slots per link; -1 for a negative argument.  max_keys is the
 * largest w * (h + 1) + 1 of the links it will serve. */
int64_t gim_label_link_ws_bytes(int B, int max_keys);

/* walk.py:link for B links in one launch sequence (three launches: build, compact, clear).
 * DEVICE memory: lab0 fp32 [n0_total][4], lab1 fp32 [n1_total][4] (16-byte aligned): the links' labels, concatenated; off0, off1
 * int32 [B + 1]: ascending row offsets of the links in the two slabs (clamped into them), or NULL when B == 1: the whole slab;
 * wh_dev int32 [B][2]: (width, height) per link, or NULL when B == 1; ws: gim_label_link_ws_bytes(B, max_keys) bytes, ALL ZERO on
 * entry and all zero again when the sequence has run (the last launch clears exactly the slots the first one wrote; nobody pays a
 * memset of the key range).  HOST memory: wh int32 [B][2], the same values as wh_dev: they are checked before anything is launched.
 *   key      of a point (x, y) of link b: rintf(x) + rintf(y) * (float)w in fp32, round half to even, no fused multiply-add
 *            (create_table: np.round(x) + np.round(y) * w).  lab0's point is its columns 2, 3, lab1's its columns 0, 1 -- the pixels
 *            of the middle frame.  A key is usable iff it is finite and in [0, w * (h + 1)]: this keeps the reference's aliasing (an
 *            x that rounds to w shares the key of (0, y + 1)).  Rows without a usable key are ignored and counted in dropped[b][side]
 *            -- the one difference from the reference, which would join them too;
 *   tables   per link and side, over the key range: the LARGEST row index of the link that has the key, stored as index + 1
 *            (integer atomicMax; dict(zip(keys, range(n))) keeps the last row of a key);
 *   result   row i of the link's lab0 rows survives iff table0[key_i] == i + 1 and table1[key_i] > 0; its partner is
 *            j = table1[key_i] - 1.  Survivors in ascending i -- np.unique(np.vstack((i, j)), axis=1) of walk.py:240, where distinct
 *            keys have distinct i -- placed by a block scan with a carried offset, one workgroup per link, no atomics:
 *            out fp32 [n0_total][4]: row off0[b] + rank = (lab0[i][0:2], lab1[j][2:4]), copied bit for bit; ij int32 [n0_total][2]:
 *            (i, j) relative to the link's rows; count int32 [B]; dropped int32 [B][2].  Nothing is written beyond count[b] rows of
 *            a link or outside its row range.
 * B == 0 returns without touching anything.  Refused before a launch (GIM_ERR_INVALID): B < 0 or > 65535, a negative row count,
 * a width or height < 1, a key range w * (h + 1) above 2^24 (keys are exact in fp32 up to there) or not below max_keys, B > 1
 * without offsets or wh_dev, a NULL or misaligned pointer. */
int gim_label_link(const float* lab0, const int32_t* off0, int n0_total, const float* lab1, const int32_t* off1, int n1_total,
                   const int32_t* wh, const int32_t* wh_dev, int B, int max_keys, void* ws, float* out, int32_t* ij,
                   int32_t* count, int32_t* dropped, gim_stream_t stream);

/* The tail of a labelling step for one pair in ONE launch (one workgroup, the same ordered compaction).  DEVICE memory: k0, k1 fp32
 * [n][2] (8-byte aligned): the matched keypoints; keep uint8 [n] or NULL; out fp32 [n][4] (16-byte aligned); count int32 [1].
 * HOST memory: affine, 8 doubles (sx0, sy0, ox0, oy0, sx1, sy1, ox1, oy1), or NULL.
 *   kept     iff (keep is NULL or keep[i] != 0) and (moved_thr <= 0 or not (|x0 - x1| < moved_thr and |y0 - y1| < moved_thr)), the
 *            differences in fp32: video_preprocessor.py:516, the watermark test; a NaN row counts as moved;
 *   row      with an affine: ((double)x * s + o) * vratio in fp64, three roundings, no fused multiply-add, then to fp32 (line 549);
 *            without: the fp32 product x * (float)vratio (line 552);
 *   out      the kept rows in input order, count[0] of them; nothing is written beyond.
 * Refused before a launch: n < 0, a NULL pointer (other than keep and affine; k0, k1, out may be NULL when n == 0), misalignment. */
int gim_label_pack(const float* k0, const float* k1, const uint8_t* keep, int n, float moved_thr, const double* affine,
                   double vratio, float* out, int32_t* count, gim_stream_t stream);

/* ======================================================================================================
 * Frame preparation of the video labeller (added within ABI revision 115: no existing structure or prototype changed with it).
 * The reference prepares both frames of a pair on the host with OpenCV: the crop to the box of the previous pass's labels and the
 * INTER_AREA resize (video_preprocessor.py:292-304, :318-329), the class map resized to the frame, cropped and resized to the
 * output with INTER_NEAREST (:342-354), the exclusion mask (:359-365), the per-method tensors (:406-493: gim_dkm's masked colour
 * image, LoFTR's grey and colour images and its 1/8 mask, gim_lightglue's masked grey image) and the segmenter's input
 * (:603-621 read_segmentation_image).  csrc/frame_prep_math.h is the arithmetic, gim_amd/frame_prep.py (frame_prep_np) its numpy
 * restatement.  The contract below is NOT byte-equality with cv2.resize: OpenCV rounds 1 / (dst / src) in double before the floor of
 * its nearest-neighbour index and has a separate integer-factor path for bytes.
 * ====================================================================================================== */

/* The output tile (tw x th pixels, at most 64 x 16) gim_frame_prep wants for a job that resizes a crop of wc x hc pixels to wn x hn:
 * the largest one, halving th and then tw, whose source footprint fits the kernel's 40 KiB of LDS.  Refused: an extent < 1, an axis
 * shrunk by more than 16. */
int gim_frame_prep_tile(int wc, int hc, int wn, int hn, int* tw, int* th);

/* J jobs in ONE launch, one workgroup of 256 lanes per work item (a tile of a job's output).
 * DEVICE memory: frames uint8 [S][H][W][3] RGB (16-byte aligned); seg uint8 [S][Hs][Ws] class maps (NULL when no job needs a mask
 * and kept is NULL); exclude uint8 [256] (16-byte aligned), non-zero: the class is excluded; jobs_dev int64 [J][16]; work_dev int32
 * [n_work][4] (16-byte aligned): (job, tile x origin, tile y origin, 0); the output buffers, each NULL when no job asks for it.
 * HOST memory: jobs and work, the same values: they are checked before anything is launched; out_elems int64 [6]: the elements of
 * the six output buffers in the order of the flags.
 *   job      words: slot, x0, y0, x1, y1 (the crop box, wc = x1 - x0, hc = y1 - y0), wn, hn (the output size), flags, the element
 *            offsets of the job's u8, mask, mask8, rgb, gray and norm outputs in their buffers, tw, th (gim_frame_prep_tile).
 *   flags    1 u8, 2 mask, 4 mask8, 8 rgb, 16 gray, 32 norm: the outputs the job writes; 64: rgb and gray are multiplied by the mask.
 *   resize   per axis with source extent n and destination extent m, s = n / m in double: destination index d covers [a, b) with
 *            a = d s, b = min((d + 1) s, n); source index k from floor(a) to ceil(b) - 1 has the weight
 *            (float)((min(b, k + 1) - max(a, k)) / (b - a)), a double expression rounded once.  Per channel
 *            t_y = sum_k wx_k * (float)src[y][k] and v = sum_y wy_y * t_y in fp32 from 0, k and y ascending, every product and sum
 *            rounded separately (no fused multiply-add); the byte is rintf(v) clamped to [0, 255].  For s < 1 this is the coverage
 *            rule INTER_AREA applies when it zooms, for an integer s the mean.
 *   mask     1 where exclude[seg[slot][sy][sx]] == 0, else 0, with cx = x0 + min(j wc / wn, wc - 1), sx = min(cx Ws / W, Ws - 1)
 *            in integers (floors), rows likewise: the reference's resize to the frame, crop and resize to the output.
 *   outputs  u8 uint8 [hn][wn][3]: the resized crop; mask uint8 [hn][wn]; mask8 uint8 [hn / 8][wn / 8] = mask[8 i][8 j]
 *            (cv2.resize(fx = fy = 1/8, INTER_NEAREST)); rgb fp32 [3][hn][wn] = (float)(u8 * m) / 255.f; gray fp32 [hn][wn] =
 *            (float)(g * m) / 255.f with g = (4899 r + 9617 g + 1868 b + 8192) >> 14 on the resized bytes; m = mask under flag 64,
 *            else 1; norm fp32 [3][hn][wn] = ((float)u8 / 255.f - mean) / std with the ImageNet constants, never masked;
 *            kept int32 [J] or NULL: the sum of the job's mask (the reference skips a pair when it is 0) -- set to zero by a
 *            memset on the stream, then integer sums over a wave and one integer atomic per wave.
 * Nothing is written outside a job's ranges.  J == 0 or n_work == 0 returns without touching anything.  Refused before a launch
 * (GIM_ERR_INVALID): a NULL or misaligned pointer, a slot outside [0, S), a box that is empty or leaves the frame, an output extent
 * < 1, an axis shrunk by more than 16, unknown flags, mask8 with hn or wn no multiple of 8, a tile that does not fit, an output that
 * is asked for without a buffer or leaves it, a mask without class maps, a work item outside its job or off the tile grid. */
int gim_frame_prep(const uint8_t* frames, int S, int H, int W, const uint8_t* seg, int Hs, int Ws, const uint8_t* exclude,
                   const int64_t* jobs, const int64_t* jobs_dev, int J, const int32_t* work, const int32_t* work_dev, int n_work,
                   const int64_t* out_elems, uint8_t* out_u8, uint8_t* out_mask, uint8_t* out_mask8, float* out_rgb,
                   float* out_gray, float* out_norm, int32_t* kept, gim_stream_t stream);

/* ======================================================================================================
 * MAGSAC++ scoring of RANSAC hypotheses (added within ABI revision 115: no existing structure or prototype changed with it).
 * The reference filters matches with cv2.USAC_MAGSAC (demo.py:197-217 and :514-517, video_preprocessor.py:578,
 * datasets/walk/walk.py:295); this is the published loss (Barath et al., CVPR 2020), pinned by the contract below, a numpy oracle
 * (pose.magsac_gain / pose.magsac_quality) and an independent special-function library -- no claim of byte-equality with cv2.
 * ====================================================================================================== */

/* Quality and inlier count of K candidate 3x3 models per pair over that pair's points, B pairs in ONE launch.  All pointers are
 * DEVICE memory; models, valid, a, b, offsets as in gim_ransac_score (a = x0 / src, b = x1 / dst).  kind 1: the Sampson error with
 * the expressions and operation order of gim_ransac_score; kind 0: the forward transfer error b ~ M a with those of
 * gim_homography_mask (w == 0 or an error that is not finite: no inlier, no gain).  For a point with squared residual r2:
 *   sigma = max_threshold / 3.64,  u = r2 / (2 sigma^2) = r2 / (max_thr2 / u_k),  t = sqrt(u),  u_k = 3.64^2 / 2
 *   G_k  = Gamma(3/2, u_k) = 0.0036572608340910747  (upper incomplete gamma)
 *   g_k  = gamma(5/2, u_k) = 1.3012265540498873     (lower incomplete gamma)
 *   N(u) = (3 sqrt(pi)/4) erf(t) - 1.5 t exp(-u) + (sqrt(pi)/2) u erfc(t) - u G_k  = gamma(5/2, u) + u (Gamma(3/2, u) - G_k)
 *   gain(u) = 1 - N(u) / g_k clamped to [0, 1] for 0 <= u < u_k and r2 finite, 0 otherwise
 * (the paper's rho(r) for n = 4 degrees of freedom and k = 3.64 up to the factor that cancels in the ratio; gain is 1 at 0, 0 at
 * u_k, continuous and non-increasing; erf, erfc, exp and sqrt in fp64, csrc/magsac_loss.h is the code for device and host).  A
 * point contributes q = llrint(gain * 2^32), an integer of [0, 2^32]; quality int64 [B][K] is the sum of q over the pair's points;
 * counts int32 [B][K] is the number of points with err <= thr2, gim_ransac_score's (kind 1) or gim_homography_mask's (kind 0).
 * Both are FULLY written by the call: 0 and 0 for a model with valid == 0 or with an entry that is not finite, and for a pair
 * without points.  A VALID ALL-ZERO model under kind 1 has err = 0 / 1e-300 = 0 at every point whose coordinates are finite, as in
 * gim_ransac_score: it counts every such point and gets the largest quality there is, 2^32 per point (under kind 0 it has w == 0:
 * 0 and 0).  Nothing here keeps it out of a RANSAC walk; the valid flags of the step entry points do (a rejected sample or an
 * unused slot is a zero model with valid == 0).  Only integer sums cross lanes and workgroups: the result does not depend on the launch shape, the point split,
 * the batch or the pair's place in it.  B == 0 or K == 0 returns without touching anything.  Refused before a launch: kind outside
 * {0, 1}, max_thr2 not finite or not positive, B > 65535, a NULL pointer, a or b not 16-byte aligned, models or quality not 8-byte
 * aligned, offsets or counts not 4-byte aligned. */
int gim_magsac_score(int kind, const double* models, const uint8_t* valid, const double* a, const double* b, const int32_t* offsets,
                     int B, int K, double thr2, double max_thr2, int64_t* quality, int32_t* counts, gim_stream_t stream);

/* gim_ransac_records keyed on an int64 quality.  quality int64 [B][K][k] and counts int32 [B][K][k], k in {1, 3, 10}: the outputs
 * of gim_magsac_score over the models of a step; nb int32 [B] as in gim_ransac_records; floor_q int64 [B]: the quality to beat.
 * A slot is eligible iff its count is at least min_count; an ineligible slot has key 0.  For s < nb[b]: Q_s = the largest key of
 * the sample's k slots, j_s the lowest slot that holds it; s is a record iff Q_s > max(floor_q[b], Q_0 .. Q_{s-1}).
 * rec int64 [B][1 + 4 K]: rec[b][0] = n_rec, then (s, j_s, c_s, Q_s) per record in ascending s, c_s the count of slot j_s; the
 * words beyond the last record are NOT written.  The same walk as gim_ransac_records, no atomics.  (pose.step_records64 is the
 * numpy restatement.)  B == 0 returns without touching anything; K == 0 writes n_rec = 0.  Refused before a launch: k outside
 * {1, 3, 10}, a NULL pointer, quality, floor_q or rec not 8-byte or counts or nb not 4-byte aligned, B > 65535, B * K * k or
 * B * (1 + 4 K) > INT32_MAX. */
int gim_ransac_records64(const int64_t* quality, const int32_t* counts, const int32_t* nb, const int64_t* floor_q, int min_count,
                         int B, int K, int k, int64_t* rec, gim_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GIM_HIP_H */
