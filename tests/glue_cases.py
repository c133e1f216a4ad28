"""Shapes, seeded inputs and plain float64 restatements of the small memory-bound kernels between the heavy ones: LayerNorm(+residual),
the two layout kernels, upsample2x_add, posenc_add, fine_gather, fine_match, the two max-pools and the two bilinear resizes.  Shared by
tests/test_glue_cases_cpu.py (which holds every restatement to the torch op / oracle function it restates, on every case, on the host
alone) and tests/test_gpu_glue_edges.py.  Nothing here touches a device; inputs and references are built once and frozen (lru_cache:
the tests clone before they modify).

Bars.  Copy, max and gather kernels are bit exact against the reference rounded to the stored kind.  An fp32 output of a computing
kernel (layernorm, upsample2x_add, resize_*, fine_match) is held to bar32(): 4 x the error of the fp32 torch op it restates against the
float64 restatement ON THE SAME CASE (4 for another summation order) + one fp32 ulp of the output scale.  A 16-bit output is compared
element by element, in units in the last place of the stored kind (ulps16), with the float64 reference rounded to that kind: one ulp,
because the kernel rounds an fp32 value that may sit a rounding away from the float64 one.  Where an output element cancels to (nearly)
nothing its 16-bit ulp is finer than fp32 arithmetic itself -- no fp32 evaluation, F.layer_norm included, is within one such ulp of
the float64 value there -- so check16() reports two counts: elements more than one ulp from round16(ref) (`strict`), and elements
outside [round16(ref - bar) - 1 ulp, round16(ref + bar) + 1 ulp] with `bar` the fp32 bar of the case (`loose`: what rounding a
value within the fp32 bar can give, and the same rule as `strict` wherever bar << ulp16)."""
import functools
import math

import torch
import torch.nn.functional as F

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTS = ("fp32", "bf16", "fp16")
NAN = float("nan")


def group(dt):
    """elements of one 16-byte channel group"""
    return 4 if dt == "fp32" else 8


def cstore(c, dt):
    """channels stored for a c-channel activation (gim_amd.packing.cstore)"""
    return (c + group(dt) - 1) // group(dt) * group(dt)


def rnd(t, dt):
    """rounded to the kind, fp32 container"""
    return t.to(TDT[dt]).float()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ bars
def max_err(got, ref64):
    return (got.double() - ref64).abs().max().item() if ref64.numel() else 0.0


def bar32(cpu_err, scale):
    """4 x the fp32 torch op's own error on the case + one fp32 ulp of the output scale"""
    return 4.0 * cpu_err + 2.0 ** -23 * scale


def ordered(t16):
    """a 16-bit float tensor as integers in value order (+-0 together): neighbouring values differ by 1"""
    i = t16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulps16(a16, b16):
    return (ordered(a16) - ordered(b16)).abs()


def check16(got16, ref64, dt, bar=0.0):
    """-> (strict, loose): elements of got16 more than one ulp from round16(ref64); elements outside
    [round16(ref64 - bar) - 1 ulp, round16(ref64 + bar) + 1 ulp].  Non-finite elements count in both."""
    got16 = got16.detach().cpu()
    assert got16.dtype == TDT[dt] and got16.shape == ref64.shape, (got16.dtype, got16.shape, ref64.shape)
    g = ordered(got16)
    bad = ~torch.isfinite(got16.float())
    strict = ((g - ordered(ref64.to(TDT[dt]))).abs() > 1) | bad
    lo, hi = ordered((ref64 - bar).to(TDT[dt])), ordered((ref64 + bar).to(TDT[dt]))
    loose = (g < lo - 1) | (g > hi + 1) | bad
    return int(strict.sum()), int(loose.sum())


# ------------------------------------------------------------------------------------------------------------ layernorm
LN_C = (4, 128, 252, 256, 260, 384, 512)
LN_R = (1, 4, 5, 203)                      # four rows (waves) per block: a lone row, a full block, ragged last blocks
LN_EPS = (1e-5, 1e-6)                      # nn.LayerNorm's default (LoFTR's norm1 / norm2); the ViT norms' value
LN_VARIANTS = ("all", "no_f32", "no_t", "no_res", "inplace")
LN_VARIANT_R = (5, 203)                    # the variants other than "all" run at these row counts
LN_CONST = (3.25, -1.5, 0.75, 1000.0, 0.0)  # constant rows: few significant bits, so every partial sum and the mean are exact
LN_REFUSED_C = (516, 6)


def ref_layernorm(x, gamma, beta, res, eps):
    """float64: (x - mean) / sqrt(biased var + eps) * gamma + beta (+ res), per row"""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    return y if res is None else y + res.double()


def fp32_layernorm(x, gamma, beta, res, eps):
    y = F.layer_norm(x.float(), (x.shape[1],), gamma, beta, eps)
    return y if res is None else y + res


@functools.lru_cache(maxsize=None)
def ln_inputs(C, R, kind, xdt):
    """(x, gamma, beta, res) fp32 containers; x rounded to xdt.  kind: randn (3 randn + 0.5), offset (1000 + randn), const"""
    g = gen(7000 + 13 * C + R)
    x = torch.randn(R, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    res = torch.randn(R, C, generator=g)
    if kind == "randn":
        x = x * 3 + 0.5
    elif kind == "offset":
        x = 1000 + x
    else:
        assert kind == "const" and R == len(LN_CONST)
        x = torch.tensor(LN_CONST)[:, None].expand(R, C).contiguous()
    return rnd(x, xdt), gamma, beta, res


@functools.lru_cache(maxsize=None)
def ln_ref(C, R, kind, xdt, with_res, eps):
    """(float64 reference, error of fp32 F.layer_norm (+ res) on the same operands against it)"""
    x, gamma, beta, res = ln_inputs(C, R, kind, xdt)
    res = res if with_res else None
    ref = ref_layernorm(x, gamma, beta, res, eps)
    return ref, max_err(fp32_layernorm(x, gamma, beta, res, eps), ref)


def ln_plan(dt, C):
    """(R, xdt, variant, eps) of one (output kind, C): every R in the model's layout, the variants at two row counts, the second eps"""
    for xdt in (("fp32",) if dt == "fp32" else ("fp32", dt)):
        for R in LN_R:
            yield R, xdt, "all", LN_EPS[0]
        for R in LN_VARIANT_R:
            for v in LN_VARIANTS[1:]:
                yield R, xdt, v, LN_EPS[0]
            yield R, xdt, "all", LN_EPS[1]


def ln_instance(dt, xdt, variant):
    """the layernorm_kernel<BF16, XBF16> instance a launch takes (ops.layernorm_residual: the output tag is out_t's, fp32 without out_t)"""
    return (dt != "fp32" and variant != "no_t", xdt != "fp32")


# ------------------------------------------------------------------------------------------------------------ layout kernels
def round_up(x, m):
    return (x + m - 1) // m * m


TO_NCHW_C = (1, 3, 63, 64, 65, 196)
TO_NCHW_HW = ((1, 1), (7, 9), (8, 8), (5, 13), (10, 13))        # HW = 1, 63, 64, 65, 130 around the 64-pixel tile
TO_NCHW_B = 2
TO_NHWC_C, TO_NHWC_CPAD, TO_NHWC_BOFF = (1, 3, 5), (4, 8), (0, 2)
TO_NHWC_HW = ((1, 1), (15, 17), (1, 257))                       # HW = 1, 255 (below one 256-thread block), 257
TO_NHWC_B, TO_NHWC_IMAGES = 2, 4
ROUNDTRIP = (2, 196, 5, 13)


def to_nchw_lds(C):
    return (round_up(C, 8), round_up(C, 8) + 8)


def to_nhwc_cases():
    for C in TO_NHWC_C:
        for cpad in TO_NHWC_CPAD:
            if cpad < C:
                continue
            for ld in (cpad, cpad + 8):
                for b_off in TO_NHWC_BOFF:
                    for hw in TO_NHWC_HW:
                        yield C, cpad, ld, b_off, hw


@functools.lru_cache(maxsize=None)
def nhwc_rows(B, H, W, ld, dt, seed):
    """[B, H, W, ld] values of the kind (fp32 container): every column random, so a read past C shows"""
    return rnd(torch.randn(B, H, W, ld, generator=gen(seed)), dt)


@functools.lru_cache(maxsize=None)
def nchw_image(B, C, H, W, seed):
    return torch.randn(B, C, H, W, generator=gen(seed))


def ref_nhwc_to_nchw(rows, C):
    """[B, H, W, ld] -> float64 [B, C, H, W]: out[b, c, y, x] = rows[b, y, x, c], element by element"""
    B, H, W, _ = rows.shape
    out = torch.empty(B, C, H, W, dtype=torch.float64)
    for c in range(C):
        out[:, c] = rows[..., c].double()
    return out


def ref_nchw_to_nhwc(src, cpad):
    """[B, C, H, W] -> float64 [B, H, W, cpad], channels >= C zero"""
    B, C, H, W = src.shape
    out = torch.zeros(B, H, W, cpad, dtype=torch.float64)
    for c in range(C):
        out[..., c] = src[:, c].double()
    return out


# ------------------------------------------------------------------------------------------------------------ bilinear
def lin_matrix(n_in, n_out, align_corners):
    """float64 [n_out, n_in] interpolation matrix of one axis, ATen's area_pixel_compute_source_index"""
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    for d in range(n_out):
        if align_corners:
            s = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        else:
            s = max(0.0, (n_in / n_out) * (d + 0.5) - 0.5)
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        A[d, i0] += 1.0 - (s - i0)
        A[d, i1] += s - i0
    return A


def ref_resize(x, size, align_corners):
    """float64 bilinear resize of [B, C, h, w] to `size`"""
    Ay, Ax = lin_matrix(x.shape[2], size[0], align_corners), lin_matrix(x.shape[3], size[1], align_corners)
    return torch.einsum("Yy,bcyx,Xx->bcYX", Ay, x.double(), Ax)


UPS_HW = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 9))
UPS_B = 2


def ups_channels(dt):
    """(channels, stored channels): one 16-byte group, and 196 stored as in the model"""
    return ((group(dt), group(dt)), (196, cstore(196, dt)))


@functools.lru_cache(maxsize=None)
def ups_case(h, w, C, dt):
    """(lo [B,C,h,w], hi [B,C,2h,2w] rounded to the kind, float64 reference, error of the fp32 torch op)"""
    g = gen(8000 + 100 * h + 10 * w + C)
    lo, hi = rnd(torch.randn(UPS_B, C, h, w, generator=g), dt), rnd(torch.randn(UPS_B, C, 2 * h, 2 * w, generator=g), dt)
    ref = hi.double() + ref_resize(lo, (2 * h, 2 * w), True)
    op = hi + F.interpolate(lo, scale_factor=2, mode="bilinear", align_corners=True)
    return lo, hi, ref, max_err(op, ref)


RESIZE_PAIRS = (("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16"), ("fp32", "fp16"), ("fp16", "fp32"), ("fp16", "fp16"))
RESIZE_SHAPES = (((12, 20), (12, 20)), ((12, 20), (24, 40)), ((12, 20), (7, 9)), ((12, 20), (1, 1)), ((1, 1), (4, 6)), ((1, 5), (4, 6)))
RESIZE_B, RESIZE_C, RESIZE_LDS = 2, 6, (8, 16)
RESIZE_IMAGE_C, RESIZE_IMAGE_CPAD, RESIZE_IMAGE_BOFF, RESIZE_IMAGE_IMAGES = (1, 3), (4, 8), (0, 1), 3


@functools.lru_cache(maxsize=None)
def resize_case(src, size, C, dt):
    """(x [B,C,h,w] rounded to dt, float64 reference, error of fp32 F.interpolate(align_corners=False))"""
    x = rnd(torch.randn(RESIZE_B, C, *src, generator=gen(8500 + 31 * src[0] + src[1] + C)), dt)
    ref = ref_resize(x, size, False)
    return x, ref, max_err(F.interpolate(x, size=size, mode="bilinear", align_corners=False), ref)


# ------------------------------------------------------------------------------------------------------------ posenc
POSENC_HW = {1: (1, 1), 7: (1, 7), 48: (6, 8)}
POSENC_NB, POSENC_C = (1, 3), (4, 256)
POSENC_OUTS = ("f32", "t", "both")


@functools.lru_cache(maxsize=None)
def ref_position_encoding(d_model, h, w):
    """float64 [d_model, h, w] of networks/loftr/utils/position_encoding.py with temp_bug_fix=False: 1-based positions, channels
    4k..4k+3 = sin(x f_k), cos(x f_k), sin(y f_k), cos(y f_k) with f_k = exp(2k * floor(-ln(1e4) / d_model / 2))"""
    q = math.floor(-math.log(10000.0) / d_model / 2)
    pe = torch.zeros(d_model, h, w, dtype=torch.float64)
    ys = torch.arange(1, h + 1, dtype=torch.float64)[:, None].expand(h, w)
    xs = torch.arange(1, w + 1, dtype=torch.float64)[None, :].expand(h, w)
    for k in range(d_model // 4):
        f = math.exp(2 * k * q)
        pe[4 * k], pe[4 * k + 1], pe[4 * k + 2], pe[4 * k + 3] = torch.sin(xs * f), torch.cos(xs * f), torch.sin(ys * f), torch.cos(ys * f)
    return pe


@functools.lru_cache(maxsize=None)
def posenc_case(hw, nb, C, dt):
    """(x [nb*hw, C] of the kind, pe [hw, C] fp32 table, float64 reference x + pe[m % hw])"""
    h, w = POSENC_HW[hw]
    x = rnd(torch.randn(nb * hw, C, generator=gen(8800 + hw + nb + C)), dt)
    pe = ref_position_encoding(C, h, w).permute(1, 2, 0).reshape(hw, C).float().contiguous()     # h = 1: the reshape is a strided view
    ref = x.double() + pe.double()[torch.arange(nb * hw) % hw]
    return x, pe, ref


# ------------------------------------------------------------------------------------------------------------ fine_gather
FG_COARSE = ((6, 8), (5, 7))               # map 0, map 1: unequal in both directions
FG_W, FG_STRIDE, FG_C, FG_M, FG_BS = (1, 3, 5, 7), (2, 4), (4, 128), (1, 37), 2
FG_OUTS = ("f32", "t", "both")


def fg_cases():
    n = 0
    for W in FG_W:
        for stride in FG_STRIDE:
            for C in FG_C:
                for ldf in (C, C + 8):
                    for M in FG_M:
                        if (W, stride, C, ldf, M) == (7, 2, 128, 136, 37):
                            for outs in FG_OUTS:
                                yield W, stride, C, ldf, M, outs
                        else:
                            yield W, stride, C, ldf, M, FG_OUTS[n % 3]
                            n += 1


def corners(hc, wc):
    return [0, wc - 1, wc * (hc - 1), hc * wc - 1]


@functools.lru_cache(maxsize=None)
def fg_ids(M):
    """(b_ids, i_ids, j_ids): two images; the first eight matches put the corners of map 0 into i_ids and those of map 1 into j_ids"""
    (h0, w0), (h1, w1) = FG_COARSE
    g = gen(9000 + M)
    if M == 1:
        return torch.tensor([1]), torch.tensor([0]), torch.tensor([h1 * w1 - 1])
    b = torch.randint(0, FG_BS, (M,), generator=g).sort()[0]
    b[:4], b[-4:] = 0, 1
    i, j = torch.randint(0, h0 * w0, (M,), generator=g), torch.randint(0, h1 * w1, (M,), generator=g)
    i[:4], j[4:8] = torch.tensor(corners(h0, w0)), torch.tensor(corners(h1, w1))
    i[8], j[8] = w0 + 1, w1 + 1                              # interior-adjacent cells: W = 7, stride 2 still crosses the border
    i[9], j[9] = w0 * (h0 - 2) + w0 - 2, w1 * (h1 - 2) + w1 - 2
    return b, i, j


@functools.lru_cache(maxsize=None)
def fg_maps(stride, C, dt):
    g = gen(9100 + stride + C)
    return tuple(rnd(torch.randn(FG_BS, C, stride * hc, stride * wc, generator=g), dt) for (hc, wc) in FG_COARSE)


def ref_fine_gather(f0, f1, b_ids, i_ids, j_ids, w0c, w1c, stride, W):
    """(u0, u1) [M, W*W, C] in the maps' dtype: the W x W window centred on fine pixel stride * (cell row, cell column), zero outside"""
    def side(f, ids, wc):
        _, C, hf, wf = f.shape
        d = torch.arange(W) - W // 2
        y = (ids // wc * stride)[:, None, None] + d[None, :, None]
        x = (ids % wc * stride)[:, None, None] + d[None, None, :]
        ok = (y >= 0) & (y < hf) & (x >= 0) & (x < wf)
        v = f[b_ids[:, None, None], :, y.clamp(0, hf - 1), x.clamp(0, wf - 1)]        # [M, W, W, C]
        return (v * ok[..., None]).reshape(ids.numel(), W * W, C)
    return side(f0, i_ids, w0c), side(f1, j_ids, w1c)


# ------------------------------------------------------------------------------------------------------------ fine_match
FM_W, FM_C, FM_M = (3, 5, 7), (4, 128), (1, 4, 5)
FM_REGIMES = ("random", "flat", "sat_centre", "sat_corner", "sat_last", "offset")
FM_BS, FM_SCALE = 2, 2.0
FM_REFUSED_WW = (50, 81)


def fm_sat_cell(regime, W):
    return {"sat_centre": W * W // 2, "sat_corner": W - 1, "sat_last": W * W - 1}[regime]


@functools.lru_cache(maxsize=None)
def fm_inputs(W, C, M, regime):
    """(f0, f1 [M, WW, C] fp32, mkpts1_c [M, 2], b_ids [M], scale1 [bs, 2])"""
    WW = W * W
    g = gen(9500 + 100 * W + C + M)
    f0, f1 = torch.randn(M, WW, C, generator=g), torch.randn(M, WW, C, generator=g)
    mk = torch.rand(M, 2, generator=g) * 100
    b = torch.arange(M) * FM_BS // M
    s1 = torch.tensor([[0.75, 1.5], [1.25, 0.625]])           # per image, different in x and y
    if regime == "flat":
        f0 = torch.zeros_like(f0)
    elif regime.startswith("sat"):
        # channel 0 alone: s_r = 16 * f1[r, 0]; 8 at the planted cell, [0, 1) elsewhere: 112 above every other after the temperature
        f0 = torch.zeros_like(f0)
        f0[:, WW // 2, 0] = 16.0 * math.sqrt(C)
        f1[:, :, 0] = torch.rand(M, WW, generator=g)
        f1[:, fm_sat_cell(regime, W), 0] = 8.0
    elif regime == "offset":
        q = f0[:, WW // 2, :]
        f1 = f1 + (80.0 * math.sqrt(C) / (q * q).sum(1))[:, None, None] * q[:, None, :]      # every similarity + 80
    return f0, f1, mk, b, s1


def ref_fine_match(f0, f1, mk1c, b_ids, s1, scale, has_scale0):
    """float64 (expec_f [M, 3], mkpts1_f [M, 2]) of fine_matching.py:43-74"""
    M, WW, C = f0.shape
    W = math.isqrt(WW)
    sim = (f0[:, WW // 2, None, :].double() * f1.double()).sum(2) / math.sqrt(C)
    e = torch.exp(sim - sim.max(1, keepdim=True)[0])
    heat = e / e.sum(1, keepdim=True)
    lin = torch.tensor([-1.0 + 2.0 * k / (W - 1) for k in range(W)], dtype=torch.float64)
    gx, gy = lin.repeat(W), lin.repeat_interleave(W)
    cx, cy = (heat * gx).sum(1), (heat * gy).sum(1)
    vx, vy = (heat * gx * gx).sum(1) - cx * cx, (heat * gy * gy).sum(1) - cy * cy
    std = vx.clamp(min=1e-10).sqrt() + vy.clamp(min=1e-10).sqrt()
    sc = scale * s1.double()[b_ids] if has_scale0 else torch.full((M, 2), scale, dtype=torch.float64)
    coords = torch.stack([cx, cy], 1)
    return torch.cat([coords, std[:, None]], 1), mk1c.double() + coords * (W // 2) * sc


def flat_std(W):
    """std of the uniform heatmap over linspace(-1, 1, W)^2: 2 sqrt(mean g^2) = 2 sqrt((W + 1) / (3 (W - 1)))"""
    return 2.0 * math.sqrt((W + 1) / (3.0 * (W - 1)))


def grid_coord_fp32(W, k):
    """the two fp32 evaluations of -1 + (2 / (W - 1)) * k: product rounded first, or fused"""
    step = torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(W - 1), dtype=torch.float32)
    sep = (step * torch.tensor(float(k), dtype=torch.float32) - 1.0).item()
    fused = (step.double() * k - 1.0).float().item()
    return {sep, fused}


SAT_STD = (2.0 * torch.sqrt(torch.tensor(1e-10, dtype=torch.float32))).item()       # 2 * sqrt(1e-10f) as fp32 computes it


@functools.lru_cache(maxsize=None)
def fm_ref(W, C, M, regime, has_scale0, hw0_f=(8, 8)):
    """(float64 expec_f, mkpts1_f; the errors of loftr_oracle.fine_matching in fp32 against them)"""
    import loftr_oracle as O
    f0, f1, mk, b, s1 = fm_inputs(W, C, M, regime)
    e64, m64 = ref_fine_match(f0, f1, mk, b, s1, FM_SCALE, has_scale0)
    o = O.fine_matching(f0, f1, mk.clone(), mk, b, M, (int(FM_SCALE * hw0_f[0]), int(FM_SCALE * hw0_f[1])), hw0_f, s1, has_scale0)
    return e64, m64, max_err(o["expec_f"], e64), max_err(o["mkpts1_f"], m64)


# ------------------------------------------------------------------------------------------------------------ max-pools
POOL2_HW = ((2, 2), (3, 5), (8, 6), (21, 30))
POOL3_HW = ((1, 1), (1, 2), (2, 1), (3, 3), (4, 5), (21, 30))
POOL_B = 2


def pool_channels(dt):
    return (group(dt), 64)


@functools.lru_cache(maxsize=None)
def pool_input(H, W, C, dt, negative):
    x = torch.randn(POOL_B, C, H, W, generator=gen(9800 + 50 * H + W + C))
    return rnd(-x.abs() - 0.5 if negative else x, dt)


def ref_maxpool(x, k, stride, pad):
    """[B, C, H, W] -> max over k x k windows at `stride`, -inf beyond the border; the output size floors"""
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    p = torch.full((B, C, H + 2 * pad + k, W + 2 * pad + k), -math.inf, dtype=torch.float64)
    p[:, :, pad:pad + H, pad:pad + W] = x.double()
    out = torch.full((B, C, Ho, Wo), -math.inf, dtype=torch.float64)
    for dy in range(k):
        for dx in range(k):
            out = torch.maximum(out, p[:, :, dy:dy + stride * Ho:stride, dx:dx + stride * Wo:stride])
    return out
