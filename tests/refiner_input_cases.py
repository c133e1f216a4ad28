"""Case tables, host-side builders, references and bounds of the ConvRefiner input-assembly tests: shared by
tests/test_refiner_input_cases_cpu.py (which judges them on the host alone) and tests/test_gpu_refiner_inputs.py.  Nothing here touches
a device or gim_amd; inputs and references are built once per case and frozen (lru_cache: the tests clone before they modify).

The four kernels (csrc/dkm.hip) and their references, all on the CPU in fp32 on inputs ALREADY rounded to the kernel's operand dtype:
    grid_sample      F.grid_sample(bilinear, zeros, align_corners=False)
    local_corr       dkm_oracle.local_correlation
    dkm_disp_emb     F.conv2d(flow - dkm_oracle.grid_coords, W[:, :, None, None], bias)
    resize_bilinear  F.interpolate(mode="bilinear", align_corners=False)

Bounds (derived, not measured).  fp32 output: BAR32 of max|ref|, the bars tests/test_gpu_dkm.py already holds these kernels to.  16-bit
output: the kernels accumulate in fp32 and round ONCE to nearest even, so elementwise
    |got - ref| <= U |ref| + BAR32 max|ref| + A        U = half an ulp of the format (2^-8 bf16, 2^-11 fp16), A = fp16's subnormal half step
worst_ratio() returns the largest |got - ref| / bound; a truncating store reaches ~2.

Exact zeros.  A tap that lies wholly outside the map contributes exactly 0 in the reference and in the kernels.  A tap whose coordinate
sits ON the zero boundary (pixel coordinate -1 or `size`, which the pixel-centre grid produces for every border query) is decided by
the last bit of the coordinate arithmetic: the reference rounds flow + window offset in normalised units, the kernel subtracts r
pixels, so one of them may see a weight of 1e-7 where the other sees 0.  robust_outside() therefore marks what is outside by more
than ZERO_MARGIN pixels in float64 geometry; the CPU test shows that the reference is exactly 0 on all of it, the GPU test demands
exactly 0 there, and boundary taps are held to the bound like every other element."""
import collections
import functools
import math

import torch
import torch.nn.functional as F

import dkm_oracle as O

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTS = ("fp32", "bf16", "fp16")
H16 = ("bf16", "fp16")
BAR32 = {"grid_sample": 2e-6, "disp_emb": 2e-6, "resize": 2e-6, "local_corr": 2e-5}
U = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
A = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}
SENTINEL = 7.0            # columns of a row buffer outside the written slice: bit-identical after the call
ZERO_MARGIN = 1e-3        # pixels
# the engines' refiner tables: scale -> (feature channels, displacement-embedding channels, local-correlation radius)
REFINER_DKM = O.REFINER
REFINER_ROMA = {"16": (512, 128, 7), "8": (512, 64, 3), "4": (256, 32, 2), "2": (64, 16, None), "1": (9, 6, None)}
CORR_SCALES = ("16", "8", "4")


def cstore(c, dt):
    """channels stored for a c-channel activation: padded to a 16-byte group (gim_amd.packing.cstore)"""
    g = 4 if dt == "fp32" else 8
    return (c + g - 1) // g * g


def refine_layout(table, scale, dt):
    """what gim_amd.dense.refine computes for the scale's input row: column of the grid_sample / disp_emb / local_corr slice, row stride"""
    c, e, r = table[scale]
    k = (2 * r + 1) ** 2 if r else 0
    return {"gs": c, "emb": 2 * c, "corr": 2 * c + e, "cs": cstore(2 * c + e + k, dt), "width": 2 * c + e + k}


def rounded(x, dt):
    return x.to(TDT[dt]).float()


def grid(b, h, w):
    """the pixel-centre grid [b, h, w, 2] (x, y)"""
    return O.grid_coords(b, h, w).permute(0, 2, 3, 1).contiguous()


def norm_of_px(p, size):
    """normalised coordinate whose align_corners=False pixel coordinate is p (float64 arithmetic)"""
    return (2.0 * p + 1.0) / size - 1.0


# ------------------------------------------------------------------------------------------------------------ bounds
def bound(ref, odt, kind, scale=None):
    """elementwise bound on |got - ref| (float64)"""
    ref = ref.double()
    scale = ref.abs().max().item() if scale is None else scale
    return U[odt] * ref.abs() + BAR32[kind] * scale + A[odt]


def worst_ratio(got, ref, odt, kind, scale=None):
    """max over ALL elements of |got - ref| / bound (a zero bound admits only equality); non-finite output -> inf"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return math.inf
    err = (got.double() - ref.double()).abs()
    return (err / bound(ref, odt, kind, scale).clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------------------ row buffers
def row_buffer(rows, width, dt):
    return torch.full((rows, width), SENTINEL, dtype=TDT[dt])


def untouched(buf_after, sl):
    """bit for bit: every column of `buf_after` outside `sl` still holds SENTINEL"""
    it = {2: torch.int16, 4: torch.int32}[buf_after.element_size()]
    want = torch.full((1,), SENTINEL, dtype=buf_after.dtype).view(it)
    keep = torch.ones(buf_after.shape[1], dtype=torch.bool)
    keep[sl] = False
    return bool((buf_after.cpu().contiguous().view(it)[:, keep] == want).all())


def nan_padded(x_nhwc, dt, pad=8):
    """[B,h,w,C] values -> (buffer [B,h,w,C+pad] of dtype dt with NaN in the padding, C): the kernel gets buffer[..., :C]"""
    B, h, w, C = x_nhwc.shape
    buf = torch.full((B, h, w, C + pad), float("nan"), dtype=TDT[dt])
    buf[..., :C] = x_nhwc.to(TDT[dt])
    return buf, C


# ------------------------------------------------------------------------------------------------------------ tap geometry
def _tap_px(flow_bhw2, r, h, w, dtype):
    """pixel coordinates (ix, iy) [B,h,w,K] of every window tap.  fp32: the reference's own arithmetic (local_correlation adds the
    window in normalised units, grid_sample unnormalises); fp64: the geometry (target pixel + integer offset)"""
    n = 2 * r + 1
    if dtype == torch.float32:
        wy = torch.linspace(-2 * r / h, 2 * r / h, n) if r else torch.zeros(1)
        wx = torch.linspace(-2 * r / w, 2 * r / w, n) if r else torch.zeros(1)
        gy, gx = torch.meshgrid(wy, wx, indexing="ij")
        cx = flow_bhw2[..., 0, None] + gx.reshape(-1)
        cy = flow_bhw2[..., 1, None] + gy.reshape(-1)
        return ((cx + 1) * w - 1) / 2, ((cy + 1) * h - 1) / 2
    f = flow_bhw2.double()
    oy, ox = torch.meshgrid(torch.arange(-r, r + 1, dtype=torch.float64), torch.arange(-r, r + 1, dtype=torch.float64), indexing="ij")
    return ((f[..., 0, None] + 1) * w - 1) / 2 + ox.reshape(-1), ((f[..., 1, None] + 1) * h - 1) / 2 + oy.reshape(-1)


def robust_outside(flow_bhw2, r, h, w):
    """bool [B*h*w, K]: taps wholly outside the map by more than ZERO_MARGIN pixels (float64 geometry)"""
    ix, iy = _tap_px(flow_bhw2, r, h, w, torch.float64)
    m = ZERO_MARGIN
    out = (ix <= -1 - m) | (ix >= w + m) | (iy <= -1 - m) | (iy >= h + m)
    return out.reshape(-1, (2 * r + 1) ** 2)


def tap_classes(flow_bhw2, r, h, w):
    """per-query classes from the reference's own fp32 arithmetic -> counts of queries whose window has all taps inside (every corner
    with weight inside the map), some taps beyond the left / right / top / bottom side (and not all outside), all taps outside"""
    ix, iy = _tap_px(flow_bhw2.float(), r, h, w, torch.float32)
    inside = (ix >= 0) & (ix <= w - 1) & (iy >= 0) & (iy <= h - 1)
    outside = (ix <= -1) | (ix >= w) | (iy <= -1) | (iy >= h)
    all_out = outside.all(-1)
    part = ~all_out
    return {"inside": int(inside.all(-1).sum()), "outside": int(all_out.sum()),
            "left": int(((ix < 0).any(-1) & part).sum()), "right": int(((ix > w - 1).any(-1) & part).sum()),
            "top": int(((iy < 0).any(-1) & part).sum()), "bottom": int(((iy > h - 1).any(-1) & part).sum())}


# ------------------------------------------------------------------------------------------------------------ local_corr
LC = collections.namedtuple("LC", "id C r dt odt B h w flow col0 stride pad")


def lc_instance(C, r, dt, odt, ld0, ld1):
    """(16-bit in, 16-bit out, V8, PT): the instantiation gim_local_corr launches (csrc/dkm.hip)"""
    ib, ob = dt != "fp32", odt != "fp32"
    v8 = ib and C % 512 == 0 and ld0 % 8 == 0 and ld1 % 8 == 0
    P = 2 * r + 2
    pt = 6 if P <= 6 else 8 if P <= 8 else 16
    if ib != ob:
        pt = 16
    return ib, ob, v8, pt


N_LC_TABLE = 25           # entries of lc_flow_table = images of an edge case


def _lc(tag, C, r, dt, odt=None, B=1, h=5, w=7, flow="random", col0=None, stride=None, pad=0):
    odt = odt or dt
    B = N_LC_TABLE if flow == "table" else B
    K = (2 * r + 1) ** 2
    col0 = 2 * C + 32 if col0 is None else col0
    stride = cstore(col0 + K, odt) if stride is None else stride
    name = f"{tag}-C{C}-r{r}-{dt}" + (f"-to-{odt}" if odt != dt else "") + f"-{B}x{h}x{w}" + (f"-pad{pad}" if pad else "")
    return LC(name, C, r, dt, odt, B, h, w, flow, col0, stride, pad)


def _lc_prod(scale, dt, odt=None):
    c, e, r = REFINER_DKM[scale]
    lay = refine_layout(REFINER_DKM, scale, odt or dt)
    return _lc(f"prod{scale}", c, r, dt, odt, col0=lay["corr"], stride=lay["cs"])


# 1. the instantiations the models run (16 -> 16 into the slice of the 16-bit row buffer), their fp32 twins, the mixed branch,
#    the channel-loop edges (C = 320 fp32: second pass ragged; C = 1024: V8 with two passes), C = 8 (most lanes idle), padded views
LC_PRODUCTION = tuple(_lc_prod(s, dt) for s in CORR_SCALES for dt in ("bf16", "fp16", "fp32")) + tuple(_lc_prod("4", dt, "fp32") for dt in H16)
LC_CHANNELS = (tuple(_lc("chan", 320, r, "fp32") for r in (2, 7)) + tuple(_lc("chan", 1024, r, dt) for r in (3, 7) for dt in H16) +
               tuple(_lc("chan", 8, 1, dt) for dt in DTS))
LC_PADDED = (_lc("view", 512, 3, "bf16", pad=8), _lc("view", 512, 7, "fp16", pad=8), _lc("view", 256, 2, "fp16", pad=8),
             _lc("view", 256, 2, "fp32", pad=8))
# 2. flow edges: one table entry per image of the batch, on a 6 x 5 map; maps smaller than the window
LC_EDGES = tuple(_lc("edge", 64, r, dt, h=6, w=5, flow="table") for r in (1, 2, 3, 7) for dt in DTS)
LC_SMALL = tuple(_lc("small", 64, r, dt, B=2, h=h, w=w) for (r, h, w) in ((7, 3, 2), (1, 1, 1)) for dt in DTS)
LC_ALL = LC_PRODUCTION + LC_CHANNELS + LC_PADDED + LC_EDGES + LC_SMALL


def lc_flow_table(r, h, w):
    """-> (names, flow [len(names), h, w, 2]): entry b is the flow of image b.  Targets are given as the pixel coordinate of the window
    centre (cx, cy: a generic interior point) or in normalised units."""
    cx, cy = (w - 1) / 2 + 0.2, (h - 1) / 2 - 0.3
    g = grid(1, h, w)[0]
    entries = [("grid", g), ("grid+half", g + torch.tensor([1.0 / w, 1.0 / h])), ("grid+quarter", g + torch.tensor([0.5 / w, 1.5 / h]))]

    def const(name, gx, gy):
        entries.append((name, torch.tensor([gx, gy], dtype=torch.float64).float().expand(h, w, 2)))

    def px(name, tx, ty):
        const(name, norm_of_px(tx, w), norm_of_px(ty, h))

    lo, hx, hy = -0.7, w - 1 + 0.7, h - 1 + 0.7
    for name, tx, ty in (("left", lo, cy), ("right", hx, cy), ("top", cx, lo), ("bottom", cx, hy),
                         ("top-left", lo, lo), ("top-right", hx, lo), ("bottom-left", lo, hy), ("bottom-right", hx, hy)):
        px(name, tx, ty)
    # wholly outside by one pixel: the nearest tap lies one pixel beyond the zero boundary (pixel coordinate -1 / size)
    for name, tx, ty in (("out-left", -2.0 - r, cy), ("out-right", w + 1.0 + r, cy), ("out-top", cx, -2.0 - r), ("out-bottom", cx, h + 1.0 + r)):
        px(name, tx, ty)
    gx0, gy0 = norm_of_px(cx, w), norm_of_px(cy, h)
    for v in (3.0, 1e9):
        for s in (1.0, -1.0):
            const(f"x{s * v:+g}", s * v, gy0)
            const(f"y{s * v:+g}", gx0, s * v)
    const("xy+1e9", 1e9, 1e9)
    const("x-1e9,y+1e9", -1e9, 1e9)
    assert len(entries) == N_LC_TABLE
    return [n for n, _ in entries], torch.stack([f for _, f in entries]).contiguous()


@functools.lru_cache(maxsize=None)
def lc_inputs(c):
    """(f0, f1 [B,C,h,w] fp32 containers of dt-rounded values, flow [B,h,w,2] fp32)"""
    g = torch.Generator().manual_seed(5100 + c.C + 7 * c.r)
    if c.flow == "table":
        flow = lc_flow_table(c.r, c.h, c.w)[1]
    else:
        flow = grid(c.B, c.h, c.w) + 0.3 * torch.randn(c.B, c.h, c.w, 2, generator=g)      # windows partly outside the map
    B = flow.shape[0]
    f0 = rounded(torch.randn(B, c.C, c.h, c.w, generator=g), c.dt)
    f1 = rounded(torch.randn(B, c.C, c.h, c.w, generator=g), c.dt)
    return f0, f1, flow


@functools.lru_cache(maxsize=None)
def lc_ref(c):
    """rows [B*h*w, (2r+1)^2]"""
    f0, f1, flow = lc_inputs(c)
    K = (2 * c.r + 1) ** 2
    return O.local_correlation(f0, f1, c.r, flow.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(-1, K).contiguous()


def lc_zero_mask(c):
    return robust_outside(lc_inputs(c)[2], c.r, c.h, c.w)


# ------------------------------------------------------------------------------------------------------------ grid_sample
GS = collections.namedtuple("GS", "id C dt B h w ho wo kind layout")


def _gs(C, dt, h, w, ho, wo, kind, layout="slice"):
    return GS(f"C{C}-{dt}-map{h}x{w}-grid{ho}x{wo}-{kind}-{layout}", C, dt, 3, h, w, ho, wo, kind, layout)


def gs_grid_table(h, w):
    """-> (names, [n, 2] fp32 grid values of a map h x w)"""
    d = 4 * ZERO_MARGIN                     # pixels inside / outside the zero boundary (pixel coordinate -1 and `size`, +-(1 + 1/size))
    ix, iy = 0.13, -0.37                    # a generic interior target on the other axis
    nx, ny = (lambda p: norm_of_px(p, w)), (lambda p: norm_of_px(p, h))
    ent = [("x=+1", 1.0, iy), ("x=-1", -1.0, iy), ("y=+1", ix, 1.0), ("y=-1", ix, -1.0),
           ("right-in", nx(w - d), iy), ("right-out", nx(w + d), iy), ("left-in", nx(-1 + d), iy), ("left-out", nx(-1 - d), iy),
           ("bottom-in", ix, ny(h - d)), ("bottom-out", ix, ny(h + d)), ("top-in", ix, ny(-1 + d)), ("top-out", ix, ny(-1 - d))]
    for v in (3.0, 1e6, 1e9, 1e12):
        ent += [(f"x+{v:g}", v, iy), (f"x-{v:g}", -v, iy), (f"y+{v:g}", ix, v), (f"y-{v:g}", ix, -v)]
    ent += [("x+1e9,y-1e9", 1e9, -1e9), ("x-1e12,y+1e12", -1e12, 1e12),
            ("centre", norm_of_px(w // 2, w), norm_of_px(h // 2, h)), ("interior", ix, iy), ("interior2", -0.61, 0.45)]
    return [e[0] for e in ent], torch.tensor([[e[1], e[2]] for e in ent], dtype=torch.float64).float()


def gs_grid(c):
    """[B, ho, wo, 2]: "centres" -- the pixel-centre grid (needs grid size == map size); "table" -- the edge table, rotated by 11
    entries per image so that every image meets every entry at another position"""
    if c.kind == "centres":
        assert (c.ho, c.wo) == (c.h, c.w)
        return grid(c.B, c.h, c.w)
    tab = gs_grid_table(c.h, c.w)[1]
    n = c.ho * c.wo
    assert n >= len(tab)
    idx = (torch.arange(n)[None, :] + 11 * torch.arange(c.B)[:, None]) % len(tab)
    return tab[idx].reshape(c.B, c.ho, c.wo, 2).contiguous()


_GS_CD = tuple((C, dt) for C in (4, 8, 64, 512) for dt in DTS if not (C == 4 and dt != "fp32"))
GS_MAIN = tuple(_gs(C, dt, 5, 7, ho, wo, kind) for (C, dt) in _GS_CD for (ho, wo, kind) in ((5, 7, "centres"), (5, 7, "table"), (4, 9, "table")))
# the scale-1 shape: the image features are one channel group per pixel and the output is a whole row (gim_amd.dense.refine, c % g != 0)
GS_WHOLE = tuple(_gs(8, dt, 5, 7, ho, wo, kind, "whole") for dt in DTS for (ho, wo, kind) in ((5, 7, "centres"), (4, 9, "table")))
GS_THIN = tuple(_gs(C, dt, h, w, ho, wo, kind) for (h, w) in ((1, 7), (7, 1)) for C in (8, 64) for dt in DTS
                for (ho, wo, kind) in ((h, w, "centres"), (5, 7, "table")))
GS_ALL = GS_MAIN + GS_WHOLE + GS_THIN


@functools.lru_cache(maxsize=None)
def gs_inputs(c):
    """(feat [B,C,h,w] fp32 container of dt-rounded values, different per image; grid [B,ho,wo,2])"""
    g = torch.Generator().manual_seed(5300 + c.C)
    return rounded(torch.randn(c.B, c.C, c.h, c.w, generator=g), c.dt), gs_grid(c)


@functools.lru_cache(maxsize=None)
def gs_ref(c):
    """rows [B*ho*wo, C]"""
    feat, gr = gs_inputs(c)
    return F.grid_sample(feat, gr, mode="bilinear", padding_mode="zeros", align_corners=False).permute(0, 2, 3, 1).reshape(-1, c.C).contiguous()


def gs_zero_mask(c):
    """bool [B*ho*wo, 1]"""
    return robust_outside(gs_inputs(c)[1], 0, c.h, c.w)


def gs_out_layout(c):
    """(column of the slice, row stride): the slice at column C of a 3 C wide row as refine writes it, or a whole row"""
    return (c.C, 3 * c.C) if c.layout == "slice" else (0, c.C)


# ------------------------------------------------------------------------------------------------------------ dkm_disp_emb
DE = collections.namedtuple("DE", "id E odt B h w col0 stride emb_scale")
# E -> (slice column, row width) of the scale that has this embedding: 2 c and 2 c + e + (2r+1)^2; E = 6 (scale 1) is written to a
# buffer of its own in the product, here to column 8 of a 24-wide row
_DE_SLICE = {128: (1024, 1024 + 128 + 225), 16: (128, 144), 6: (8, 24)}
DE_MAPS = ((1, 5), (5, 1), (7, 9), (8, 6))
ROMA_EMB_SCALE = 40.0 / 32.0 * 1.5       # roma.py:545-547 with the upsampling pass's scale factor


def _de(E, odt, h, w, emb_scale=None):
    col0, width = _DE_SLICE[E]
    return DE(f"E{E}-{odt}-{h}x{w}" + ("-scaled" if emb_scale else ""), E, odt, 2, h, w, col0, cstore(width, odt), emb_scale)


DE_ALL = tuple(_de(E, odt, h, w) for E in (6, 16, 128) for odt in DTS for (h, w) in DE_MAPS) + tuple(_de(16, odt, 7, 9, ROMA_EMB_SCALE) for odt in DTS)


@functools.lru_cache(maxsize=None)
def de_inputs(c):
    """(flow [B,h,w,2]: image 0 the grid itself, image 1 the grid + noise; wgt [E,2]; bias [E])"""
    g = torch.Generator().manual_seed(5400 + c.E)
    flow = grid(c.B, c.h, c.w).clone()
    flow[1:] += 0.1 * torch.randn(c.B - 1, c.h, c.w, 2, generator=g)
    return flow, torch.randn(c.E, 2, generator=g), torch.randn(c.E, generator=g)


@functools.lru_cache(maxsize=None)
def de_ref(c):
    """rows [B*h*w, E]; with emb_scale as RoMa applies it: to the displacement, not to the weights"""
    flow, wgt, bias = de_inputs(c)
    d = flow.permute(0, 3, 1, 2) - O.grid_coords(c.B, c.h, c.w)
    if c.emb_scale:
        d = c.emb_scale * d
    return F.conv2d(d, wgt[:, :, None, None], bias).permute(0, 2, 3, 1).reshape(-1, c.E).contiguous()


# ------------------------------------------------------------------------------------------------------------ resize_bilinear
RS = collections.namedtuple("RS", "id C dt odt B src dst")
RS_SIZES = (((7, 9), (14, 18)), ((2, 3), (32, 48)), ((6, 5), (6, 5)), ((13, 17), (5, 6)), ((1, 5), (3, 9)))
RS_PAIRS = (("fp32", "fp32"),) + tuple(p for k in H16 for p in ((k, k), (k, "fp32"), ("fp32", k)))


def _rs(C, dt, odt, src, dst):
    return RS(f"C{C}-{dt}-to-{odt}-{src[0]}x{src[1]}-to-{dst[0]}x{dst[1]}", C, dt, odt, 2, src, dst)


RS_ALL = tuple(_rs(8, a, b, s, d) for (a, b) in RS_PAIRS for (s, d) in RS_SIZES) + tuple(_rs(C, "fp32", "fp32", s, d) for C in (1, 2) for (s, d) in RS_SIZES)


@functools.lru_cache(maxsize=None)
def rs_input(c):
    """[B,C,h,w] fp32 container of dt-rounded values"""
    return rounded(torch.randn(c.B, c.C, *c.src, generator=torch.Generator().manual_seed(5500 + c.C)), c.dt)


@functools.lru_cache(maxsize=None)
def rs_ref(c):
    """[B,Ho,Wo,C]"""
    return F.interpolate(rs_input(c), size=c.dst, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------ the composed row
ROW = collections.namedtuple("ROW", "id scale dt B h w")
ROW_ALL = tuple(ROW(f"scale4-{dt}", "4", dt, 2, 5, 7) for dt in H16)


@functools.lru_cache(maxsize=None)
def row_inputs(c):
    """(x, y [B,C,h,w] dt-rounded, flow [B,h,w,2], emb weights [E,2], emb bias [E])"""
    ch, e, _ = REFINER_DKM[c.scale]
    g = torch.Generator().manual_seed(5600)
    x = rounded(torch.randn(c.B, ch, c.h, c.w, generator=g), c.dt)
    y = rounded(torch.randn(c.B, ch, c.h, c.w, generator=g), c.dt)
    flow = grid(c.B, c.h, c.w) + 0.3 * torch.randn(c.B, c.h, c.w, 2, generator=g)
    return x, y, flow, torch.randn(e, 2, generator=g), torch.randn(e, generator=g)


@functools.lru_cache(maxsize=None)
def row_ref(c):
    """-> {segment: rows [B*h*w, width]} of cat[x, grid_sample(y), emb, local_corr] (dkm.py:75-123)"""
    ch, e, r = REFINER_DKM[c.scale]
    x, y, flow, wgt, bias = row_inputs(c)
    fl = flow.permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(c.B * c.h * c.w, -1).contiguous()   # noqa: E731
    return {"x": rows(x), "gs": rows(F.grid_sample(y, flow, align_corners=False)),
            "emb": rows(F.conv2d(fl - O.grid_coords(c.B, c.h, c.w), wgt[:, :, None, None], bias)),
            "corr": rows(O.local_correlation(x, y, r, fl))}
