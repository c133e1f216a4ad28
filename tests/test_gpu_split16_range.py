"""The fp32 split-product GEMM (gim_conv_args.split16, Igemm::compute_split16) at the edges of IEEE fp16's range, against a plain torch model of
its arithmetic and against fp64:

  * the model: hi = rn16(v), lo = rn16(v - hi) of every activation x and of every weight times wscale = 4096, the three products
    hi hi + hi lo + lo hi summed in fp64, divided by wscale.  Kernel against model must agree to fp32 accumulation noise, a bound derived from
    sum |x| |w| at the launch's K (printed); that catches flushed fp16 subnormals, a wrong hi / lo pairing and a missing or doubled wscale.  Where the
    low halves are fp16 subnormals the test also checks that the kernel is much closer to the model than to the same model with subnormal inputs
    flushed (the 16-bit MFMA's A / B inputs keep them);
  * model against fp64: the accuracy the header documents (include/gim_hip.h, split16) per activation band -- the floor of the layers whose
    activations are all small;
  * the range: x = 65519 (hi = 65504, lo = 15) is exact; x = 65520 and a weight of 16.0 split into infinities, and the launch must say so through
    bit 8 of its `health` word (version 114), also under ReLU, which turns the NaN accumulators into plain zeros;
  * split16 = 0 with fp32 operands and a 16-bit output on the tile use_lds_dma = 3 picks (the 256 x 256 tile had no exact-product loop: version 113
    ran the split loop with wscale = 1 there) -- exact products, every element within one output ulp of the fp64 result.
Launch shapes: a 3 x 3 convolution (K = 576) and the strided-row ops.linear, on the 128 x 128 and the 256 x 256 tile (ops.FORCE_BIG_TILE), N = 256
and N = 196 (the SKIP variant), with and without a residual where the tile takes one."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
WSCALE = 4096.0


def _halves(v, flush=False):
    """fp32 tensor -> (hi, lo) as float64, hi = rn16(v), lo = rn16(v - hi) (the subtraction in fp32, as the kernel does it)"""
    hi = v.half()
    lo = (v - hi.float()).half()
    if flush:   # what an MFMA that flushed fp16-subnormal A / B inputs would multiply
        tiny = 2.0 ** -14
        hi = torch.where(hi.float().abs() < tiny, torch.zeros_like(hi), hi)
        lo = torch.where(lo.float().abs() < tiny, torch.zeros_like(lo), lo)
    return hi.double(), lo.double()


def split_model(x, w, bias, stride, pad, flush=False):
    """x [B,H,W,cin] fp32, w [cout,cin,k,k] fp32 -> [B,Ho,Wo,cout] float64: the split arithmetic of the kernel (before residual / activation)"""
    xh, xl = _halves(x.permute(0, 3, 1, 2).contiguous(), flush)
    wh, wl = _halves(w * WSCALE, flush)
    conv = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)  # noqa: E731
    acc = conv(xh, wh) + conv(xh, wl) + conv(xl, wh)
    return (acc / WSCALE + bias.double()[None, :, None, None]).permute(0, 2, 3, 1)


def fp64_conv(x, w, bias, stride, pad):
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)


def accum_bound(x, w, bias, stride, pad):
    """fp32 accumulation noise of the kernel: the three products of a K step are exact in fp32 (11 x 11 bits), the accumulators take 3 K / 16
    MFMA updates of 16 products each; a random-walk bound 4 sqrt(3 K) u sum |x| |w| (every product counted as a rounding step: the MFMA's internal
    summation order is not documented) plus the output's own rounding"""
    K = w[0].numel()
    sabs = F.conv2d(x.permute(0, 3, 1, 2).double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    return 4.0 * math.sqrt(3 * K) * U32 * sabs, K


# activation bands (|x| log-uniform in [lo, hi], random signs, a quarter zeros) -> model vs fp64 bound (max error / output scale), the accuracy the
# header documents; `sub`: the low halves (or the values themselves) are fp16 subnormals -- the flushed model must lie far from the kernel
BANDS = {
    "wide": ((1.2e-4, 148.0), 4e-7, False),     # today's test_gpu_split16 band
    "mid": ((1e-3, 1e-1), 2e-6, True),          # lo subnormal
    "low": ((1e-5, 5e-5), 3e-3, True),          # hi subnormal too
    "tiny": ((1e-7, 1e-6), 0.15, True),
}
WEIGHTS = {
    "normal": None,
    "tiny": (1e-10, 1e-8),     # w * 4096 below 6.1e-5: the weights' hi halves are subnormal
    "folded16": "edge",        # normal weights plus entries of |w| = 15.99 (a BatchNorm-folded filter just inside the range)
}


def _x(shape, band, g):
    lo, hi = band
    mag = torch.exp(torch.rand(shape, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))
    return mag * (torch.rand(shape, generator=g) > 0.25) * torch.sign(torch.randn(shape, generator=g))


def _w(cout, cin, k, kind, g):
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    if kind == "tiny":
        lo, hi = WEIGHTS["tiny"]
        w = torch.exp(torch.rand(w.shape, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo)) * torch.sign(w)
    elif kind == "folded16":
        w.view(-1)[torch.randperm(w.numel(), generator=g)[:64]] = 15.99 * torch.sign(torch.randn(64, generator=g))
    return w


def _run(x, pk, act, res=None, big=False, split=True, out_dtype=None, health=None, linear=False):
    from gim_amd import ops
    old = (ops.FORCE_BIG_TILE, ops.FP32_SPLIT)
    ops.FORCE_BIG_TILE, ops.FP32_SPLIT = big, split
    try:
        if linear:
            y = torch.empty(x.shape[0], pk.n_store, device=x.device)
            ops.linear(x, pk, y, act, True, health=health)
        else:
            y = ops.conv2d(x, pk, act, res=res, out_dtype=out_dtype, health=health)
        torch.cuda.synchronize()
    finally:
        ops.FORCE_BIG_TILE, ops.FP32_SPLIT = old
    return y


def _conv_case(band, wkind, cout, seed, B=1, H=16, W=24, cin=64, k=3):
    from gim_amd import _lib
    from gim_amd.packing import cstore, pack_conv
    g = torch.Generator().manual_seed(seed)
    w = _w(cout, cin, k, wkind, g)
    bias = torch.randn(cout, generator=g) * 0.1 * BANDS[band][0][1] * (1.0 if wkind != "tiny" else 1e-8)   # of the band's output size
    x = _x((B, H, W, cin), BANDS[band][0], g)
    xs = torch.zeros(B, H, W, cstore(cin, _lib.GIM_F32))
    xs[..., :cin] = x
    pk = pack_conv(w, None, _lib.GIM_F32, torch.device("cuda:0"), stride=1, pad=k // 2, bias=bias)
    return x, xs, w, bias, pk


def _check_vs_model(tag, got, x, w, bias, pad, res=None, act=None):
    """kernel vs model within the accumulation bound, model vs fp64 within the band's documented bound; returns the errors"""
    model = split_model(x, w, bias, 1, pad)
    ref = fp64_conv(x, w, bias, 1, pad)
    tol, K = accum_bound(x, w, bias, 1, pad)
    flushed = split_model(x, w, bias, 1, pad, flush=True)
    if res is not None:
        model, ref, flushed = model + res, ref + res, flushed + res
        tol = tol + U32 * res.abs()
    if act is not None:
        model, ref, flushed = act(model), act(ref), act(flushed)
    cout = w.shape[0]
    got = got[..., :cout].double().cpu()
    scale = ref.abs().max().item()
    d = (got - model).abs()
    ratio = (d / (tol + U32 * model.abs() + 1e-300)).max().item()
    e_model = (model - ref).abs().max().item() / scale
    e_kernel = d.max().item() / scale
    e_flush = (flushed - model).abs().max().item() / scale
    print(f"[split16 range] {tag} K={K}: kernel-model {e_kernel:.2e} of scale ({ratio:.3f} of the bound 4 sqrt(3K) u sum|x||w|, "
          f"mean bound {tol.mean().item() / scale:.1e}); model-fp64 {e_model:.2e}; flushed model-model {e_flush:.2e}")
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (tag, ratio)
    return e_kernel, e_model, e_flush


CONV = [(256, False), (256, True), (196, True), (256, "res")]   # (cout, big): 128 tile, 256 tile, 256 tile SKIP (N = 196), 128 tile + residual


@pytest.mark.parametrize("cout,big", CONV, ids=["n256-tile128", "n256-tile256", "n196-tile256-skip", "n256-tile128-res"])
@pytest.mark.parametrize("band", list(BANDS))
def test_split16_bands_vs_model_and_fp64(band, cout, big):
    from gim_amd import ops
    x, xs, w, bias, pk = _conv_case(band, "normal", cout, seed=11)
    res = None
    if big == "res":
        g = torch.Generator().manual_seed(5)
        res = torch.randn(1, 16, 24, pk.n_store, generator=g) * float(fp64_conv(x, w, bias, 1, 1).abs().max())
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = _run(xs.cuda(), pk, ops.ACT_NONE, res=res.cuda() if res is not None else None, big=big is True, health=hw)
    e_kernel, e_model, e_flush = _check_vs_model(f"{band} n{cout} {big}", y, x, w, bias, 1, res=res[..., :cout].double() if res is not None else None)
    assert int(hw.item()) == 0
    if res is None:
        assert e_model <= BANDS[band][1], (band, e_model)
    if BANDS[band][2]:
        # the kernel keeps fp16-subnormal operands: it sits much closer to the model than the flushed model does
        assert e_flush > 0 and e_kernel < 0.05 * e_flush, (band, e_kernel, e_flush)


@pytest.mark.parametrize("big", [False, True], ids=["tile128", "tile256"])
@pytest.mark.parametrize("wkind", ["tiny", "folded16"])
def test_split16_weight_edges_vs_model(wkind, big):
    """w * 4096 below the fp16 normals (the weights' hi halves are subnormal) and folded |w| = 15.99 (hi = 65495, in range: no health bit)"""
    from gim_amd import ops
    x, xs, w, bias, pk = _conv_case("wide", wkind, 256, seed=23)
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = _run(xs.cuda(), pk, ops.ACT_NONE, big=big, health=hw)
    _, e_model, e_flush = _check_vs_model(f"weights {wkind} {'tile256' if big else 'tile128'}", y, x, w, bias, 1)
    assert int(hw.item()) == 0
    assert e_model <= (4e-7 if wkind == "folded16" else 5e-3), e_model


def _linear_case(band, seed, R=1000, K=256, N=256, ld=320):
    from gim_amd import _lib
    from gim_amd.packing import pack_conv
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    x = _x((R, K), BANDS[band][0], g)
    buf = torch.zeros(R, ld)
    buf[:, :K] = x
    pk = pack_conv(w.view(N, K, 1, 1), None, _lib.GIM_F32, torch.device("cuda:0"))
    return x, buf, w, pk


@pytest.mark.parametrize("band", list(BANDS))
def test_split16_linear_rows_bands(band):
    """the strided-row linear (row stride 320 > K = 256) of the fp32 token projections"""
    from gim_amd import ops
    x, buf, w, pk = _linear_case(band, seed=31)
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = _run(buf.cuda()[:, :256], pk, ops.ACT_NONE, health=hw, linear=True)
    xi = x.view(1, 1, -1, 256)
    _, e_model, e_flush = _check_vs_model(f"linear {band}", y.view(1, 1, -1, pk.n_store), xi, w.view(256, 256, 1, 1), torch.zeros(256), 0)
    assert int(hw.item()) == 0
    assert e_model <= BANDS[band][1], (band, e_model)


# ---- the range edge ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True], ids=["tile128", "tile256"])
def test_split16_x_65519_is_exact(big):
    """rn16(65519) = 65504, lo = 15: the largest activations that split finitely; no health bit, values to the accumulation bound"""
    from gim_amd import ops
    x, xs, w, bias, pk = _conv_case("wide", "normal", 256, seed=41)
    x[0, 3:6, 4:9, ::7] = 65519.0 * torch.sign(x[0, 3:6, 4:9, ::7] + 0.5)
    xs[..., :64] = x
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = _run(xs.cuda(), pk, ops.ACT_NONE, big=big, health=hw)
    hi, lo = _halves(torch.tensor([65519.0, -65519.0]))
    assert hi.tolist() == [65504.0, -65504.0] and (hi + lo).tolist() == [65519.0, -65519.0]   # the split itself is exact
    _, e_model, _ = _check_vs_model("x = 65519", y, x, w, bias, 1)
    assert e_model <= 2e-7
    # against fp64 directly: the accumulation bound alone
    ref = fp64_conv(x, w, bias, 1, 1)
    tol, _ = accum_bound(x, w, bias, 1, 1)
    assert ((y[..., :256].double().cpu() - ref).abs() <= tol + U32 * ref.abs()).all()
    assert int(hw.item()) == 0


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("where", ["x65520", "w16"])
@pytest.mark.parametrize("big", [False, True], ids=["tile128", "tile256"])
def test_split16_overflow_sets_health_bit8(big, where, act):
    """x = 65520 (rn16 = inf) in one pixel, or a weight of 16.0 (16 * 4096 = 65536 -> inf) in one output channel: the accumulators of that
    pixel's 3 x 3 neighbourhood (every channel) or of that channel (every pixel) are NaN -- the model says so too -- and the launch ORs 8 into its
    health word.  Under ReLU the stored values there are plain 0 (fmaxf(NaN, 0)): only the bit tells.  Every other output is untouched."""
    from gim_amd import ops
    x, xs, w, bias, pk = _conv_case("wide", "normal", 256, seed=43)
    if where == "x65520":
        x[0, 7, 11, 5] = 65520.0
        xs[..., :64] = x
    else:
        w[37, 2, 1, 1] = 16.0
        from gim_amd import _lib
        from gim_amd.packing import pack_conv
        pk = pack_conv(w, None, _lib.GIM_F32, torch.device("cuda:0"), stride=1, pad=1, bias=bias)
    actc = ops.ACT_RELU if act == "relu" else ops.ACT_NONE
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    hw[0] = 1 | 4   # bits that other launches own: OR-ed into, never cleared
    y = _run(xs.cuda(), pk, actc, big=big, health=hw)[..., :256].double().cpu()
    assert int(hw.item()) == 1 | 4 | 8
    model = split_model(x, w, bias, 1, 1)
    bad = torch.isnan(model)
    assert bad.any() and torch.isnan(model).sum() == (9 * 256 if where == "x65520" else 16 * 24)
    if act == "relu":
        assert torch.equal(y[bad], torch.zeros_like(y[bad]))   # silently zero: what bit 8 exists for
        model = F.relu(model)
    else:
        assert torch.isnan(y[bad]).all()
    tol, _ = accum_bound(x, w, bias, 1, 1)
    ok = ~bad
    assert ((y[ok] - model[ok]).abs() <= tol[ok] + U32 * model[ok].abs()).all()
    # the same launch without a health word still runs (NULL: no check)
    _run(xs.cuda(), pk, actc, big=big, health=None)


def test_split16_linear_overflow_sets_health_bit8():
    from gim_amd import ops
    x, buf, w, pk = _linear_case("wide", seed=47)
    buf[123, 17] = -7e4
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = _run(buf.cuda()[:, :256], pk, ops.ACT_RELU, health=hw, linear=True).cpu()
    assert int(hw.item()) == 8
    assert torch.equal(y[123, :256], torch.zeros(256))   # every column of that row: NaN -> ReLU -> 0
    # exact products take the row: no bit, the real values
    hw.zero_()
    ye = _run(buf.cuda()[:, :256], pk, ops.ACT_RELU, health=hw, linear=True, split=False).cpu()
    assert int(hw.item()) == 0
    ref = F.relu(buf[:, :256].double() @ w.double().t())
    assert ((ye[:, :256].double() - ref).abs().max() / ref.abs().max()).item() <= 2e-6 and ye[123, :256].abs().max() > 0


# ---- split16 = 0: exact products whatever tile the launch lands on ----------------------------------------------------------------------
@pytest.mark.parametrize("cout", [256, 200])
@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float16], ids=["bf16out", "fp16out"])
def test_exact_products_with_16bit_output_on_the_big_tile_path(odt, cout):
    """fp32 operands, split16 = 0, a 16-bit output, use_lds_dma = 3 (ops.FORCE_BIG_TILE): version 113 sent this launch to the 256 x 256 tile,
    whose K loop always split (wscale 1: |x| ~ 7e4 became inf, weights ~ 1e-6 fp16 subnormals).  Exact products: within one output ulp of the
    fp64 result, every element.  N = 200 is the SKIP variant's shape here (N <= npad - 32; a 16-bit output needs N % 8 == 0, so not 196)."""
    from gim_amd import _lib, ops
    from gim_amd.packing import cstore, pack_conv
    g = torch.Generator().manual_seed(53)
    cin = 64
    big_x = odt == torch.bfloat16   # (an fp16 output of |x| ~ 7e4 times 1e-6 weights over K = 576 stays inside fp16 either way)
    w = (torch.rand(cout, cin, 3, 3, generator=g) + 0.5) * 1e-6 * torch.sign(torch.randn(cout, cin, 3, 3, generator=g))
    bias = torch.randn(cout, generator=g) * 0.01
    x = (torch.rand(2, 16, 24, cin, generator=g) * 4e4 + 5e4) * torch.sign(torch.randn(2, 16, 24, cin, generator=g))
    if not big_x:
        x = x / 4.0
    xs = torch.zeros(2, 16, 24, cstore(cin, _lib.GIM_F32))
    xs[..., :cin] = x
    pk = pack_conv(w, None, _lib.GIM_F32, torch.device("cuda:0"), stride=1, pad=1, bias=bias)
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = _run(xs.cuda(), pk, ops.ACT_NONE, big=True, split=False, out_dtype=odt, health=hw)[..., :cout].cpu()
    ref = fp64_conv(x, w, bias, 1, 1)
    r16 = ref.to(odt)
    up = torch.nextafter(r16, torch.full_like(r16, float("inf"))).double() - r16.double()
    down = r16.double() - torch.nextafter(r16, torch.full_like(r16, float("-inf"))).double()
    ulp = torch.maximum(up.abs(), down.abs())   # (at a power of two the spacing differs on either side)
    # (+ the exact-product fp32 accumulation, <= 2^-21 sum |x| |w|: it decides only outputs that cancel to near zero)
    tol = ulp + 2.0 ** -21 * F.conv2d(x.permute(0, 3, 1, 2).double().abs(), w.double().abs(), bias.double().abs(), padding=1).permute(0, 2, 3, 1)
    err = (y.double() - ref).abs()
    print(f"[split16 range] split16=0 {odt} n{cout}: max err {err.max().item():.3e}, max err / ulp {(err / ulp).max().item():.3f}, "
          f"max err / tolerance {(err / tol).max().item():.3f}")
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), (err / tol).max().item()
    assert int(hw.item()) == 0   # (no split launch: the word is not handed on)
