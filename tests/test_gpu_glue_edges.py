"""The small memory-bound kernels between the heavy ones, at their edges: layernorm_kernel (both 256-channel halves, all four template
instances, strided and aliased operands), the two layout kernels (full and ragged 64 x 64 tiles, gray images, ld > C), upsample2x_add
(1-pixel sides), posenc_add (hw coprime to the block, one output at a time), fine_gather (unequal maps, every window size and stride),
fine_match (flat, saturated and offset softmax), the two max-pools (odd, 1- and 2-pixel sides, all-negative maps) and the two bilinear
resizes in every (input kind, output kind) pair.  Shapes, inputs and float64 references: tests/glue_cases.py, held to the torch ops and
the oracle on the host by tests/test_glue_cases_cpu.py.

Every output buffer is prefilled with NaN: columns beyond the written width, rows beyond the written count and images outside the
written range must still be NaN afterwards; a column a kernel documents as zero padding must be exactly 0.  Where ops.* always passes
C as the leading dimension the entry point is called through _lib.lib with its committed prototype.

Bars (glue_cases): copy, max and gather kernels bit exact; fp32 outputs of computing kernels 4 x the fp32 torch op's own error on the
same case + one fp32 ulp of the output scale; 16-bit outputs per element within one ulp of the stored kind of the rounded float64
reference -- of what rounding a value within the fp32 bar can give (check16's `loose` count; its `strict` count, one ulp of round16(ref)
whatever the element's size, is printed: fp32 F.layer_norm itself misses it on elements that cancel to nearly nothing).

Measured on an MI355X (`[ratio]` lines of pytest -s: largest GPU error / bar over the cases of a kernel, and GPU error / error of the
fp32 torch op where that error makes the bar):
    layernorm          0.37 of the bar (fp16, C = 4), 2.7 x F.layer_norm's error; 1000 + randn rows 0.61 (C = 260), 2.5 x
    upsample2x_add     0.17, 1.0 x
    resize_bilinear    0.37, 2.7 x (fp32 -> fp32); resize_image 0.26, 1.2 x
    fine_match         0.51 (W = 7), 3.8 x (W = 3) -- with one fmaf chain over C in fine_match_kernel the large-offset regime (every
                       similarity + 80, C = 128) was at 1.44 of the bar = 6.0 x loftr_oracle.fine_matching's error (8.0e-6 against 1.3e-6
                       in expec_f, W = 3, M = 4): the kernel sums four partial chains since
    16-bit outputs     `loose` count 0 everywhere.  `strict` count: layernorm on 3 randn + 0.5 rows bf16 1, fp16 20 of 3.75e6 elements;
                       on 1000 + randn rows bf16 361, fp16 2778 of 3.2e5; upsample2x_add bf16 6, fp16 1 of 1.3e5; the resizes 0
    everything else (layouts, posenc_add, fine_gather, the max-pools, identity resizes, constant LayerNorm rows) is exact"""
import pytest
import torch

import glue_cases as G

pytestmark = pytest.mark.gpu
NAN = G.NAN


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _gim(dt):
    from gim_amd import _lib
    return {"bf16": _lib.GIM_BF16, "fp16": _lib.GIM_F16, "fp32": _lib.GIM_F32}[dt]


def _nan(shape, dt, dev):
    return torch.full(shape, NAN, dtype=G.TDT[dt], device=dev)


def _call(name, *args):
    """an entry point through its committed ctypes prototype, on the current stream; raises GimHipError on a refusal"""
    from gim_amd import _lib, ops
    _lib.check(getattr(_lib.lib, name)(*[ops._p(a) if (a is None or torch.is_tensor(a)) else a for a in args], ops._stream()), name)


def _nan_outside(buf, rows, cols, what):
    """buf [Rtot, ld]: everything outside [0:rows, cols] is still NaN"""
    b = buf.detach().float().cpu()
    keep = torch.ones(b.shape, dtype=torch.bool)
    keep[:rows, cols] = False
    assert torch.isnan(b[keep]).all(), f"{what}: wrote outside its rows / columns"


def _rows(x, ld, dt, dev, seed=0):
    """[B,C,H,W] host values of the kind -> device [B*H*W, ld] rows of the kind, random junk in the columns >= C"""
    B, C, H, W = x.shape
    buf = torch.randn(B * H * W, ld, generator=G.gen(1234 + seed))
    buf[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    return buf.to(G.TDT[dt]).to(dev)


class _Worst:
    """largest GPU error / bar of a test, printed as one `[ratio]` line"""

    def __init__(self, kernel):
        self.kernel, self.ratio, self.vs_cpu, self.strict, self.n16 = kernel, 0.0, 0.0, 0, 0

    def close32(self, got, ref64, cpu_err, what):
        got = got.detach().cpu()
        assert got.dtype == torch.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
        assert torch.isfinite(got).all(), f"{what}: non-finite output"
        bar = G.bar32(cpu_err, ref64.abs().max().item() if ref64.numel() else 0.0)
        err = G.max_err(got, ref64)
        print(f"[close] {what}: gpu {err:.3e} cpu {cpu_err:.3e} (bar {bar:.3e})")
        self.ratio = max(self.ratio, err / bar if bar else 0.0)
        if cpu_err > bar / 8:      # where the fp32 op's error, not the ulp term, makes the bar
            self.vs_cpu = max(self.vs_cpu, err / cpu_err)
        assert err <= bar, f"{what}: gpu err {err:.3e} > bar {bar:.3e} (fp32 torch op: {cpu_err:.3e})"
        return bar

    def close16(self, got, ref64, dt, bar, what):
        strict, loose = G.check16(got, ref64, dt, bar)
        self.strict, self.n16 = self.strict + strict, self.n16 + ref64.numel()
        if strict:
            print(f"[close] {what}: {strict} of {ref64.numel()} elements beyond one {dt} ulp of round(ref) (fp32 bar {bar:.3e})")
        assert loose == 0, f"{what}: {loose} elements beyond one {dt} ulp of what rounding ref +- {bar:.3e} gives"

    def report(self, tag=""):
        print(f"[ratio] {self.kernel} {tag}: err/bar {self.ratio:.3f}, err/cpu_err {self.vs_cpu:.2f}, 16-bit strict misses {self.strict} of {self.n16}")


def _exact(got, ref64, dt, what):
    """bit exact against the reference rounded to the stored kind"""
    got = got.detach().cpu()
    assert got.dtype == G.TDT[dt] and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    assert torch.equal(got, ref64.to(G.TDT[dt])), f"{what}: not exact ({int((got != ref64.to(G.TDT[dt])).sum())} elements differ)"


# ------------------------------------------------------------------------------------------------------------ layernorm
def _ln_launch(dev, dt, C, R, xdt, variant, eps, kind="randn"):
    """one launch in the model's layout: x and res column slices of 2C-wide buffers, out_t a column slice, two spare rows.
    -> (out_f32 buffer | None, out_t buffer | None)"""
    from gim_amd import ops
    x, gamma, beta, res = G.ln_inputs(C, R, kind, xdt)
    xb = torch.full((R, 2 * C), 7.0, dtype=G.TDT[xdt], device=dev)
    xb[:, C:] = x.to(dev)
    rb = torch.full((R + 2, 2 * C), NAN, device=dev)
    rb[:R, :C] = res.to(dev)
    o32 = None if variant == "no_f32" else (rb if variant == "inplace" else _nan((R + 2, 2 * C), "fp32", dev))
    ot = None if variant == "no_t" else _nan((R + 2, 2 * C), dt, dev)
    ops.layernorm_residual(xb[:, C:], gamma.to(dev), beta.to(dev), None if variant == "no_res" else rb[:R, :C],
                           o32[:R, :C] if o32 is not None else None, ot[:R, C:] if ot is not None else None, eps)
    torch.cuda.synchronize()
    return o32, ot


def _ln_check(w, o32, ot, dt, C, R, xdt, variant, eps, kind="randn"):
    ref, cpu_err = G.ln_ref(C, R, kind, xdt, variant != "no_res", eps)
    what = f"layernorm {dt} C={C} R={R} x={xdt} {variant} eps={eps:g} {kind}"
    bar = G.bar32(cpu_err, ref.abs().max().item())
    if o32 is not None:
        w.close32(o32[:R, :C], ref, cpu_err, what + " f32")
        _nan_outside(o32, R, slice(0, C), what + " f32")
    if ot is not None:
        if dt == "fp32":
            w.close32(ot[:R, C:], ref, cpu_err, what + " T")
        else:
            w.close16(ot[:R, C:], ref, dt, bar, what + " T")
        _nan_outside(ot, R, slice(C, 2 * C), what + " T")


@pytest.mark.parametrize("C", G.LN_C)
@pytest.mark.parametrize("dt", G.DTS)
def test_layernorm(dt, C):
    dev, w = _dev(), _Worst("layernorm")
    for R, xdt, variant, eps in G.ln_plan(dt, C):
        o32, ot = _ln_launch(dev, dt, C, R, xdt, variant, eps)
        _ln_check(w, o32, ot, dt, C, R, xdt, variant, eps)
        if variant == "inplace":       # res and out_f32 the same rows (loftr.py: T.X32): bit for bit the out-of-place result
            p32, pt = _ln_launch(dev, dt, C, R, xdt, "all", eps)
            assert torch.equal(o32[:R, :C], p32[:R, :C]) and torch.equal(ot[:R, C:], pt[:R, C:]), (C, R, xdt)
    w.report(f"{dt} C={C}")


@pytest.mark.parametrize("C", (260, 512))
@pytest.mark.parametrize("dt", G.DTS)
def test_layernorm_offset_and_constant_rows(dt, C):
    """x = 1000 + randn: a mean large against the spread, judged by fp32 F.layer_norm's error on the same rows; constant rows: variance 0,
    the output is beta (+ res) exactly and finite"""
    dev, w = _dev(), _Worst("layernorm rows")
    for xdt in (("fp32",) if dt == "fp32" else ("fp32", dt)):
        for R in (5, 203):
            o32, ot = _ln_launch(dev, dt, C, R, xdt, "all", 1e-5, "offset")
            _ln_check(w, o32, ot, dt, C, R, xdt, "all", 1e-5, "offset")
        R = len(G.LN_CONST)
        _, gamma, beta, res = G.ln_inputs(C, R, "const", xdt)
        for variant in ("all", "no_res"):
            for eps in G.LN_EPS:
                o32, ot = _ln_launch(dev, dt, C, R, xdt, variant, eps, "const")
                want = (beta + res) if variant == "all" else beta.expand(R, C)
                assert torch.equal(o32[:R, :C].cpu(), want), (C, xdt, variant, eps)
                assert torch.equal(ot[:R, C:].cpu(), want.to(G.TDT[dt])), (C, xdt, variant, eps)
    w.report(f"{dt} C={C}")


@pytest.mark.parametrize("C", G.LN_REFUSED_C)
def test_layernorm_refuses(C):
    from gim_amd import _lib, ops
    dev = _dev()
    x, out = torch.zeros(4, round(C / 4 + 1) * 4, device=dev), _nan((4, 520), "fp32", dev)
    with pytest.raises(_lib.GimHipError, match="layernorm"):
        ops.layernorm_residual(x[:, :C], torch.ones(C, device=dev), torch.zeros(C, device=dev), None, out[:, :C], None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------------------ layout kernels
@pytest.mark.parametrize("dt", G.DTS)
def test_nhwc_to_nchw(dt):
    from gim_amd import ops
    dev = _dev()
    B = G.TO_NCHW_B
    for C in G.TO_NCHW_C:
        for ld in G.to_nchw_lds(C):
            for (H, W) in G.TO_NCHW_HW:
                rows = G.nhwc_rows(B, H, W, ld, dt, 100 + C)
                dst = _nan((B + 1, C, H, W), "fp32", dev)
                _call("gim_nhwc_to_nchw", rows.to(G.TDT[dt]).to(dev), dst, B, C, H, W, ld, _gim(dt))
                torch.cuda.synchronize()
                _exact(dst[:B], G.ref_nhwc_to_nchw(rows, C), "fp32", f"nhwc_to_nchw {dt} C={C} ld={ld} {H}x{W}")
                assert torch.isnan(dst[B]).all(), (C, ld, H, W)
                if ld == G.to_nchw_lds(C)[1] and (H, W) == (10, 13):        # the wrapper: ld from the tensor's last dimension
                    assert torch.equal(ops.nhwc_to_nchw(rows.to(G.TDT[dt]).to(dev), C), dst[:B])


@pytest.mark.parametrize("dt", G.DTS)
def test_nchw_to_nhwc(dt):
    dev = _dev()
    B, N = G.TO_NHWC_B, G.TO_NHWC_IMAGES
    for C, cpad, ld, b_off, (H, W) in G.to_nhwc_cases():
        src = G.nchw_image(B, C, H, W, 200 + C)
        dst = _nan((N, H * W, ld), dt, dev)
        _call("gim_nchw_to_nhwc", src.to(dev), dst, B, C, H, W, cpad, ld, b_off, _gim(dt))
        torch.cuda.synchronize()
        what = f"nchw_to_nhwc {dt} C={C} cpad={cpad} ld={ld} b_off={b_off} {H}x{W}"
        ref = G.ref_nchw_to_nhwc(src, cpad).reshape(B, H * W, cpad)
        _exact(dst[b_off:b_off + B, :, :cpad], ref, dt, what)                # channels [C, cpad) exactly 0
        assert (dst[b_off:b_off + B, :, C:cpad].float() == 0).all(), what
        assert torch.isnan(dst[b_off:b_off + B, :, cpad:].float()).all(), what + ": columns >= cpad written"
        other = [b for b in range(N) if not b_off <= b < b_off + B]
        assert torch.isnan(dst[other].float()).all(), what + ": images outside [b_off, b_off + B) written"


@pytest.mark.parametrize("dt", G.DTS)
def test_layout_roundtrip_196(dt):
    from gim_amd import ops
    dev = _dev()
    B, C, H, W = G.ROUNDTRIP
    x = G.nchw_image(B, C, H, W, 300)
    cs = G.cstore(C, dt)
    buf = _nan((B, H, W, cs), dt, dev)
    ops.nchw_to_nhwc(x.to(dev), buf)
    back = ops.nhwc_to_nchw(buf, C)
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), G.rnd(x, dt)) and (buf[..., C:].float() == 0).all()


# ------------------------------------------------------------------------------------------------------------ upsample2x_add
@pytest.mark.parametrize("dt", G.DTS)
def test_upsample2x_add(dt):
    dev, w = _dev(), _Worst("upsample2x_add")
    B = G.UPS_B
    for (h, wd) in G.UPS_HW:
        for C, cs in G.ups_channels(dt):
            lo, hi, ref, cpu_err = G.ups_case(h, wd, C, dt)
            ldx, ldy, n = cs + 8, cs + 16, B * 4 * h * wd
            pad = lambda t: torch.cat([t, torch.zeros(B, cs - C, *t.shape[2:])], 1)      # noqa: E731  stored channels beyond C: zeros
            x = _rows(pad(lo), ldx, dt, dev, seed=h)
            y = _nan((n + 2, ldy), dt, dev)
            y[:n, :cs] = pad(hi).permute(0, 2, 3, 1).reshape(n, cs).to(G.TDT[dt]).to(dev)
            _call("gim_upsample2x_add", x, y, B, h, wd, cs, ldx, ldy, _gim(dt))
            torch.cuda.synchronize()
            what = f"upsample2x_add {dt} {h}x{wd} C={C} ldx={ldx} ldy={ldy}"
            ref_rows = ref.permute(0, 2, 3, 1).reshape(n, C)
            if dt == "fp32":
                w.close32(y[:n, :C], ref_rows, cpu_err, what)
            else:
                w.close16(y[:n, :C], ref_rows, dt, G.bar32(cpu_err, ref.abs().max().item()), what)
            assert (y[:n, C:cs].float() == 0).all(), what
            _nan_outside(y, n, slice(0, cs), what)
    w.report(dt)


# ------------------------------------------------------------------------------------------------------------ posenc_add
@pytest.mark.parametrize("dt", G.DTS)
def test_posenc_add(dt):
    from gim_amd import ops
    dev = _dev()
    for hw in G.POSENC_HW:
        for nb in G.POSENC_NB:
            for C in G.POSENC_C:
                x, pe, ref = G.posenc_case(hw, nb, C, dt)
                R = nb * hw
                for outs in G.POSENC_OUTS:
                    o32 = _nan((R + 2, C + 4), "fp32", dev) if outs != "t" else None
                    ot = _nan((R + 2, 2 * C), dt, dev) if outs != "f32" else None
                    ops.posenc_add(x.to(G.TDT[dt]).to(dev), pe.to(dev), o32[:R, :C] if o32 is not None else None,
                                   ot[:R, C:] if ot is not None else None)
                    torch.cuda.synchronize()
                    what = f"posenc_add {dt} hw={hw} nb={nb} C={C} {outs}"
                    if o32 is not None:       # one fp32 rounding of the sum
                        _exact(o32[:R, :C], ref, "fp32", what + " f32")
                        _nan_outside(o32, R, slice(0, C), what + " f32")
                    if ot is not None:
                        if dt == "fp32":
                            _exact(ot[:R, C:], ref, "fp32", what + " T")
                        else:
                            assert G.check16(ot[:R, C:], ref, dt)[0] == 0, what + " T"
                        _nan_outside(ot, R, slice(C, 2 * C), what + " T")


# ------------------------------------------------------------------------------------------------------------ fine_gather
@pytest.mark.parametrize("dt", G.DTS)
def test_fine_gather(dt):
    dev = _dev()
    (h0, w0), (h1, w1) = G.FG_COARSE
    for W, stride, C, ldf, M, outs in G.fg_cases():
        f0, f1 = G.fg_maps(stride, C, dt)
        b, i, j = G.fg_ids(M)
        u0, u1 = G.ref_fine_gather(f0, f1, b, i, j, w0, w1, stride, W)
        ref = torch.cat([u0, u1], 0).reshape(-1, C).double()
        n = 2 * M * W * W
        o32 = _nan((n + 3, C + 4), "fp32", dev) if outs != "t" else None
        ot = _nan((n + 3, 2 * C), dt, dev) if outs != "f32" else None
        _call("gim_fine_gather", _rows(f0, ldf, dt, dev, 1), _rows(f1, ldf, dt, dev, 2), b.to(dev), i.to(dev), j.to(dev),
              o32, ot[:, C:] if ot is not None else None, M, stride * h0, stride * w0, stride * h1, stride * w1, C, ldf, w0, w1, stride, W,
              C + 4, 2 * C, _gim(dt))
        torch.cuda.synchronize()
        what = f"fine_gather {dt} W={W} stride={stride} C={C} ldf={ldf} M={M} {outs}"
        if o32 is not None:
            _exact(o32[:n, :C], ref, "fp32", what + " f32")
            _nan_outside(o32, n, slice(0, C), what + " f32")
        if ot is not None:
            _exact(ot[:n, C:], ref, dt, what + " T")
            _nan_outside(ot, n, slice(C, 2 * C), what + " T")


def test_fine_gather_refuses_even_windows():
    from gim_amd import _lib
    dev = _dev()
    f, ids, out = torch.zeros(1, 8, 8, 4, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), _nan((2 * 16, 4), "fp32", dev)
    for W in (2, 4):
        with pytest.raises(_lib.GimHipError, match="fine_gather"):
            _call("gim_fine_gather", f, f, ids, ids, ids, out, None, 1, 8, 8, 8, 8, 4, 4, 2, 2, 4, W, 4, 4, _gim("fp32"))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------------------ fine_match
@pytest.mark.parametrize("W", G.FM_W)
def test_fine_match(W):
    dev, w = _dev(), _Worst("fine_match")
    WW = W * W
    for C in G.FM_C:
        for M in G.FM_M:
            for regime in G.FM_REGIMES:
                f0, f1, mk, b, s1 = G.fm_inputs(W, C, M, regime)
                fb0, fb1 = torch.full((M * WW, 2 * C), 7.0, device=dev), torch.full((M * WW, 2 * C), -7.0, device=dev)
                fb0[:, C:], fb1[:, :C] = f0.reshape(-1, C).to(dev), f1.reshape(-1, C).to(dev)       # column slices: ld = 2C
                for has in (False, True):
                    e64, m64, cpu_e, cpu_m = G.fm_ref(W, C, M, regime, has)
                    expec, mk1 = _nan((M + 2, 3), "fp32", dev), _nan((M + 2, 2), "fp32", dev)
                    _call("gim_fine_match", fb0[:, C:], fb1[:, :C], mk.to(dev), b.to(dev), s1.to(dev), expec, mk1, M, WW, C, 2 * C,
                          G.FM_SCALE, int(has))
                    torch.cuda.synchronize()
                    what = f"fine_match W={W} C={C} M={M} {regime} scale0={int(has)}"
                    w.close32(expec[:M], e64, cpu_e, what + " expec_f")
                    w.close32(mk1[:M], m64, cpu_m, what + " mkpts1_f")
                    assert torch.isnan(expec[M:]).all() and torch.isnan(mk1[M:]).all(), what
                    if regime.startswith("sat"):      # every other expf underflows: the cell's own grid coordinate, variance exactly 0
                        r, e = G.fm_sat_cell(regime, W), expec[:M].cpu()
                        assert set(e[:, 0].tolist()) <= G.grid_coord_fp32(W, r % W) and set(e[:, 1].tolist()) <= G.grid_coord_fp32(W, r // W), (what, e)
                        assert (e[:, 2] == G.SAT_STD).all(), (what, e[:, 2])
    w.report(f"W={W}")


@pytest.mark.parametrize("WW", G.FM_REFUSED_WW)
def test_fine_match_refuses(WW):
    from gim_amd import _lib
    dev = _dev()
    f, mk = torch.zeros(WW, 4, device=dev), torch.zeros(1, 2, device=dev)
    expec, mk1 = _nan((1, 3), "fp32", dev), _nan((1, 2), "fp32", dev)
    with pytest.raises(_lib.GimHipError, match="fine_match"):
        _call("gim_fine_match", f, f, mk, None, None, expec, mk1, 1, WW, 4, 4, 2.0, 0)
    torch.cuda.synchronize()
    assert torch.isnan(expec).all() and torch.isnan(mk1).all()


# ------------------------------------------------------------------------------------------------------------ max-pools
@pytest.mark.parametrize("dt", G.DTS)
@pytest.mark.parametrize("kernel", ["maxpool2x2", "maxpool3x3s2"])
def test_maxpool(kernel, dt):
    dev = _dev()
    B = G.POOL_B
    k, pad, shapes = (2, 0, G.POOL2_HW) if kernel == "maxpool2x2" else (3, 1, G.POOL3_HW)
    for C in G.pool_channels(dt):
        for n_case, (H, W) in enumerate(shapes):
            for negative in ((False, True) if n_case in (1, len(shapes) - 1) else (False,)):
                x = G.pool_input(H, W, C, dt, negative)
                ref = G.ref_maxpool(x, k, 2, pad)
                Ho, Wo = ref.shape[2:]
                ldx, ldy, n = C + 8, C + 16, B * Ho * Wo
                y = _nan((n + 2, ldy), dt, dev)
                _call("gim_" + kernel, _rows(x, ldx, dt, dev, H), y, B, H, W, C, ldx, ldy, _gim(dt))
                torch.cuda.synchronize()
                what = f"{kernel} {dt} {H}x{W} C={C} negative={negative}"
                _exact(y[:n, :C], ref.permute(0, 2, 3, 1).reshape(n, C), dt, what)
                _nan_outside(y, n, slice(0, C), what)


# ------------------------------------------------------------------------------------------------------------ resizes
@pytest.mark.parametrize("pair", G.RESIZE_PAIRS, ids=lambda p: f"{p[0]}-to-{p[1]}")
def test_resize_bilinear(pair):
    dev, w = _dev(), _Worst("resize_bilinear")
    idt, odt = pair
    B, C = G.RESIZE_B, G.RESIZE_C
    for n_case, (src, size) in enumerate(G.RESIZE_SHAPES):
        for ldx, ldy in ((8, 16), (16, 8)) if n_case % 2 else ((8, 8), (16, 16)):
            x, ref, cpu_err = G.resize_case(src, size, C, idt)
            n = B * size[0] * size[1]
            y = _nan((n + 2, ldy), odt, dev)
            _call("gim_resize_bilinear", _rows(x, ldx, idt, dev, n_case), y, B, src[0], src[1], size[0], size[1], C, ldx, ldy, _gim(idt), _gim(odt))
            torch.cuda.synchronize()
            what = f"resize_bilinear {idt}->{odt} {src}->{size} ldx={ldx} ldy={ldy}"
            ref_rows = ref.permute(0, 2, 3, 1).reshape(n, C)
            if src == size:
                _exact(y[:n, :C], ref_rows, odt, what + " (identity)")
            elif odt == "fp32":
                w.close32(y[:n, :C], ref_rows, cpu_err, what)
            else:
                w.close16(y[:n, :C], ref_rows, odt, G.bar32(cpu_err, ref.abs().max().item()), what)
            _nan_outside(y, n, slice(0, C), what)
    w.report(f"{idt}->{odt}")


@pytest.mark.parametrize("odt", G.DTS)
def test_resize_image(odt):
    dev, w = _dev(), _Worst("resize_image")
    B, N = G.RESIZE_B, G.RESIZE_IMAGE_IMAGES
    for n_case, (src, size) in enumerate(G.RESIZE_SHAPES):
        for C in G.RESIZE_IMAGE_C:
            for cpad in G.RESIZE_IMAGE_CPAD:
                b_off = G.RESIZE_IMAGE_BOFF[(n_case + C + cpad // 4) % 2]
                x, ref, cpu_err = G.resize_case(src, size, C, "fp32")
                dst = _nan((N, size[0], size[1], cpad), odt, dev)
                _call("gim_resize_image", x.to(dev), dst, B, C, src[0], src[1], size[0], size[1], cpad, b_off, _gim(odt))
                torch.cuda.synchronize()
                what = f"resize_image ->{odt} {src}->{size} C={C} cpad={cpad} b_off={b_off}"
                got, ref_rows = dst[b_off:b_off + B, ..., :C], ref.permute(0, 2, 3, 1)
                if src == size:
                    _exact(got, ref_rows, odt, what + " (identity)")
                elif odt == "fp32":
                    w.close32(got, ref_rows, cpu_err, what)
                else:
                    w.close16(got, ref_rows, odt, G.bar32(cpu_err, ref.abs().max().item()), what)
                assert (dst[b_off:b_off + B, ..., C:].float() == 0).all(), what + ": padding channels"
                other = [b for b in range(N) if not b_off <= b < b_off + B]
                assert torch.isnan(dst[other].float()).all(), what + ": images outside [b_off, b_off + B) written"
    w.report(f"->{odt}")
