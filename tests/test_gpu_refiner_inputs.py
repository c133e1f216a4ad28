"""The four gather kernels that assemble the ConvRefiner's input row (gim_amd.dense.refine: ops.grid_sample, ops.dkm_disp_emb,
ops.local_corr; ops.resize_bilinear between the scales), through gim_amd.ops, in the dtypes, channel widths, column slices and row
strides the two dense matchers run them with, and at the edges of their hand-written bounds handling.  Cases, references (CPU, fp32, on
operands already rounded to the kernel's dtype) and the derived bounds are tests/refiner_input_cases.py; every comparison covers every
output element and prints its worst |got - ref| / bound.

Measured on MI355X, worst |got - ref| / bound per kernel (the bound is 1; `pytest -s` prints every case):
                     fp32 out   bf16 out   fp16 out
    local_corr         0.066      0.975      0.898      (composed row: 0.901 / 0.846)
    grid_sample        0.000      0.988      0.979      (composed row: 0.986 / 0.964; fp32 differs from the reference below 5e-4 of its bar)
    dkm_disp_emb       0.042      0.989      0.987      (composed row: 0.969 / 0.953)
    resize_bilinear    0.060      0.995      0.977
A 16-bit ratio just below 1 is one rounding to nearest at an element near half an ulp; a truncating store gives ~2.  All 940 426
elements whose taps lie wholly outside the map are exactly zero, and no output is nonzero where a boundary tap of the reference is 0.

What these cases found: grid_sample with a grid value of +1e9 / +1e12 on one axis and an in-range value on the other read 2^31 pixels
outside the map (the float -> int conversion saturates at INT_MAX and x0 + 1 wraps); the kernel now clamps the floor to +-65536 before
the conversion, as local_corr does.  With the PT = 8 lane -> px decoding of local_corr_kernel swapped on a scratch build, every
r = 1, 2, 3 case and the composed row fail (ratios ~4e4) and the r = 7 / mixed-dtype (PT = 16) cases pass."""
import pytest
import torch

import refiner_input_cases as R

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _nhwc(x, dt):
    """[B,C,h,w] -> NHWC of dtype dt with the strides of a freshly allocated tensor (permute().contiguous() keeps stride 1 on a
    one-pixel axis, and ops.local_corr reads the pixel pitch from stride(2))"""
    B, C, h, w = x.shape
    return torch.empty(B, h, w, C, dtype=R.TDT[dt]).copy_(x.permute(0, 2, 3, 1))


def _check(got, ref, odt, kind, what, zero=None, scale=None):
    """every element within the derived bound; exactly zero where every tap lies outside the map"""
    ratio = R.worst_ratio(got, ref, odt, kind, scale)
    got = got.detach().float().cpu()
    extra = ""
    if zero is not None:
        zero = zero.expand_as(ref)
        nz = int((got[zero] != 0).sum())
        edge = int(((ref == 0) & ~zero & (got != 0)).sum())
        extra = f"; {int(zero.sum())} elements with every tap outside, {nz} of them nonzero; {edge} nonzero where the reference's boundary taps are 0"
    print(f"[refiner] {what}: worst |got - ref| / bound = {ratio:.3f}{extra}")
    assert ratio <= 1.0, f"{what}: worst |got - ref| / bound = {ratio:.3f}"
    if zero is not None:
        assert nz == 0, f"{what}: {nz} nonzero outputs where every tap lies outside the map"


def _slice_buffer(rows, col0, width, stride, dt, dev):
    buf = R.row_buffer(rows, stride, dt).to(dev)
    return buf, slice(col0, col0 + width)


# ------------------------------------------------------------------------------------------------------------ local_corr
@pytest.mark.parametrize("c", R.LC_ALL, ids=lambda c: c.id)
def test_local_corr(c):
    from gim_amd import ops
    dev = _dev()
    f0, f1, flow = R.lc_inputs(c)
    K = (2 * c.r + 1) ** 2
    if c.pad:       # channel-slice views of wider rows: ld0 = ld1 = C + pad, NaN in the padding
        a, b = (R.nan_padded(f.permute(0, 2, 3, 1), c.dt, c.pad)[0].to(dev)[..., :c.C] for f in (f0, f1))
        assert a.stride(2) == c.C + c.pad and a.shape[3] == c.C
    else:
        a, b = _nhwc(f0, c.dt).to(dev), _nhwc(f1, c.dt).to(dev)
    buf, sl = _slice_buffer(c.B * c.h * c.w, c.col0, K, c.stride, c.odt, dev)
    ops.local_corr(a, b, flow.to(dev), c.r, buf[:, c.col0:])
    torch.cuda.synchronize()
    _check(buf[:, sl], R.lc_ref(c), c.odt, "local_corr", f"local_corr {c.id}", zero=R.lc_zero_mask(c))
    assert R.untouched(buf, sl), f"{c.id}: columns outside [{sl.start}, {sl.stop}) of the row buffer changed"


# ------------------------------------------------------------------------------------------------------------ grid_sample
@pytest.mark.parametrize("c", R.GS_ALL, ids=lambda c: c.id)
def test_grid_sample(c):
    from gim_amd import ops
    dev = _dev()
    feat, grid = R.gs_inputs(c)
    col0, stride = R.gs_out_layout(c)
    buf, sl = _slice_buffer(c.B * c.ho * c.wo, col0, c.C, stride, c.dt, dev)
    out = buf[:, col0:2 * col0] if c.layout == "slice" else buf         # rows[:, c:2 * c] of refine; the scale-1 shape: a whole row
    ops.grid_sample(_nhwc(feat, c.dt).to(dev), grid.to(dev), out)
    torch.cuda.synchronize()
    _check(buf[:, sl], R.gs_ref(c), c.dt, "grid_sample", f"grid_sample {c.id}", zero=R.gs_zero_mask(c))
    assert R.untouched(buf, sl), f"{c.id}: columns outside [{sl.start}, {sl.stop}) of the row buffer changed"


# ------------------------------------------------------------------------------------------------------------ dkm_disp_emb
@pytest.mark.parametrize("c", R.DE_ALL, ids=lambda c: c.id)
def test_disp_emb(c):
    from gim_amd import ops
    dev = _dev()
    flow, wgt, bias = R.de_inputs(c)
    ew = wgt.to(dev)
    if c.emb_scale:
        ew = ew * c.emb_scale               # as refine does: the scale goes into the weights on the host side of the launch
    buf, sl = _slice_buffer(c.B * c.h * c.w, c.col0, c.E, c.stride, c.odt, dev)
    ops.dkm_disp_emb(flow.to(dev), ew.contiguous(), bias.to(dev), buf[:, c.col0:])
    torch.cuda.synchronize()
    _check(buf[:, sl], R.de_ref(c), c.odt, "disp_emb", f"disp_emb {c.id}")
    assert R.untouched(buf, sl), f"{c.id}: columns outside [{sl.start}, {sl.stop}) of the row buffer changed"


# ------------------------------------------------------------------------------------------------------------ resize_bilinear
@pytest.mark.parametrize("c", R.RS_ALL, ids=lambda c: c.id)
def test_resize_bilinear(c):
    from gim_amd import ops
    dev = _dev()
    x = R.rs_input(c)
    y = ops.resize_bilinear(_nhwc(x, c.dt).to(dev), c.dst, out_dtype=R.TDT[c.odt])
    torch.cuda.synchronize()
    assert y.dtype == R.TDT[c.odt] and y.shape == (c.B, *c.dst, c.C)
    _check(y, R.rs_ref(c), c.odt, "resize", f"resize {c.id}")
    if c.src == c.dst:      # identity: every weight is 0 or 1, the output is the input (rounded once where the output is narrower)
        assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1).to(R.TDT[c.odt])), f"{c.id}: the identity size is not exact"


# ------------------------------------------------------------------------------------------------------------ the composed row
@pytest.mark.parametrize("c", R.ROW_ALL, ids=lambda c: c.id)
def test_refine_row_assembly(c):
    """the c % g == 0 branch of gim_amd.dense.refine at (c, e, r) = (256, 32, 2): the three launches into one zeroed row buffer, the
    whole row against cat[x, grid_sample(y), emb, local_corr], the tail up to the row stride exactly zero"""
    from gim_amd import ops
    dev = _dev()
    ch, e, r = R.REFINER_DKM[c.scale]
    lay = R.refine_layout(R.REFINER_DKM, c.scale, c.dt)
    cs = lay["cs"]
    xc, yc, flow_c, wgt, bias = R.row_inputs(c)
    x, y, flow = _nhwc(xc, c.dt).to(dev), _nhwc(yc, c.dt).to(dev), flow_c.to(dev)
    ew, eb = wgt.to(dev), bias.to(dev)
    b, h, w, _ = x.shape
    D = torch.zeros(b, h, w, cs, dtype=R.TDT[c.dt], device=dev)
    rows = D.view(b * h * w, cs)
    D[..., :ch].copy_(x[..., :ch])
    ops.grid_sample(y, flow, rows[:, ch:2 * ch])
    ops.dkm_disp_emb(flow, ew, eb, rows[:, 2 * ch:])
    ops.local_corr(x, y, flow, r, rows[:, 2 * ch + e:])
    torch.cuda.synchronize()
    ref = R.row_ref(c)
    got = rows.cpu()
    assert torch.equal(got[:, :ch].float(), ref["x"]), "the query features"
    _check(got[:, lay["gs"]:lay["emb"]], ref["gs"], c.dt, "grid_sample", f"row {c.id} grid_sample")
    _check(got[:, lay["emb"]:lay["corr"]], ref["emb"], c.dt, "disp_emb", f"row {c.id} disp_emb")
    _check(got[:, lay["corr"]:lay["width"]], ref["corr"], c.dt, "local_corr", f"row {c.id} local_corr")
    assert lay["width"] < cs and (got[:, lay["width"]:].view(torch.int16) == 0).all(), "the zero tail up to the row stride"
