"""The cases, references and bounds of tests/refiner_input_cases.py, checked without a GPU: the flow / grid tables contain the edge
classes they are built for (counted with the reference's own arithmetic), the reference is exactly zero wherever every tap is outside
the map and equals the feature at the pixel centres, the slice columns and row strides of the cases are the ones gim_amd.dense.refine
computes from the engines' REFINER tables, the cases reach the local_corr instantiations the models run, every reference is finite and
covers every output element, and the 16-bit bound admits one rounding to nearest and refuses a truncating store."""
import pytest
import torch

import refiner_input_cases as R

SIDES = ("left", "right", "top", "bottom")


# ------------------------------------------------------------------------------------------------------------ edge classes
@pytest.mark.parametrize("c", [c for c in R.LC_EDGES if c.dt == "fp32"], ids=lambda c: c.id)
def test_local_corr_flow_table_contains_its_classes(c):
    names, flow = R.lc_flow_table(c.r, c.h, c.w)
    assert flow.shape == (len(names), c.h, c.w, 2) and len(set(names)) == len(names) == c.B == R.N_LC_TABLE
    cl = R.tap_classes(flow, c.r, c.h, c.w)
    print(f"[refiner case] {c.id}: queries per class {cl}")
    for k in SIDES + ("outside",):
        assert cl[k] >= 1, (k, cl)
    # a window with room for its fractional corner fits the 6 x 5 map at r = 1 only (2r + 2 <= 5); at 2r + 1 = 5 it fits at fraction
    # zero alone, which the last bit of the coordinate decides
    assert (cl["inside"] >= 1) if 2 * c.r + 2 <= min(c.h, c.w) else (cl["inside"] == 0 or 2 * c.r + 1 == min(c.h, c.w)), cl
    per = {n: R.tap_classes(flow[i:i + 1], c.r, c.h, c.w) for i, n in enumerate(names)}
    # the grid itself and the half-pixel shift: fractions 0 and 0.5 (fp64 geometry)
    ix, iy = R._tap_px(flow[:2], c.r, c.h, c.w, torch.float64)
    assert ((ix[0] - ix[0].round()).abs().max() < 1e-6) and ((ix[1] - ix[1].floor() - 0.5).abs().max() < 1e-6)
    assert ((iy[0] - iy[0].round()).abs().max() < 1e-6) and ((iy[1] - iy[1].floor() - 0.5).abs().max() < 1e-6)
    n = c.h * c.w
    for side in SIDES:                                       # partly outside on its own side, for every query of the image
        assert per[side][side] == n and per[side]["outside"] == 0, (side, per[side])
    for a, b in (("top", "left"), ("top", "right"), ("bottom", "left"), ("bottom", "right")):
        p = per[f"{a}-{b}"]
        assert p[a] == n and p[b] == n and p["outside"] == 0, (a, b, p)
    for nm in ("out-left", "out-right", "out-top", "out-bottom", "x+1e+09", "x-1e+09", "y+1e+09", "y-1e+09", "xy+1e9", "x-1e9,y+1e9"):
        assert per[nm]["outside"] == n, (nm, per[nm])
    for nm in ("x+3", "x-3", "y+3", "y-3"):                  # +-3.0: 9.5 / 11.5 pixels from the map's first pixel: beyond r <= 3 windows
        assert per[nm]["outside"] == (n if c.r <= 3 else 0), (nm, per[nm])
    # "by one pixel": the nearest tap of the out-* entries is one pixel beyond the zero boundary
    k = names.index("out-left")
    ix, _ = R._tap_px(flow[k:k + 1], c.r, c.h, c.w, torch.float64)
    assert abs(ix.max().item() + 2.0) < 1e-6
    k = names.index("out-right")
    ix, _ = R._tap_px(flow[k:k + 1], c.r, c.h, c.w, torch.float64)
    assert abs(ix.min().item() - (c.w + 1.0)) < 1e-6


@pytest.mark.parametrize("c", [c for c in R.LC_SMALL if c.dt == "fp32"], ids=lambda c: c.id)
def test_local_corr_small_maps_are_smaller_than_the_window(c):
    assert 2 * c.r + 1 > max(c.h, c.w)
    cl = R.tap_classes(R.lc_inputs(c)[2], c.r, c.h, c.w)
    assert all(cl[k] == c.B * c.h * c.w for k in SIDES) and cl["inside"] == 0 and cl["outside"] == 0, cl
    ref = R.lc_ref(c)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0 and (ref[R.lc_zero_mask(c)] == 0).all() and R.lc_zero_mask(c).any()


@pytest.mark.parametrize("hw", [(5, 7), (1, 7), (7, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_table_contains_its_classes(hw):
    h, w = hw
    names, tab = R.gs_grid_table(h, w)
    assert len(set(names)) == len(names) and len(names) <= 35
    per = {n: R.tap_classes(tab[i].reshape(1, 1, 1, 2), 0, h, w) for i, n in enumerate(names)}
    cl = R.tap_classes(tab.reshape(1, 1, -1, 2), 0, h, w)
    print(f"[refiner case] grid table {h}x{w}: entries per class {cl}")
    assert all(cl[k] >= 1 for k in SIDES + ("inside", "outside")), cl
    for side in SIDES:
        assert per[f"{side}-in"][side] == 1 and per[f"{side}-in"]["outside"] == 0 and per[f"{side}-out"]["outside"] == 1, side
    for nm in names:
        if nm[0] in "xy" and nm[1] in "+-" and "=" not in nm:      # +-3, +-1e6, +-1e9, +-1e12
            assert per[nm]["outside"] == 1, nm
    # exactly +-1: the sample point is the map's edge, half a pixel beyond the last pixel centre: half weight
    # (of what the other axis leaves: on a one-pixel axis the interior target is itself partly outside)
    feat = torch.ones(1, 1, h, w)
    gs = lambda g: torch.nn.functional.grid_sample(feat, g.reshape(1, 1, 1, 2), align_corners=False).item()   # noqa: E731
    centre = tab[names.index("centre")]
    for nm in ("x=+1", "x=-1", "y=+1", "y=-1"):
        g = tab[names.index(nm)]
        other = centre.clone()
        other[1 if nm[0] == "x" else 0] = g[1 if nm[0] == "x" else 0]
        assert gs(other) > 0.5 and abs(gs(g) - 0.5 * gs(other)) < 1e-6, (nm, gs(g), gs(other))
    assert per["centre"]["inside"] == 1


def test_every_image_of_a_grid_case_meets_every_table_entry():
    for c in R.GS_ALL:
        gr = R.gs_inputs(c)[1]
        assert gr.shape == (c.B, c.ho, c.wo, 2) and c.B == 3
        if c.kind == "table":
            tab = R.gs_grid_table(c.h, c.w)[1]
            for b in range(c.B):
                rows = gr[b].reshape(-1, 2)
                assert all((rows == t).all(1).any() for t in tab), (c.id, b)
            assert not torch.equal(gr[0], gr[1])
        feat = R.gs_inputs(c)[0]
        assert not torch.equal(feat[0], feat[1]) and not torch.equal(feat[1], feat[2])      # the batch index shows
    assert {(c.ho, c.wo) == (c.h, c.w) for c in R.GS_ALL} == {True, False}
    assert {c.C for c in R.GS_ALL} == {4, 8, 64, 512} and {c.dt for c in R.GS_ALL if c.C == 4} == {"fp32"}
    assert {(c.h, c.w) for c in R.GS_THIN} == {(1, 7), (7, 1)}


# ------------------------------------------------------------------------------------------------------------ the references
def test_reference_is_exactly_zero_where_every_tap_is_outside():
    n_edge = 0
    for c in R.LC_ALL:
        ref, z = R.lc_ref(c), R.lc_zero_mask(c)
        assert z.shape == ref.shape and (ref[z] == 0).all(), c.id
        n_edge += int(((ref == 0) & ~z).sum())
        if c.flow == "table":
            assert z.all(1).sum() >= 10 * c.h * c.w, c.id          # the out-* and +-1e9 images: whole rows
    print(f"[refiner case] local_corr: {n_edge} reference zeros lie on the zero boundary itself (held to the bound, not to exact zero)")
    for c in R.GS_ALL:
        ref, z = R.gs_ref(c), R.gs_zero_mask(c)
        assert z.shape == (ref.shape[0], 1) and (ref[z[:, 0]] == 0).all(), c.id
        assert torch.equal((ref == 0).all(1), z[:, 0]), c.id           # grid_sample's tables keep clear of the boundary: the two agree
        if c.kind == "table":
            assert z.sum() >= 20 * c.B, c.id


def test_reference_equals_the_feature_at_pixel_centres():
    worst = 0.0
    for c in R.GS_ALL:
        if c.kind != "centres":
            continue
        feat = R.gs_inputs(c)[0].permute(0, 2, 3, 1).reshape(-1, c.C)
        d = (R.gs_ref(c) - feat).abs().max().item() / feat.abs().max().item()
        worst = max(worst, d)
        assert d <= 1e-6, (c.id, d)
    # local_corr on the grid itself: the centre tap is <f0, f1> / sqrt(C) at the query's own pixel
    for c in R.LC_EDGES:
        f0, f1, _ = R.lc_inputs(c)
        K = (2 * c.r + 1) ** 2
        ref = R.lc_ref(c)[:c.h * c.w, K // 2]
        want = ((f0[0].double() * f1[0].double()).sum(0) / c.C ** 0.5).reshape(-1)
        d = (ref.double() - want).abs().max().item() / R.lc_ref(c).abs().max().item()
        worst = max(worst, d)
        assert d <= 1e-6, (c.id, d)
    print(f"[refiner case] pixel centres: reference vs feature, worst {worst:.2e} of scale")


def test_every_reference_is_finite_and_covers_every_output_element():
    for c in R.LC_ALL:
        f0, f1, flow = R.lc_inputs(c)
        B = flow.shape[0]
        assert B == c.B and f0.shape == f1.shape == (B, c.C, c.h, c.w)
        assert R.lc_ref(c).shape == (B * c.h * c.w, (2 * c.r + 1) ** 2) and torch.isfinite(R.lc_ref(c)).all(), c.id
        assert torch.equal(f0, R.rounded(f0, c.dt)) and torch.equal(f1, R.rounded(f1, c.dt))
        assert R.bound(R.lc_ref(c), c.odt, "local_corr").numel() == R.lc_ref(c).numel()
    for c in R.GS_ALL:
        assert R.gs_ref(c).shape == (c.B * c.ho * c.wo, c.C) and torch.isfinite(R.gs_ref(c)).all(), c.id
        assert torch.equal(R.gs_inputs(c)[0], R.rounded(R.gs_inputs(c)[0], c.dt))
    for c in R.DE_ALL:
        assert R.de_ref(c).shape == (c.B * c.h * c.w, c.E) and torch.isfinite(R.de_ref(c)).all() and R.de_ref(c).abs().max() > 0.1, c.id
    for c in R.RS_ALL:
        assert R.rs_ref(c).shape == (c.B, *c.dst, c.C) and torch.isfinite(R.rs_ref(c)).all(), c.id
        if c.src == c.dst:
            assert torch.equal(R.rs_ref(c), R.rs_input(c).permute(0, 2, 3, 1)), c.id      # identity: exact in the reference too
    for c in R.ROW_ALL:
        lay = R.refine_layout(R.REFINER_DKM, c.scale, c.dt)
        ref = R.row_ref(c)
        assert sum(v.shape[1] for v in ref.values()) == lay["width"] and all(torch.isfinite(v).all() for v in ref.values())
        assert all(v.shape[0] == c.B * c.h * c.w for v in ref.values())


def test_case_tables_hold_what_the_issue_lists():
    assert {(c.C, c.r, c.dt, c.odt) for c in R.LC_PRODUCTION} == (
        {(C, r, dt, dt) for (C, r) in ((512, 7), (512, 3), (256, 2)) for dt in R.DTS} | {(256, 2, "bf16", "fp32"), (256, 2, "fp16", "fp32")})
    assert all((c.B * c.h * c.w) % 4 != 0 for c in R.LC_PRODUCTION + R.LC_CHANNELS + R.LC_PADDED)       # the ragged last workgroup runs
    assert {(c.C, c.dt) for c in R.LC_CHANNELS} >= {(320, "fp32"), (1024, "bf16"), (1024, "fp16"), (8, "fp32"), (8, "bf16"), (8, "fp16")}
    assert all(c.pad == 8 for c in R.LC_PADDED) and {c.dt for c in R.LC_PADDED} == set(R.DTS)
    assert {(c.r, c.dt) for c in R.LC_EDGES} == {(r, dt) for r in (1, 2, 3, 7) for dt in R.DTS} and all((c.C, c.h, c.w) == (64, 6, 5) for c in R.LC_EDGES)
    assert {(c.r, c.h, c.w) for c in R.LC_SMALL} == {(7, 3, 2), (1, 1, 1)}
    assert {(c.E, c.odt, c.h, c.w) for c in R.DE_ALL if not c.emb_scale} == {(E, o, h, w) for E in (6, 16, 128) for o in R.DTS for (h, w) in R.DE_MAPS}
    assert all(c.col0 > 0 and c.stride >= c.col0 + c.E for c in R.DE_ALL) and any(c.emb_scale for c in R.DE_ALL)
    assert {(c.dt, c.odt) for c in R.RS_ALL if c.C == 8} == {(a, b) for a in R.DTS for b in R.DTS if "fp32" in (a, b) or a == b}
    assert {c.C for c in R.RS_ALL if (c.dt, c.odt) == ("fp32", "fp32")} == {1, 2, 8}
    assert {(c.src, c.dst) for c in R.RS_ALL} == {((7, 9), (14, 18)), ((2, 3), (32, 48)), ((6, 5), (6, 5)), ((13, 17), (5, 6)), ((1, 5), (3, 9))}
    for group in (R.LC_ALL, R.GS_ALL, R.DE_ALL, R.RS_ALL, R.ROW_ALL):
        assert len({c.id for c in group}) == len(group)


# ------------------------------------------------------------------------------------------------------------ layout and dispatch
def test_slices_and_strides_are_the_production_layout():
    """against gim_amd.dense.refine's own arithmetic: cs = P[cr{s}.cin_store] = cstore(refiner_dims(...)[0], dt), slices at c, 2c, 2c + e"""
    from gim_amd import _lib
    from gim_amd.dense import refiner_dims
    from gim_amd.packing import PRECISION_DTYPE, cstore
    from gim_amd.roma.roma import REFINER as ROMA
    assert R.REFINER_ROMA == ROMA
    for dt in R.DTS:
        gdt = PRECISION_DTYPE[dt]
        assert all(R.cstore(n, dt) == cstore(n, gdt) for n in range(1, 1400))
        for table in (R.REFINER_DKM, ROMA):
            for s in table:
                c, e, r = table[s]
                lay = R.refine_layout(table, s, dt)
                assert lay["cs"] == cstore(refiner_dims(table, s)[0], gdt) and lay["width"] == refiner_dims(table, s)[0]
                assert (lay["gs"], lay["emb"], lay["corr"]) == (c, 2 * c, 2 * c + e)
    assert _lib.GIM_F32 == PRECISION_DTYPE["fp32"]
    for c in R.LC_PRODUCTION:
        scale = {(512, 7): "16", (512, 3): "8", (256, 2): "4"}[(c.C, c.r)]
        for table in (R.REFINER_DKM, ROMA):
            lay = R.refine_layout(table, scale, c.odt)
            assert (c.col0, c.stride) == (lay["corr"], lay["cs"]), c.id
    assert {c.col0 for c in R.LC_PRODUCTION} == {1152, 1088, 544}
    for c in R.LC_ALL:
        assert c.stride >= c.col0 + (2 * c.r + 1) ** 2 and c.col0 > 0, c.id
    for c in R.DE_ALL:
        if c.E in (128, 16):
            scale = {128: "16", 16: "2"}[c.E]
            lay = R.refine_layout(R.REFINER_DKM, scale, c.odt)
            assert (c.col0, c.stride) == (lay["emb"], lay["cs"]), c.id
    for c in R.GS_ALL:
        assert R.gs_out_layout(c) == ((c.C, 3 * c.C) if c.layout == "slice" else (0, c.C))
    for c in R.ROW_ALL:
        assert R.REFINER_DKM[c.scale] == (256, 32, 2) and R.refine_layout(R.REFINER_DKM, c.scale, c.dt)["cs"] == 576


def test_cases_reach_the_local_corr_instantiations_the_models_run():
    seen = {}
    for c in R.LC_ALL:
        ld = c.C + c.pad
        seen.setdefault(R.lc_instance(c.C, c.r, c.dt, c.odt, ld, ld), set()).add(c.dt if c.dt != "fp32" else c.odt)
    # <16-bit in, 16-bit out, V8, PT>: scales 16, 8 and 4 of both engines, each in the bf16 and the fp16 flavour of the library
    for inst in ((True, True, True, 16), (True, True, True, 8), (True, True, False, 6)):
        assert seen.get(inst, set()) >= {"bf16", "fp16"}, (inst, seen.get(inst))
    for pt in (6, 8, 16):
        assert (False, False, False, pt) in seen and (True, True, False, pt) in seen
    assert seen.get((True, False, False, 16), set()) >= {"bf16", "fp16"}
    nch = lambda c: (c.C + 64 * (8 if R.lc_instance(c.C, c.r, c.dt, c.odt, c.C, c.C)[2] else 4) - 1) // (64 * (8 if R.lc_instance(c.C, c.r, c.dt, c.odt, c.C, c.C)[2] else 4))   # noqa: E731
    assert {nch(c) for c in R.LC_CHANNELS if c.C == 320} == {2} and 320 % 256 != 0
    assert {nch(c) for c in R.LC_CHANNELS if c.C == 1024} == {2} and all(R.lc_instance(c.C, c.r, c.dt, c.odt, c.C, c.C)[2] for c in R.LC_CHANNELS if c.C == 1024)


# ------------------------------------------------------------------------------------------------------------ the bound and the helpers
@pytest.mark.parametrize("odt", ["bf16", "fp16"])
def test_bound_admits_one_rounding_and_refuses_truncation(odt):
    g = torch.Generator().manual_seed(9)
    x = (0.5 + torch.rand(4096, generator=g)) * torch.logspace(-2, 1, 4096) * (1 - 2 * torch.randint(0, 2, (4096,), generator=g))   # normal range of both formats
    once = x.to(R.TDT[odt])
    assert R.worst_ratio(once, x, odt, "grid_sample") <= 1.0
    bits = 16 if odt == "bf16" else 13
    trunc = (x.view(torch.int32) >> bits << bits).view(torch.float32)          # chop instead of round
    assert torch.equal(trunc.to(R.TDT[odt]).float(), trunc)
    assert R.worst_ratio(trunc, x, odt, "grid_sample") > 1.5
    twice = x.to(torch.float16).to(torch.bfloat16) if odt == "bf16" else None     # fp32 -> fp16 -> bf16: double rounding
    if twice is not None:
        assert R.worst_ratio(twice, x, odt, "grid_sample") > 1.0
    assert R.worst_ratio(torch.full((4,), float("nan")), torch.zeros(4), odt, "resize") == float("inf")
    assert R.worst_ratio(torch.zeros(4), torch.zeros(4), "fp32", "resize") == 0.0
    assert R.worst_ratio(torch.tensor([0.0, 1e-30]), torch.zeros(2), "bf16", "resize") > 1.0      # a zero reference admits only zero


def test_row_buffer_helpers():
    for dt in R.DTS:
        buf = R.row_buffer(5, 24, dt)
        sl = slice(8, 14)
        buf[:, sl] = 1.0
        assert R.untouched(buf, sl)
        bad = buf.clone()
        bad[3, 14] = 7.0001 if dt == "fp32" else 7.0625
        assert not R.untouched(bad, sl)
        bad = buf.clone()
        bad[0, 7] = float("nan")
        assert not R.untouched(bad, sl)
    x = torch.randn(1, 2, 3, 8)
    buf, C = R.nan_padded(x, "bf16")
    assert C == 8 and buf.shape == (1, 2, 3, 16) and torch.isnan(buf[..., 8:]).all() and torch.equal(buf[..., :8], x.bfloat16())
    v = buf[..., :C]
    assert v.shape[3] == 8 and v.stride(2) == 16 and v.data_ptr() == buf.data_ptr()
