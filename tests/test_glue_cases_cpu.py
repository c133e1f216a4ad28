"""The cases and float64 restatements of tests/glue_cases.py, checked without a GPU: every restatement agrees, on every case of the
module, with the torch op or oracle function it restates (F.layer_norm, F.max_pool2d, F.interpolate with the matching align_corners,
loftr_oracle.fine_preprocess / fine_matching / position_encoding, a plain permute), the planted fine_match regimes are what they claim,
the LayerNorm plan reaches all four template instances in both 16-bit flavours, and the 16-bit comparison helpers count what they say.
Each test prints the fp32 torch op's own error against the restatement: the figure the GPU bars are built from (glue_cases.bar32).

Measured on the host (largest error of the fp32 op against the float64 restatement, absolute):
    layernorm 3 randn + 0.5: 1.2e-6; 1000 + randn: 4.1e-4; constant rows: 1.2e-7
    upsample2x_add 1.2e-6, resize 3.8e-6, fine_match expec_f 2.7e-6 / mkpts1_f 1.2e-5 (coordinates up to 100)
    fp32 F.layer_norm rounded to 16 bits, elements more than one 16-bit ulp from the rounded float64 value, of 364 588 (R = 203, every
    C): 3 randn + 0.5 rows: bf16 0, fp16 1; 1000 + randn rows: bf16 672, fp16 3950 -- one ulp of a cancelled element is finer than fp32
    arithmetic, so check16's `loose` count (0 in all four) is what an fp32 kernel can be held to there."""
import math

import pytest
import torch
import torch.nn.functional as F

import glue_cases as G
import loftr_oracle as O


def test_layernorm_restatement():
    worst = {}
    for C in G.LN_C:
        for R in G.LN_R + (len(G.LN_CONST),):
            for kind in ("randn", "offset") + (("const",) if R == len(G.LN_CONST) else ()):
                for xdt in G.DTS:
                    for with_res in (True, False):
                        for eps in G.LN_EPS:
                            x, gamma, beta, res = G.ln_inputs(C, R, kind, xdt)
                            ref, err = G.ln_ref(C, R, kind, xdt, with_res, eps)
                            want = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps) + (res.double() if with_res else 0)
                            assert ref.dtype == torch.float64 and G.max_err(ref, want) <= 1e-9 * max(1.0, want.abs().max().item()), (C, R, kind)
                            worst[kind] = max(worst.get(kind, 0.0), err)
                            if kind == "const":      # variance 0: beta (+ res), and the fp32 op agrees to an fp32 rounding of it
                                assert torch.equal(ref, (beta.double() + (res.double() if with_res else 0)).expand(R, C))
    print("[glue case] layernorm: fp32 F.layer_norm vs float64, absolute: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_layernorm_plan_reaches_every_instance():
    """layernorm_kernel<BF16, XBF16>: four instances, the three with a 16-bit side once per 16-bit flavour"""
    seen = {}
    for dt in G.DTS:
        for C in G.LN_C:
            for R, xdt, variant, eps in G.ln_plan(dt, C):
                kinds = {k for k in (dt, xdt) if k != "fp32"} or {"fp32"}
                seen.setdefault(G.ln_instance(dt, xdt, variant), set()).update(kinds)
    assert seen == {(False, False): {"fp32", "bf16", "fp16"}, (True, False): {"bf16", "fp16"}, (False, True): {"bf16", "fp16"},
                    (True, True): {"bf16", "fp16"}}, seen
    assert 260 in G.LN_C and 512 in G.LN_C and all(c % 4 == 0 and c <= 512 for c in G.LN_C)
    assert all(c % 4 or c > 512 for c in G.LN_REFUSED_C)
    assert {r % 4 for r in G.LN_R} == {0, 1, 3} and 1 in G.LN_R


def test_layernorm_fp32_op_in_16_bits():
    """how far one ulp of a 16-bit output is from what fp32 arithmetic delivers: F.layer_norm in fp32, rounded to the kind, against the
    rounded float64 value, element by element"""
    for dt in ("bf16", "fp16"):
        for kind in ("randn", "offset"):
            strict = loose = n = 0
            for C in G.LN_C:
                x, gamma, beta, res = G.ln_inputs(C, 203, kind, dt)
                ref, err = G.ln_ref(C, 203, kind, dt, True, 1e-5)
                s, l = G.check16(G.fp32_layernorm(x, gamma, beta, res, 1e-5).to(G.TDT[dt]), ref, dt, G.bar32(err, ref.abs().max().item()))
                strict, loose, n = strict + s, loose + l, n + ref.numel()
            print(f"[glue case] fp32 F.layer_norm rounded to {dt}, {kind}: {strict} of {n} elements beyond one ulp, {loose} beyond the loose rule")
            assert loose == 0


def test_check16_counts():
    ref = torch.tensor([1.0, -1.0, 0.0, 2.0 ** -12, 64.0], dtype=torch.float64)      # powers of two: x (1 + k eps) is k ulps up
    for dt in ("bf16", "fp16"):
        tdt = G.TDT[dt]
        exact = ref.to(tdt)
        assert G.check16(exact, ref, dt) == (0, 0)
        up = torch.nextafter(exact.float(), torch.full((5,), math.inf)).to(tdt)          # fp32 neighbour rounds back: same value
        assert G.check16(up, ref, dt) == (0, 0)
        eps = torch.finfo(tdt).eps
        one = (exact.float() * (1 + eps)).to(tdt)                                        # one ulp up (0 stays)
        assert G.ulps16(one, exact).tolist() == [1, 1, 0, 1, 1] and G.check16(one, ref, dt) == (0, 0)
        two = (exact.float() * (1 + 2 * eps)).to(tdt)
        assert G.ulps16(two, exact).tolist() == [2, 2, 0, 2, 2] and G.check16(two, ref, dt) == (4, 4)
        assert G.check16(two, ref, dt, bar=4.0 * eps * 2.0 ** -12) == (4, 3)                # the bar reaches two ulps at 2^-12 only
        bad = exact.clone()
        bad[2] = G.NAN
        assert G.check16(bad, ref, dt) == (1, 1)
        neg = torch.tensor([-0.0], dtype=tdt)
        assert G.ulps16(neg, torch.zeros(1, dtype=tdt)).item() == 0
        tiny = torch.tensor([torch.finfo(tdt).tiny], dtype=tdt)
        assert G.ulps16(tiny, -tiny).item() == 2 * G.ordered(tiny).item()
    assert G.bar32(0.0, 8.0) == 2.0 ** -20 and G.bar32(1e-6, 0.0) == 4e-6


def test_layout_restatements():
    for C in G.TO_NCHW_C:
        for ld in G.to_nchw_lds(C):
            assert ld >= C and ld % 8 == 0
            for (H, W) in G.TO_NCHW_HW:
                rows = G.nhwc_rows(G.TO_NCHW_B, H, W, ld, "bf16", 1)
                assert torch.equal(G.ref_nhwc_to_nchw(rows, C), rows[..., :C].permute(0, 3, 1, 2).double())
    assert sorted(h * w for h, w in G.TO_NCHW_HW) == [1, 63, 64, 65, 130]
    n = 0
    for C, cpad, ld, b_off, (H, W) in G.to_nhwc_cases():
        src = G.nchw_image(G.TO_NHWC_B, C, H, W, 2)
        want = torch.zeros(G.TO_NHWC_B, H, W, cpad, dtype=torch.float64)
        want[..., :C] = src.permute(0, 2, 3, 1).double()
        assert torch.equal(G.ref_nchw_to_nhwc(src, cpad), want) and cpad >= C and ld >= cpad and b_off + G.TO_NHWC_B <= G.TO_NHWC_IMAGES
        n += 1
    assert n == 5 * 2 * 2 * 3 and sorted(h * w for h, w in G.TO_NHWC_HW) == [1, 255, 257]


def test_upsample_restatement():
    worst = 0.0
    for dt in G.DTS:
        for (h, w) in G.UPS_HW:
            for C, cs in G.ups_channels(dt):
                lo, hi, ref, err = G.ups_case(h, w, C, dt)
                want = hi.double() + F.interpolate(lo.double(), scale_factor=2, mode="bilinear", align_corners=True)
                assert ref.shape == (G.UPS_B, C, 2 * h, 2 * w) and G.max_err(ref, want) <= 1e-12, (h, w, C)
                assert cs % G.group(dt) == 0 and cs >= C
                worst = max(worst, err)
    print(f"[glue case] upsample2x_add: fp32 hi + F.interpolate vs float64, absolute: {worst:.2e}")


def test_resize_restatement():
    worst = 0.0
    for dt in G.DTS:
        for (src, size) in G.RESIZE_SHAPES:
            for C in (G.RESIZE_C,) + G.RESIZE_IMAGE_C:
                x, ref, err = G.resize_case(src, size, C, dt)
                want = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False)
                assert G.max_err(ref, want) <= 1e-12, (src, size, C)
                if src == size:
                    assert torch.equal(ref, x.double())
                worst = max(worst, err)
    print(f"[glue case] resize: fp32 F.interpolate vs float64, absolute: {worst:.2e}")
    assert {a for a, _ in G.RESIZE_PAIRS} == set(G.DTS) and all(a == b or "fp32" in (a, b) for a, b in G.RESIZE_PAIRS) and len(set(G.RESIZE_PAIRS)) == 7


def test_posenc_restatement():
    for C in G.POSENC_C:
        for hw, (h, w) in G.POSENC_HW.items():
            assert h * w == hw
            pe = G.ref_position_encoding(C, h, w)
            assert G.max_err(O.position_encoding(C, h, w)[0], pe) <= 1e-6
            for nb in G.POSENC_NB:
                for dt in G.DTS:
                    x, tab, ref = G.posenc_case(hw, nb, C, dt)
                    assert tab.is_contiguous() and x.is_contiguous() and tab.dtype == torch.float32     # handed over as bare pointers
                    feat = x.view(nb, h, w, C).permute(0, 3, 1, 2)
                    want = (feat.double() + tab.double().view(h, w, C).permute(2, 0, 1)[None]).flatten(2).transpose(1, 2).reshape(nb * hw, C)
                    assert torch.equal(ref, want)
    assert math.gcd(7, 256) == 1 and 48 % 16 == 0


def test_fine_gather_restatement():
    (h0, w0), (h1, w1) = G.FG_COARSE
    assert (h0, w0) != (h1, w1) and h0 != h1 and w0 != w1
    b, i, j = G.fg_ids(37)
    assert i[:4].tolist() == G.corners(h0, w0) and j[4:8].tolist() == G.corners(h1, w1) and set(b.tolist()) == {0, 1}
    assert (b.diff() >= 0).all() and i.max() < h0 * w0 and j.max() < h1 * w1 and j.max() >= w1 * (h1 - 1)
    seen = set()
    for W, stride, C, ldf, M, outs in G.fg_cases():
        seen.add((W, stride, C, ldf - C, M))
        f0, f1 = G.fg_maps(stride, C, "fp32")
        b, i, j = G.fg_ids(M)
        u0, u1 = G.ref_fine_gather(f0, f1, b, i, j, w0, w1, stride, W)
        want0 = O.fine_preprocess(f0, f0, b, i, i, (h0, w0), f0.shape[2:], W)[0]
        want1 = O.fine_preprocess(f1, f1, b, j, j, (h1, w1), f1.shape[2:], W)[0]
        assert torch.equal(u0, want0) and torch.equal(u1, want1), (W, stride, C, M)
        if M == 37 and W > 1:
            assert (u0[:4] == 0).any() and (u1[4:8] == 0).any()
        if M == 37 and W == 7 and stride == 2:
            assert (u0[8] == 0).any() and (u1[8] == 0).any()           # an interior-adjacent cell crosses the border too
    assert len(seen) == 4 * 2 * 2 * 2 * 2


@pytest.mark.parametrize("W", G.FM_W)
def test_fine_match_restatement(W):
    worst_e = worst_m = 0.0
    WW = W * W
    for C in G.FM_C:
        for M in G.FM_M:
            for regime in G.FM_REGIMES:
                f0, f1, mk, b, s1 = G.fm_inputs(W, C, M, regime)
                sim = torch.einsum("mc,mrc->mr", f0[:, WW // 2].double(), f1.double()) / math.sqrt(C)
                for has in (False, True):
                    e64, m64, ee, em = G.fm_ref(W, C, M, regime, has)
                    scale = max(1.0, m64.abs().max().item())
                    assert ee <= 2e-5 and em <= 2e-5 * scale, (W, C, M, regime, ee, em)        # the oracle in fp32 is that close
                    worst_e, worst_m = max(worst_e, ee), max(worst_m, em)
                if regime == "flat":
                    assert (sim == 0).all() and e64[:, :2].abs().max() <= 1e-15 and G.max_err(e64[:, 2], torch.full((M,), G.flat_std(W), dtype=torch.float64)) <= 1e-14
                if regime.startswith("sat"):
                    r = G.fm_sat_cell(regime, W)
                    others = torch.cat([sim[:, :r], sim[:, r + 1:]], 1)
                    assert (sim[:, r, None] - others).min() > 110
                    lin = [-1.0 + 2.0 * k / (W - 1) for k in range(W)]
                    assert G.max_err(e64[:, 0], torch.full((M,), lin[r % W], dtype=torch.float64)) <= 1e-15
                    assert G.max_err(e64[:, 1], torch.full((M,), lin[r // W], dtype=torch.float64)) <= 1e-15
                    assert G.max_err(e64[:, 2], torch.full((M,), 2e-5, dtype=torch.float64)) <= 1e-12
                if regime == "offset":
                    base = torch.einsum("mc,mrc->mr", f0[:, WW // 2].double(), G.fm_inputs(W, C, M, "random")[1].double()) / math.sqrt(C)
                    assert G.max_err(sim - base, torch.full_like(sim, 80.0)) <= 1e-3 and sim.min() > 70
                    e_rnd = G.fm_ref(W, C, M, "random", False)[0]
                    assert G.max_err(e64, e_rnd) <= 2e-3                # the offset cancels in the softmax (f1 + t q is rounded to fp32)
    assert abs(G.SAT_STD - 2e-5) < 1e-11 and G.grid_coord_fp32(5, 3) == {0.5} and G.grid_coord_fp32(7, 6) == {1.0}
    assert all(math.isqrt(ww) ** 2 != ww or ww > 64 for ww in G.FM_REFUSED_WW)
    print(f"[glue case] fine_match W={W}: fp32 oracle vs float64, absolute: expec_f {worst_e:.2e}, mkpts1_f {worst_m:.2e}")


def test_maxpool_restatement():
    for dt in G.DTS:
        for C in G.pool_channels(dt):
            for negative in (False, True):
                for (H, W) in G.POOL2_HW:
                    x = G.pool_input(H, W, C, dt, negative)
                    assert torch.equal(G.ref_maxpool(x, 2, 2, 0), F.max_pool2d(x.double(), 2, 2))
                for (H, W) in G.POOL3_HW:
                    x = G.pool_input(H, W, C, dt, negative)
                    ref = G.ref_maxpool(x, 3, 2, 1)
                    assert torch.equal(ref, F.max_pool2d(x.double(), 3, 2, 1)) and ref.shape[2:] == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
                    assert not negative or (ref < 0).all()
