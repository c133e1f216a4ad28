"""The cases and references of tests/linear_attention_cases.py, checked without a GPU: the float64 reference is the oracle's
LinearAttention, every case takes the route (and has the chunk count) it is built for, the masks mask what they claim, every template
instance the dispatch of csrc/linear_attention.hip names is reached by a case, and a plain fp32 torch evaluation of the formula stays
below half of each case's GPU bar -- the reference-side margin of the bounds in tests/test_gpu_linear_attention_edges.py.

Measured on the host (deviation of the fp32 torch evaluation from ref_attention, of max|ref|, largest over the cases of a group;
fp32 inputs / the same operands rounded to 16 bits):
    routing 3.7e-7 / 4.4e-7, plain 4.9e-7 / 4.9e-7, misaligned - / 4.1e-7, dtype pairs 5.3e-7 / 3.8e-7, strided 3.8e-7 / 4.3e-7,
    masked 5.1e-7 / 4.7e-7: a twentieth of the tightest bar (1e-5, fp32 outputs)
    long-S states (fp32 torch state against ref_state): S = 8193: KV 3.8e-7, Ksum 1.8e-7; S = 4097: KV 4.5e-7, Ksum 1.8e-7
    -> LONG_S_FP32_DEV = 1e-6 for both (rounded up), 4 x that = 4e-6 < 1e-5: the bar of the two long-S cases is BAR_STATE itself."""
import pytest
import torch

import linear_attention_cases as C
import loftr_oracle as O


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape", [(3, 70, 257, 8, 32), (4, 25, 33, 8, 16), (2, 130, 129, 4, 32)], ids=lambda s: "x".join(map(str, s)))
def test_ref_attention_is_the_oracle(shape, masked):
    """on raw fp32 inputs (the oracle maps them through elu + 1 itself), within 1e-5 of scale: the bound of test_linear_attention's
    fp32 sanity line"""
    nb, L, S, H, D = shape
    q, k, v = C.raw_operands(nb, L, S, H, D, 77)
    qm, km = C.build_masks("random", nb, L, S, 77) if masked else (None, None)
    want = O.linear_attention(q, k, v, qm, km)
    got = C.ref_attention(torch.nn.functional.elu(q) + 1, torch.nn.functional.elu(k) + 1, v, qm, km)
    assert got.dtype == torch.float64 and C.rel_err(got, want) <= 1e-5, C.rel_err(got, want)


def test_cases_take_the_route_they_claim():
    for c in C.ROUTING:
        assert c.route == ("short" if c.L <= 64 and c.S <= 64 else "mfma" if c.D == 32 else "plain"), c.id
    assert {c.route for c in C.ROUTING} == {"short", "mfma", "plain"}
    assert all(c.route == "plain" for c in C.PLAIN + C.MISALIGNED)
    assert all(C.route(c.nb, c.L, c.S, c.H, c.D, c.dt, c.layout)[1:] == ("la_kv_kernel", "la_apply_mfma_kernel") for c in C.MISALIGNED)
    assert {C.nchunk(c.S, "la_kv_kernel") for c in C.PLAIN} == {1, 2, 3} and {c.S for c in C.PLAIN} == {65, 128, 129, 257}
    assert {(c.H, c.D) for c in C.PLAIN} == {(4, 32), (1, 32), (2, 16), (12, 16), (8, 16), (15, 32)}
    assert {(c.L, c.D) for c in C.PLAIN} == {(65, 16), (130, 16), (65, 32), (130, 32)}
    assert max(c.H * (c.D * c.D + c.D) * 4 for c in C.PLAIN) == 63360 and 16 * (32 * 32 + 32) * 4 > 64 * 1024
    for group in (C.DTYPE_PAIRS, C.STRIDED, C.MASKED):
        assert {c.route for c in group} == {"short", "mfma", "plain"}
    for c in C.ALL:
        assert c.route == C.route(c.nb, c.L, c.S, c.H, c.D, c.dt, c.layout)[0], c.id
        assert (c.H * c.D) % 4 == 0


def test_every_dispatched_instance_is_reached():
    """la_short_kernel<D, A, B>, la_apply_kernel<D, A, B>: D in {16, 32} x four dtype pairs; la_apply_mfma_kernel<A, B>: four pairs;
    la_kv_kernel<D, A>: four -- A / B = 16-bit input / output, each in the bf16 and the fp16 flavour of the library"""
    seen = {}
    for c in C.ALL:
        for inst in C.instances(c):
            kinds = {x for x in (c.dt, c.odt) if x != "fp32"} or {"bf16", "fp16"}     # an all-fp32 instance exists once
            seen.setdefault(inst, set()).update(kinds)
    want = [(n, D, a, b) for n in ("la_short_kernel", "la_apply_kernel") for D in (16, 32) for a in (False, True) for b in (False, True)]
    want += [("la_apply_mfma_kernel", 32, a, b) for a in (False, True) for b in (False, True)]
    want += [("la_kv_kernel", D, a) for D in (16, 32) for a in (False, True)]
    for inst in want:
        assert seen.get(inst) == {"bf16", "fp16"}, (inst, seen.get(inst))


def test_masks_mask_what_they_claim():
    for c in C.MASKED + tuple(c for c in C.MISALIGNED if c.mask):
        _, _, _, qm, km = C.case_inputs(c)
        assert qm.shape == (c.nb, c.L) and km.shape == (c.nb, c.S) and qm.dtype == km.dtype == torch.bool
        if c.mask == "seqzero":       # designed otherwise: whole sequences masked / valid
            assert not qm[0].any() and not km[1].any() and km[0].all() and km[2:].all() and qm[c.nb - 1].all()
            continue
        for m in (qm, km):
            assert m.any(1).all() and (~m).any(1).all(), c.id          # one valid and one masked row per sequence
        if c.mask == "chunk":
            assert not km[:, 256:512].any() and km[:, :256].all() and km[:, 512:].all() and km[:, 512:].shape[1] >= 1
            assert not qm[:, 64:128].any() and qm[:, :64].all() and qm[:, 128:].all()
        if c.mask in ("prefix", "prefix256", "prefix512"):
            for m in (qm, km):
                assert (m.int().diff(dim=1) <= 0).all(), c.id                 # a prefix: never back to valid
        if c.mask in ("prefix256", "prefix512"):
            assert (km.sum(1) == (256 if c.mask == "prefix256" else 512)).all() and km.sum(1).max() < c.S
    big = C.with_garbage(torch.zeros(2, 5, 2, 4), C.mask_prefix(2, 5, [2, 5]), "fp16")
    assert big[0, 2:].abs().min() == 32752.0 and (big[0, :2] == 0).all() and (big[1] == 0).all() and (big[0, 2] < 0).any()
    assert all(torch.isfinite(torch.tensor(C.garbage_value(dt)).to(C.TDT[dt])) for dt in C.DTS)


def test_long_s_cases_have_33_chunks():
    nb, S, H, D = C.LONG_S["mfma"]
    assert C.route(nb, 1, S, H, D, "fp32")[1] == "la_kv_mfma2_kernel" and C.route(nb, 1, S, H, D, "bf16")[1] == "la_kv_h16_kernel"
    assert C.nchunk(S, "la_kv_mfma2_kernel") == 33 and C.nchunk(S - 1, "la_kv_mfma2_kernel") == 32
    nb, S, H, D = C.LONG_S["plain"]
    assert C.route(nb, 1, S, H, D, "fp32")[1] == "la_kv_kernel" and C.nchunk(S, "la_kv_kernel") == 33 and C.nchunk(S - 1, "la_kv_kernel") == 32


@pytest.mark.parametrize("kind", ["mfma", "plain"])
def test_long_s_reference_margin(kind):
    nb, S, H, D = C.LONG_S[kind]
    k, v = C.state_operands(nb, S, H, D, "fp32", 4200)
    (kv64, ks64), (kv32, ks32) = C.ref_state(k, v), C.fp32_state(k, v)
    dev = max(C.rel_err(kv32, kv64), C.rel_err(ks32, ks64))
    print(f"[la case] long S {kind}: fp32 torch state vs fp64: KV {C.rel_err(kv32, kv64):.2e} Ksum {C.rel_err(ks32, ks64):.2e} of scale; "
          f"recorded {C.LONG_S_FP32_DEV[kind]:.1e}, GPU bar {C.long_s_bar(kind):.1e}")
    assert dev <= C.LONG_S_FP32_DEV[kind] and dev < 0.5 * C.long_s_bar(kind)


@pytest.mark.parametrize("group", ["ROUTING", "PLAIN", "MISALIGNED", "DTYPE_PAIRS", "STRIDED", "MASKED"])
def test_fp32_evaluation_stays_below_half_the_bar(group):
    worst = {}
    for c in getattr(C, group):
        ref = C.case_ref(c)
        assert ref.dtype == torch.float64 and torch.isfinite(ref).all() and ref.abs().max() > 0.1, c.id
        dev = C.rel_err(C.fp32_attention(*C.case_inputs(c)), ref)
        worst[c.dt != "fp32"] = max(worst.get(c.dt != "fp32", 0.0), dev)
        assert dev < 0.5 * C.BAR_OUT[c.odt], (c.id, dev)
    print(f"[la case] {group}: fp32 torch vs fp64, of scale: fp32 inputs {worst.get(False, 0):.2e}, 16-bit inputs {worst.get(True, 0):.2e}")


def test_layout_helpers():
    x = torch.arange(3 * 256, dtype=torch.float32).reshape(3, 256) / 64
    for name, (pm, cm) in C.LAYOUTS["strided"].items():
        buf, sl = C.lay_out(name, x, torch.bfloat16, "strided")
        assert buf.shape == (3, 256 * pm) and sl == slice(256 * cm, 256 * cm + 256) and torch.equal(buf[:, sl], x.bfloat16())
        assert C.foreign_columns_untouched(buf, sl)
        buf[1, sl.start - 1] = -7.0
        assert not C.foreign_columns_untouched(buf, sl)
    buf, sl = C.lay_out("k", x, torch.float16, "misaligned")
    assert buf.shape == (3, 260) and sl == slice(4, 260) and buf.data_ptr() % 16 == 0
    assert buf[:, sl].data_ptr() % 16 == 8 and (buf.stride(0) * 2) % 16 == 8
    assert C.lay_out("q", x, torch.float16, "misaligned")[0].shape == (3, 256)
