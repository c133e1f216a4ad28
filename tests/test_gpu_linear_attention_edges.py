"""csrc/linear_attention.hip at its kernel, dtype, mask and chunk edges, against the float64 references of
tests/linear_attention_cases.py (whose cases tests/test_linear_attention_cases_cpu.py judges on the host): the routing boundary of
ops.linear_attention, the plain (non-MFMA) kernels at every (H, D) they serve and on K / V views that are not 16-byte aligned, every
(input, output) dtype pair, q / k / v / out as column views of wider buffers, padding masks of every kind with large finite values in
the masked rows, the finalize kernel past its first 32 chunks, and the masked state's independence of the batch it travels in.

Bars: of max|ref|, BAR_OUT by output dtype (1e-2 bf16, 1.25e-3 fp16, 1e-5 fp32), BAR_STATE = 1e-5 for the fp32 state."""
import pytest
import torch

import linear_attention_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _u8(m, dev):
    return m.reshape(-1).to(torch.uint8).to(dev) if m is not None else None


def _launch(c, ws=None, garbage=None):
    """run case c through ops.linear_attention -> (out [nb,L,H,D] on the host, the out buffer, its column slice, ws)"""
    from gim_amd import ops
    dev = _dev()
    Q, K, V, qm, km = C.case_inputs(c)
    if c.garbage if garbage is None else garbage:
        Q, K, V = C.with_garbage(Q, qm, c.dt), C.with_garbage(K, km, c.dt), C.with_garbage(V, km, c.dt)
    Cc = c.H * c.D
    bufs = {}
    for name, x, n, dt in (("q", Q, c.L, c.dt), ("k", K, c.S, c.dt), ("v", V, c.S, c.dt), ("out", torch.full_like(Q, C.SENTINEL), c.L, c.odt)):
        buf, sl = C.lay_out(name, x.reshape(c.nb * n, Cc), C.TDT[dt], c.layout)
        bufs[name] = (buf.to(dev), sl)
    view = {n: b[:, sl] for n, (b, sl) in bufs.items()}
    ws = ops.linear_attention(view["q"], view["k"], view["v"], view["out"], c.nb, c.L, c.nb, c.S, c.H, ws, _u8(qm, dev), _u8(km, dev))
    torch.cuda.synchronize()
    obuf, osl = bufs["out"]
    return obuf[:, osl].float().cpu().view(c.nb, c.L, c.H, c.D), obuf, osl, ws


def _check(c, got):
    ref = C.case_ref(c)
    assert torch.isfinite(got).all(), c.id
    err = C.rel_err(got, ref)
    print(f"[la edge] {c.id} ({c.route}): {err:.2e} of scale, bar {C.BAR_OUT[c.odt]:.2e}")
    assert err <= C.BAR_OUT[c.odt], (c.id, err)


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("c", C.ROUTING, ids=_ids(C.ROUTING))
def test_routing_boundary(c):
    """L, S of 64 / 65 around `L <= 64 and S <= 64`; S <= 64 with L > 64 (one chunk: no finalize, the partial IS the state); nb = 1 and
    L = 1; nb of 3, 5, 6: the short kernel's last workgroup holds fewer than four sequences"""
    _check(c, _launch(c)[0])


@pytest.mark.parametrize("c", C.PLAIN, ids=_ids(C.PLAIN))
def test_plain_kernels(c):
    """la_kv_kernel<16|32> + la_apply_kernel<16|32>: everything but H = 8, D = 32 -- 1, 1, 2 and 3 chunks of 128 rows, H below / above the
    four waves of an apply workgroup, H = 15 at D = 32 (63 360 B of LDS: the largest state that fits)"""
    _check(c, _launch(c)[0])


def test_plain_apply_refuses_a_state_beyond_64k():
    """H = 16, D = 32: 67 584 B of state; gim_linear_attention_apply refuses before its launch and writes nothing"""
    from gim_amd import _lib, ops
    dev = _dev()
    nb, L, S, H, D = 1, 65, 65, 16, 32
    q, k, v = (torch.ones(nb * n, H * D, device=dev) for n in (L, S, S))
    out = torch.full((nb * L, H * D), C.SENTINEL, device=dev)
    with pytest.raises(_lib.GimHipError, match="too large"):
        ops.linear_attention(q, k, v, out, nb, L, nb, S, H)
    torch.cuda.synchronize()
    assert bool((out == C.SENTINEL).all())


@pytest.mark.parametrize("c", C.MISALIGNED, ids=_ids(C.MISALIGNED))
def test_misaligned_kv_views_take_the_plain_kv_kernel(c):
    """16-bit H = 8, D = 32 with K / V starting 8 bytes past a 16-byte boundary, rows 520 bytes apart: the MFMA KV kernels' 16-byte loads
    do not apply, la_kv_kernel<32> computes the state (128-row partials), la_apply_mfma_kernel consumes it.  Same reference as the
    aligned layout; the two states agree to the state bar (not bit for bit: other chunks, 1 / S before / after the sum)."""
    from gim_amd import ops
    dev = _dev()
    got, _, _, _ = _launch(c)
    _check(c, got)
    _, K, V, _, km = C.case_inputs(c)
    if c.garbage:
        K, V = C.with_garbage(K, km, c.dt), C.with_garbage(V, km, c.dt)
    n = c.nb * c.H * (c.D * c.D + c.D)
    states = []
    for layout in ("misaligned", "plain"):
        (kb, ksl), (vb, vsl) = (C.lay_out(nm, x.reshape(c.nb * c.S, 256), C.TDT[c.dt], layout) for nm, x in (("k", K), ("v", V)))
        kd, vd = kb.to(dev)[:, ksl], vb.to(dev)[:, vsl]
        assert kd.data_ptr() % 16 == (8 if layout == "misaligned" else 0) and vd.data_ptr() % 16 == kd.data_ptr() % 16
        ws, _ = ops.linear_attention_state(kd, vd, c.nb, c.S, c.H, None, _u8(km, dev))
        torch.cuda.synchronize()
        states.append(ws[:n].cpu().view(c.nb, c.H, -1))
    kv_ref, ks_ref = C.ref_state(*C.case_inputs(c)[1:3], km)
    for st in states:
        assert C.rel_err(st[..., :c.D * c.D], kv_ref) <= C.BAR_STATE and C.rel_err(st[..., c.D * c.D:], ks_ref) <= C.BAR_STATE
    d_kv, d_ks = C.rel_err(states[0][..., :c.D * c.D], states[1][..., :c.D * c.D]), C.rel_err(states[0][..., c.D * c.D:], states[1][..., c.D * c.D:])
    print(f"[la edge] {c.id}: misaligned vs aligned state: KV {d_kv:.2e} Ksum {d_ks:.2e} of scale")
    assert d_kv <= C.BAR_STATE and d_ks <= C.BAR_STATE


@pytest.mark.parametrize("c", C.DTYPE_PAIRS, ids=_ids(C.DTYPE_PAIRS))
def test_dtype_pairs(c):
    """every (input, output) pair the entry points accept; the bar follows the OUTPUT dtype, the reference knows the input rounding only"""
    _check(c, _launch(c)[0])


@pytest.mark.parametrize("c", C.STRIDED, ids=_ids(C.STRIDED))
def test_strided_everything(c):
    """q, k, v and out as column views (pitches 2C / 3C, sentinels around them): ldq / ldk / ldv / ldo all differ from C, and the
    columns of the out buffer that are not out's keep their bits"""
    got, obuf, osl, _ = _launch(c)
    _check(c, got)
    assert obuf.shape[1] == 3 * c.H * c.D and C.foreign_columns_untouched(obuf, osl), c.id


@pytest.mark.parametrize("c", C.MASKED, ids=_ids(C.MASKED))
def test_masks_with_garbage_in_masked_rows(c):
    """q_mask / kv_mask of every kind on the short, MFMA and plain routes, in all three dtypes, with 0.5 x max (16-bit) / 1e30 (fp32) in
    the masked rows of q, k and v: a masked row must be dropped, not multiplied.  Fully q-masked rows and fully kv-masked sequences
    give exactly 0.0; the all-valid sequence beside them gives what it gives alone.
    Each case runs a second time with the masked rows left as drawn: 0.5 x bf16's max in a q row makes q.Ksum ~1e38, whose reciprocal
    is a denormal that flushes to zero, so a kernel that ignored q_mask would still store 0.0 there -- ordinary values show it."""
    _, _, _, qm, km = C.case_inputs(c)
    dead = ~km.any(1)
    for garbage in (True, False):
        got, _, _, _ = _launch(c, garbage=garbage)
        _check(c, got)
        assert bool((got[~qm] == 0.0).all()), (c.id, garbage)
        assert bool((got[dead] == 0.0).all()), (c.id, garbage)
    if c.mask == "seqzero":
        assert dead.tolist() == [False, True] + [False] * (c.nb - 2) and not qm[0].any()
        Q, K, V, _, _ = C.case_inputs(c)
        alone = C.ref_attention(Q[-1:], K[-1:], V[-1:])
        assert C.rel_err(got[-1:], alone) <= C.BAR_OUT[c.odt], c.id


# ------------------------------------------------------------------------------------------------------------ state
def _state(k, v, nb, S, H, D, dt, km=None, garbage=False):
    """ops.linear_attention_state of host operands k / v [nb,S,H,D] -> (state [nb, H*(D*D+D)] fp32 on the device, ws, need)"""
    from gim_amd import ops
    dev = _dev()
    if garbage:
        k, v = C.with_garbage(k, km, dt), C.with_garbage(v, km, dt)
    kd, vd = (x.reshape(nb * S, H * D).to(C.TDT[dt]).to(dev) for x in (k, v))
    ws, need = ops.linear_attention_state(kd, vd, nb, S, H, None, _u8(km, dev))
    torch.cuda.synchronize()
    return ws[:nb * H * (D * D + D)].view(nb, H * (D * D + D)).clone(), ws, need


def _check_state(tag, st, ref, nb, H, D, bar):
    st = st.cpu().view(nb, H, D * D + D)
    assert torch.isfinite(st).all(), tag
    e_kv, e_ks = C.rel_err(st[..., :D * D], ref[0]), C.rel_err(st[..., D * D:], ref[1])
    print(f"[la edge] state {tag}: KV {e_kv:.2e} Ksum {e_ks:.2e} of scale, bar {bar:.1e}")
    assert e_kv <= bar and e_ks <= bar, (tag, e_kv, e_ks)


@pytest.mark.parametrize("masked", [True, False], ids=["prefix8192", "unmasked"])
@pytest.mark.parametrize("kind,dt", [("mfma", "fp32"), ("mfma", "bf16"), ("mfma", "fp16"), ("plain", "fp32"), ("plain", "fp16")])
def test_state_over_33_chunks(kind, dt, masked):
    """la_kv_finalize_kernel's second trip (c0 += 32): S = 8193 = 32 x 256 + 1 on the MFMA path, S = 4097 = 32 x 128 + 1 on the plain one
    (H = 4).  `prefix8192` masks all but the first S - 1 rows (garbage in the one masked row, the 33rd partial is zero); unmasked, the
    33rd partial carries the last row, which a finalize pass that stopped after 32 chunks would drop (2e-4 of Ksum).
    Bar: max(1e-5, 4 x the fp32 host deviation) = 1e-5; the host deviation of a plain fp32 torch state is 3.8e-7 (S = 8193) / 4.5e-7
    (S = 4097) of scale, recorded rounded up as linear_attention_cases.LONG_S_FP32_DEV = 1e-6.
    Measured on the MI355X, of scale (KV / Ksum): S = 8193 fp32 2.0e-7 / 1.3e-7, bf16 1.0e-7 / 1.0e-7, fp16 1.2e-7 / 1.1e-7;
    S = 4097 (plain) fp32 2.6e-7 / 1.4e-7, fp16 2.5e-7 / 1.0e-7 -- masked and unmasked alike, under a thirtieth of the bar."""
    nb, S, H, D = C.LONG_S[kind]
    k, v = C.state_operands(nb, S, H, D, dt, 4200)
    km = C.mask_prefix(nb, S, S - 1) if masked else None
    st, _, _ = _state(k, v, nb, S, H, D, dt, km, garbage=masked)
    _check_state(f"{kind} S={S} {dt} {'prefix' if masked else 'unmasked'}", st, C.ref_state(k, v, km), nb, H, D, C.long_s_bar(kind))


@pytest.mark.parametrize("mask", ["random", "prefix256"])
@pytest.mark.parametrize("dt", C.DTS)
def test_masked_state_is_batch_invariant(dt, mask):
    """(130, 257) with kv_mask and garbage: 16-bit, the large call runs la_kv_h16_kernel<512> (one wave owns a 256-row chunk in two
    accumulator sets, both of which must honour the mask), the two-sequence calls la_kv_h16_kernel<256>; fp32, la_kv_mfma2_kernel both
    times.  The states of sequences [0, 2) and [128, 130) computed alone are BIT-identical to their rows of the large call, and the
    large call's state meets the reference."""
    nb, S = C.INVARIANCE
    H, D = 8, 32
    assert nb * ((S + 255) // 256) * 2 > 512 and 2 * ((S + 255) // 256) * 2 <= 512    # 512-row shape for nb, 256-row shape for 2
    k, v = C.state_operands(nb, S, H, D, dt, 4300)
    km = C.mask_random(nb, S, 4301) if mask == "random" else C.mask_prefix_chunks(nb, S, 1)
    big, _, _ = _state(k, v, nb, S, H, D, dt, km, garbage=True)
    _check_state(f"{nb}x{S} {dt} {mask}", big, C.ref_state(k, v, km), nb, H, D, C.BAR_STATE)
    for b0 in (0, nb - 2):
        small, _, _ = _state(k[b0:b0 + 2], v[b0:b0 + 2], 2, S, H, D, dt, km[b0:b0 + 2], garbage=True)
        assert torch.equal(small, big[b0:b0 + 2]), (dt, mask, b0, (small - big[b0:b0 + 2]).abs().max().item())


def test_workspace_handling():
    """a too-small ws is replaced, a large enough one comes back as the same object, `need` is gim_linear_attention_ws_bytes"""
    from gim_amd import ops
    from gim_amd._lib import lib
    dev = _dev()
    c = next(x for x in C.DTYPE_PAIRS if x.route == "mfma" and x.dt == x.odt == "fp32")
    need = lib.gim_linear_attention_ws_bytes(c.nb, c.S, c.H, c.D)
    assert need == c.nb * c.H * (c.D * c.D + c.D) * 4 * ((c.S + 127) // 128 + 1)
    small = torch.empty(need // 4 - 1, dtype=torch.float32, device=dev)
    got, _, _, ws = _launch(c, small)
    _check(c, got)
    assert ws is not small and ws.numel() * 4 >= need
    exact = torch.empty(need // 4, dtype=torch.float32, device=dev)
    got, _, _, ws = _launch(c, exact)
    _check(c, got)
    assert ws is exact
    Q, K, V, _, _ = C.case_inputs(c)
    kd, vd = (x.reshape(c.nb * c.S, c.H * c.D).to(dev) for x in (K, V))
    ws2, need2 = ops.linear_attention_state(kd, vd, c.nb, c.S, c.H, exact)
    assert ws2 is exact and need2 == need
    ws3, need3 = ops.linear_attention_state(kd, vd, c.nb, c.S, c.H, small)
    assert ws3 is not small and need3 == need and ws3.numel() * 4 >= need
    torch.cuda.synchronize()
    assert torch.equal(ws2[:c.nb * c.H * (c.D * c.D + c.D)], ws3[:c.nb * c.H * (c.D * c.D + c.D)])
    one = lib.gim_linear_attention_ws_bytes(5, 64, 8, 16)            # one chunk: the partial is the state, no room for partials
    assert one == 5 * 8 * (16 * 16 + 16) * 4
