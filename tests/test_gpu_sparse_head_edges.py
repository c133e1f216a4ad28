"""The sparse path's index-producing kernels at their edges: SuperPoint's selection tail (sp_nms, sp_topk, sp_sample_desc) and LightGlue's
assignment (lg_assign, lg_log_assignment, lg_emit_matches), through the C ABI, against the plain references of
tests/sparse_head_cases.py (checked on the CPU by tests/test_sparse_head_cases_cpu.py) and the oracle.

Bars: those of tests/test_gpu_lightglue.py -- keypoint coordinates, arg-max / match indices, `count`, the packed lists' indices, m_bids
and the scaled keypoints: exact; fp32 floats: 2e-5 of the reference's scale (sp_sample_desc: 2e-6, as there).  Match indices are
compared everywhere but at the rows / columns sparse_head_cases.exempt() names (arg-max gap below 1e-3 in float64); the CPU test caps
them at 1 % per case, and on the seeded cases of this file there are none.

Largest fraction of scale measured on MI355X (one run, pytest -s, as _close prints them; bar 2e-5), per lg_assign case family,
mscores0 (= mscores1, = the scores list) / log_assignment:
  ragged (3,129,127) / (2,257,64) / (2,1100,1030)   4.5e-6 / 7.6e-6 / 1.00e-5       4.5e-7 / 5.1e-7 / 6.5e-7
  degenerate (1,1,5) (1,5,1) (1,1,1) (2,1,130)      <= 6.2e-8 (0 at N = 1)           <= 4.7e-7
  ties, columns / rows (2,200,260) / (2,260,200)    6.2e-6 / 5.0e-6                  5.4e-7 / 5.3e-7
  empty pair in the middle (3,150,140)              6.4e-6                           4.9e-7
  no match / threshold 0 (2,140,150)                5.9e-6                           4.5e-7
  unscaled final_proj (2,300,170)                   5.0e-6                           5.6e-7
(the matching scores' share is the fp32 rounding of similarities of magnitude ~300 ahead of exp(): the fp32 CPU oracle sits at 6e-6 ...
1.3e-5 from float64 on the inputs of test_lg_assign, tests/test_sparse_head_cases_cpu.py.)  sp_sample_desc (bar 2e-6): 4.0e-7.
"""
import pytest
import torch
import torch.nn.functional as F

import lightglue_oracle as O
import sparse_head_cases as C

pytestmark = pytest.mark.gpu
DTS = ["fp32", "bf16", "fp16"]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _tdt(dt):
    return {"bf16": torch.bfloat16, "fp16": torch.float16}.get(dt, torch.float32)


def _close(got, ref, tol, what=""):
    """tests/test_gpu_lightglue.py::_close"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    print(f"[close] {what}: {err / scale:.3e} of scale (tol {tol:g})")   # pytest -s: the measured value
    assert err <= tol * scale, f"{what}: max|err|={err:.3e} scale={scale:.3e} tol={tol}"


# ------------------------------------------------------------------------------------------------ lg_assign
def _run_assign(c, ld=None):
    """ops.lg_assign on the case; ld: descriptors as [:, :, :256] views of [B, n, ld] buffers whose padding is NaN"""
    from gim_amd import ops
    dev = _dev()
    p = f"log_assignment.{C.LAYER}"
    d0, d1 = c["d0"].to(dev), c["d1"].to(dev)
    if ld is not None:
        bufs = [torch.full((*d.shape[:2], ld), float("nan"), device=dev) for d in (d0, d1)]
        for buf, d in zip(bufs, (d0, d1)):
            buf[:, :, :256] = d
        d0, d1 = bufs[0][:, :, :256], bufs[1][:, :, :256]
        assert d0.stride(1) == ld and not d0.is_contiguous()
    return ops.lg_assign(d0, d1, c["md0"].to(dev), c["md1"].to(dev), c["sd"][p + ".matchability.weight"].reshape(-1).to(dev),
                         c["sd"][p + ".matchability.bias"].to(dev), c["th"])


def _check_assign(name):
    """the checks of test_lg_assign, against assign_reference; -> (result, reference)"""
    from gim_amd import ops
    dev = _dev()
    c, ref = C.assign_case(name), C.assign_ref(name)
    B, M, N = c["B"], c["M"], c["N"]
    r = _run_assign(c)
    e0, e1 = C.exempt(ref)
    m0, m1 = r.matches0.cpu(), r.matches1.cpu()
    assert m0.dtype == torch.int64 and m0.shape == (B, M) and m1.shape == (B, N)
    assert torch.equal(m0[~e0], ref["m0"][~e0]), f"{name}: matches0"
    assert torch.equal(m1[~e1], ref["m1"][~e1]), f"{name}: matches1"
    _close(r.mscores0.cpu()[~e0], ref["ms0"][~e0], 2e-5, f"{name} mscores0")
    _close(r.mscores1.cpu()[~e1], ref["ms1"][~e1], 2e-5, f"{name} mscores1")
    count = r.count.tolist()
    assert count == [(m0[b] > -1).sum().item() for b in range(B)]
    if not e0.any():
        assert count == [(ref["m0"][b] > -1).sum().item() for b in range(B)]
    la = ops.lg_log_assignment(r)
    _close(la, ref["scores"], 2e-5, f"{name} log_assignment")          # every element: core, dustbin row and column, corner
    assert (la[:, M, N] == 0).all()
    total = sum(count)
    kp0, kp1, sc0, sc1 = C.emit_inputs(c)
    matches, sc, mk0, mk1, bids = ops.lg_emit_matches(r, total, kp0.to(dev), kp1.to(dev), sc0.to(dev), sc1.to(dev))
    assert (matches.shape, matches.dtype, sc.shape, sc.dtype) == ((total, 2), torch.int64, (total,), torch.float32)
    assert (mk0.shape, mk0.dtype, mk1.shape, bids.shape, bids.dtype) == ((total, 2), torch.float32, (total, 2), (total,), torch.int64)
    # the lists follow matches0 (the reference's, where no index is exempt): torch.where order, pair after pair
    exp_m, exp_s, exp0, exp1, exp_b = C.expected_lists(m0 if e0.any() else ref["m0"], ref["ms0"], kp0, kp1, sc0, sc1)
    assert torch.equal(matches.cpu(), exp_m) and torch.equal(bids.cpu(), exp_b)
    assert torch.equal(mk0.cpu(), exp0) and torch.equal(mk1.cpu(), exp1)
    if total:
        _close(sc, exp_s, 2e-5, f"{name} scores list")
    return r, ref, (matches, sc, mk0, mk1, bids)


@pytest.mark.parametrize("name", ["ragged_129_127", "ragged_257_64", "filter_1100"])
def test_lg_assign_ragged_batches(name):
    """partial 128-tiles on both sides with B > 1 (the batch offsets of rowpart / colpart / best / ls), and 1100 rows: the filter's
    second compaction round is partially filled, with matches on both sides of row 1024 (the carried s_base decides `pos`)"""
    r, ref, _ = _check_assign(name)
    if name == "filter_1100":
        pos, m0 = r.pos.cpu(), ref["m0"]
        for b in range(2):
            rows = torch.where(m0[b] > -1)[0]
            assert (rows >= 1024).any() and (rows < 1024).any()
            assert torch.equal(pos[b][rows], torch.arange(len(rows), dtype=torch.int32))
            assert (pos[b][m0[b] < 0] == -1).all()


@pytest.mark.parametrize("name", ["m1_n5", "m5_n1", "m1_n1", "m1_n130"])
def test_lg_assign_degenerate(name):
    """one keypoint on a side: the 128 x 128 tile loop reads a one-row matrix; every element of log_assignment is compared"""
    _check_assign(name)


@pytest.mark.parametrize("name", ["ties_cols", "ties_rows"])
def test_lg_assign_ties(name):
    """bit-identical columns (rows): the lower index of each pair takes the match, the higher gets -1 / score 0 -- inside one tile (the
    key comparison), across tiles (the atomicMax) and with the higher one in the ragged last tile"""
    r, ref, _ = _check_assign(name)
    c = C.assign_case(name)
    side = c["dup"][0][0]
    mm, ms = (r.matches1.cpu(), r.mscores1.cpu()) if side == 1 else (r.matches0.cpu(), r.mscores0.cpu())
    other = r.matches0.cpu() if side == 1 else r.matches1.cpu()
    for _, b, j, jj in c["dup"]:
        assert int(mm[b, jj]) == -1 and float(ms[b, jj]) == 0.0, (b, j, jj)
        assert int(mm[b, j]) > -1 and int(other[b, int(mm[b, j])]) == j, (b, j, jj)


def test_lg_assign_empty_pair_in_the_middle():
    """B = 3, pair 1 without a match: lga_emit's offset of pair 2 is the prefix sum over `count` = count[0] + 0"""
    r, ref, (matches, sc, mk0, mk1, bids) = _check_assign("empty_middle")
    count = r.count.tolist()
    assert count[1] == 0 and count[0] > 0 and count[2] > 0
    assert (r.matches0[1] == -1).all() and (r.matches1[1] == -1).all() and (r.pos[1] == -1).all()
    assert set(bids.tolist()) == {0, 2}
    # pair 2 on its own: its slice of the lists starts right behind pair 0's
    c = C.assign_case("empty_middle")
    kp0, kp1, sc0, sc1 = C.emit_inputs(c)
    rows = torch.where(ref["m0"][2] > -1)[0]
    cols = ref["m0"][2][rows]
    tail = slice(count[0], count[0] + count[2])
    assert torch.equal(matches.cpu()[tail], torch.stack([rows, cols], -1))
    assert torch.equal(mk0.cpu()[tail], kp0[2][rows] * sc0[2]) and torch.equal(mk1.cpu()[tail], kp1[2][cols] * sc1[2])


def test_lg_assign_no_match():
    """threshold 1.0: count == 0, every match -1, mscores still the reference's; lg_emit_matches(total = 0) -> empty tensors"""
    r, ref, lists = _check_assign("no_match")
    assert r.count.tolist() == [0, 0]
    assert (r.matches0 == -1).all() and (r.matches1 == -1).all() and (r.pos == -1).all()
    assert (r.mscores0 > 0).any()
    for t, shape, dtype in zip(lists, ((0, 2), (0,), (0, 2), (0, 2), (0,)),
                               (torch.int64, torch.float32, torch.float32, torch.float32, torch.int64)):
        assert t.shape == shape and t.dtype == dtype


def test_lg_assign_threshold_zero():
    """threshold 0.0: every mutual pair is valid"""
    r, ref, _ = _check_assign("thr_zero")
    assert torch.equal(r.matches0.cpu() > -1, ref["ms0"] > 0) and torch.equal(r.matches1.cpu() > -1, ref["ms1"] > 0)
    assert torch.equal((r.mscores0 > 0).cpu(), ref["ms0"] > 0)


def test_lg_assign_row_stride():
    """descriptors as [:, :, :256] views of [B, n, 320] buffers (what lightglue.py passes): bit for bit the contiguous call"""
    from gim_amd import ops
    c = C.assign_case("ragged_129_127")
    a, b = _run_assign(c), _run_assign(c, ld=320)
    assert b.args.ld_desc == 320 and a.args.ld_desc == 256
    for k in ("matches0", "matches1", "mscores0", "mscores1", "pos", "count"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(ops.lg_log_assignment(a), ops.lg_log_assignment(b))


def test_lg_assign_unscaled_final_proj():
    """final_proj as the model has it (40 I + w) on O.planted_descriptors: the peaked softmax the real model runs in -- |sim| up to 84,
    matching scores up to 0.93.  The fp32 oracle stays at 5.3e-7 (log_assignment) / 3.8e-6 (mscores0) of scale from float64 on this
    input (tests/test_sparse_head_cases_cpu.py), below half the bar, so the floats are compared too."""
    r, ref, _ = _check_assign("unscaled")
    assert float(r.mscores0.max()) > 0.9


# ------------------------------------------------------------------------------------------------ sp_topk
def _check_topk(s, k, thr):
    from gim_amd import ops
    kpts, ksc, nv = ops.sp_topk(s.to(_dev()), k, thr)
    B = s.shape[0]
    assert kpts.shape == (B, k, 2) and ksc.shape == (B, k) and nv.dtype == torch.int32
    ref_k, ref_s, ref_n = C.topk_reference(s, thr, k)
    kpts, ksc = kpts.cpu(), ksc.cpu()
    assert nv.tolist() == ref_n
    for b in range(B):
        n = ref_n[b]
        assert torch.equal(kpts[b, :n], ref_k[b]), b
        assert torch.equal(ksc[b, :n], ref_s[b]), b
        assert (kpts[b, n:] == 0).all() and (ksc[b, n:] == 0).all()
    return ref_n


@pytest.mark.parametrize("k", [1, 1000, 2048, 4096])
def test_sp_topk_many_candidates(k):
    """15360 candidates per image (4 candidate workgroups, n > 4096): the radix-select and gather loops take 15 trips; k = 1: no sort
    pass"""
    assert _check_topk(C.distinct_map(3, *C.TOPK_HW, seed=41), k, 0.0) == [k] * 3


def test_sp_topk_ties_across_workgroups():
    """16 levels of 960 pixels each: the k-th boundary falls inside a level whose pixels lie in all 4 candidate workgroups (their append
    order into the list is not deterministic); kept: the lowest flat indices of that level"""
    _check_topk(C.quantised_map(3, *C.TOPK_HW, seed=42), C.TIE_K, 0.0)


@pytest.mark.parametrize("dk", [-1, 0, 1])
def test_sp_topk_few_switch(dk):
    """exactly n candidates over several workgroups, k = n - 1 (top-k, sorted by score), n and n + 1 (all, in flat-index order)"""
    n = _check_topk(C.sparse_map(2, *C.TOPK_HW, C.FEW_N, seed=43), C.FEW_N + dk, 0.0)
    assert n == [min(C.FEW_N, C.FEW_N + dk)] * 2


def test_sp_topk_empty_map():
    s = torch.zeros(2, 40, 56)
    s[1, :4] = -1.0                      # a masked border is no candidate either
    assert _check_topk(s, 64, 0.0) == [0, 0]


@pytest.mark.parametrize("k", [4096, 300])
def test_sp_topk_threshold_equality(k):
    """score == thr is no candidate, one ulp above is"""
    s, above = C.threshold_map(C.THR, seed=44)
    n = _check_topk(s, k, C.THR)
    assert n == [min(k, int((s[b] == above).sum())) for b in range(2)]


def test_sp_topk_mixed_batch():
    """one call: n > k, n <= k and n == 0"""
    H, W = C.TOPK_HW
    s = torch.cat([C.distinct_map(1, H, W, seed=45), C.sparse_map(1, H, W, C.FEW_N, seed=46), torch.zeros(1, H, W)])
    assert _check_topk(s, 500, 0.0) == [500, C.FEW_N, 0]


def test_sp_topk_batch_limit():
    """64 images per call are accepted, 65 are refused before anything is launched or written"""
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    dev = _dev()
    _check_topk(C.distinct_map(64, 8, 8, seed=47), 10, 0.5)
    s = C.distinct_map(65, 8, 8, seed=47).to(dev)
    with pytest.raises(GimHipError):
        ops.sp_topk(s, 10, 0.5)
    ws = torch.full((ops.lib.gim_sp_topk_ws_bytes(65, 8, 8),), 7, dtype=torch.uint8, device=dev)
    kpts, ksc = torch.full((65, 10, 2), 7.0, device=dev), torch.full((65, 10), 7.0, device=dev)
    nv = torch.full((65,), 7, dtype=torch.int32, device=dev)
    rc = ops.lib.gim_sp_topk(ops._p(s), ops._p(ws), ops._p(kpts), ops._p(ksc), ops._p(nv), 65, 8, 8, 10, 0.5, ops._stream())
    assert rc != 0
    torch.cuda.synchronize()
    assert (ws == 7).all() and (kpts == 7.0).all() and (ksc == 7.0).all() and (nv == 7).all()


# ------------------------------------------------------------------------------------------------ sp_nms
_NMS = [(H, W, r, 0) for H, W in ((50, 72), (17, 130), (5, 7), (1, 40)) for r in (0, 1, 4, 8)] + [(50, 72, 4, 4), (50, 72, 4, 30),
                                                                                                    (50, 72, 8, 4)]


@pytest.mark.parametrize("H,W,radius,border", _NMS)
def test_sp_nms_edges(H, W, radius, border):
    """H no multiple of the 16-row tile, maps narrower than a tile and than the radius, radius 0 and 8 (the whole LDS halo), plateaus
    across the tile borders x = 64 / y = 16, a border that masks every row, two images of different content"""
    from gim_amd import ops
    s = C.smooth_map(2, H, W, seed=48)
    assert not torch.equal(s[0], s[1])
    got = ops.sp_nms(s.to(_dev()), radius, border).cpu()
    ref = O.simple_nms(s, radius)
    if border:
        ref = O.mask_borders(ref, torch.tensor([[W, H]] * 2), border)
    if border == 30:
        assert (ref == -1).all()
    if radius == 0:
        assert torch.equal(O.simple_nms(s, 0), s)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ sp_sample_desc
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,w", [(2, 2), (3, 9)])
def test_sp_sample_desc_edges(dt, h, w):
    """B*K = 213 keypoints: the last workgroup has one wave that returns early; keypoints on the four image corners and along the last
    row and column (outside the sample grid), on the smallest descriptor map and on a 3 x 9 one; checks as test_sp_sample_desc"""
    from gim_amd import ops
    dev = _dev()
    B, K = 3, 71
    g = torch.Generator().manual_seed(49)
    dense = torch.randn(B, 256, h, w, generator=g).to(_tdt(dt)).float()
    kp = C.sample_desc_keypoints(B, K, h, w, seed=50)
    ref = O.sample_descriptors_legacy(kp.clone(), F.normalize(dense, p=2, dim=1), 8).transpose(-1, -2)
    rows = dense.permute(0, 2, 3, 1).reshape(B * h * w, 256).contiguous().to(_tdt(dt)).to(dev)
    out = torch.full((B * K + 3, 256), 7.0, device=dev)
    out_t = torch.full((B * K + 3, 320), 7.0, dtype=_tdt(dt), device=dev)
    ops.sp_sample_desc(rows, kp.to(dev), h, w, out[:B * K], out_t[:B * K, :256])
    _close(out[:B * K].view(B, K, 256), ref, 2e-6, f"sample_desc {dt} {h}x{w}")
    assert torch.equal(out_t[:B * K, :256], out[:B * K].to(_tdt(dt)))
    assert (out_t[:, 256:] == 7.0).all() and (out[B * K:] == 7.0).all() and (out_t[B * K:] == 7.0).all()
