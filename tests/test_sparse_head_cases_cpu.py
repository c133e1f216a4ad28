"""The references and case families of tests/sparse_head_cases.py, checked without a GPU: topk_reference against O.select_keypoints where
that is defined (distinct scores) and against the tie order the existing GPU test expects; assign_reference (float64) against the fp32
oracle on the inputs of the existing test_lg_assign; and, per assignment case, the properties the GPU tests rely on -- tie groups are the
planted duplicates and nothing else, at most 1 % of the rows plus columns have an arg-max gap below LOW_GAP, match-rich cases are
match-rich, no-match cases have none, and no reference score sits within 1e-4 (relative) of the threshold."""
import numpy as np
import pytest
import torch

import lightglue_oracle as O
import sparse_head_cases as C


# ------------------------------------------------------------------------------------------------ sp_topk
@pytest.mark.parametrize("k", [1, 1000, 4096, 20000])
@pytest.mark.parametrize("thr", [0.0, 0.5])
def test_topk_reference_equals_oracle_on_distinct_scores(k, thr):
    s = C.distinct_map(3, *C.TOPK_HW, seed=41)
    kp, sc, nv = C.topk_reference(s, thr, k)
    ref_k, ref_s = O.select_keypoints(s, thr, k)
    for b in range(3):
        assert nv[b] == len(ref_k[b]) == min(k, int((s[b] > thr).sum()))
        assert torch.equal(kp[b], ref_k[b]) and torch.equal(sc[b], ref_s[b])


def test_topk_reference_reproduces_ties_and_plateau():
    """the expected output of test_gpu_lightglue.py::test_sp_topk_ties_and_plateau"""
    nms = torch.zeros(1, 32, 32)
    nms[0, 5:9, 5:9] = 0.5
    nms[0, 20, 3] = 0.7
    kp, sc, nv = C.topk_reference(nms, 0.0, 8)
    assert nv == [8]
    assert kp[0][0].tolist() == [3.0, 20.0] and float(sc[0][0]) == pytest.approx(0.7)
    assert kp[0][1:].tolist() == [[5.0 + i, 5.0] for i in range(4)] + [[5.0 + i, 6.0] for i in range(3)]
    kp, sc, nv = C.topk_reference(nms, 0.0, 64)          # fewer candidates than k: flat-index order, the 0.7 pixel last
    assert nv == [17] and kp[0][-1].tolist() == [3.0, 20.0] and kp[0][0].tolist() == [5.0, 5.0]


def test_topk_case_families():
    H, W = C.TOPK_HW
    s = C.quantised_map(3, H, W, seed=42)
    for b in range(3):
        flat = s[b].reshape(-1)
        levels = torch.unique(flat)
        assert len(levels) == 16 and all(int((flat == v).sum()) == 960 for v in levels)
        above = int((flat > levels[-4]).sum())
        assert above < C.TIE_K < above + 960                      # the cut falls inside the fourth level from the top
        idx = torch.where(flat == levels[-4])[0]
        kept, dropped = idx[:C.TIE_K - above], idx[C.TIE_K - above:]
        assert set((idx // C.CAND_PPB).tolist()) == {0, 1, 2, 3}                # the level lies in all four candidate workgroups,
        assert len(set((kept // C.CAND_PPB).tolist())) > 1 and len(dropped)     # the kept part in more than one
        kp, sc, nv = C.topk_reference(s[b:b + 1], 0.0, C.TIE_K)
        got = (kp[0][:, 1] * W + kp[0][:, 0]).long()
        assert torch.equal(got[above:], kept) and (sc[0][above:] == levels[-4]).all()
    f = C.sparse_map(2, H, W, C.FEW_N, seed=43)
    for b in range(2):
        pos = torch.where(f[b].reshape(-1) > 0)[0]
        assert len(pos) == C.FEW_N and len(set((pos // C.CAND_PPB).tolist())) >= 2
    t, above = C.threshold_map(C.THR, seed=44)
    assert np.float32(C.THR) == C.THR and above > C.THR
    assert min(int((t == v).sum()) for v in (C.THR, above)) > 100 and int(((t < C.THR) & (t > 0)).sum()) > 100
    kp, sc, nv = C.topk_reference(t, C.THR, 4096)
    assert nv == [int((t[b] == above).sum()) for b in range(2)] and all((x == above).all() for x in sc)


# ------------------------------------------------------------------------------------------------ lg_assign
def _frac(a, b):
    return ((a - b).abs().max() / max(1e-6, b.abs().max())).item()


@pytest.mark.parametrize("name", ["base_128", "base_300_170", "base_2048", "unscaled"])
def test_assign_reference_vs_fp32_oracle(name):
    """float64 restatement vs O.log_assignment / O.filter_matches (fp32) on the three inputs of test_lg_assign and on the unscaled case:
    the same matches0 / matches1, and `scores` (the log_assignment matrix) within HALF of the 2e-5-of-scale bar of test_gpu_lightglue.py,
    so that the GPU tests can put the float64 numbers where that file has the fp32 oracle's, at the same bar.
    Measured, fraction of scale, in the order of the parameters: log_assignment 5.3e-7 / 5.9e-7 / 6.0e-7 / 5.3e-7.
    matching_scores0 = exp(row maximum) are printed too: 6.2e-6 / 7.3e-6 / 1.33e-5 / 3.8e-6.  These are the fp32 oracle's own error, not
    the reference's: its fp32 similarity sum over 256 products is off by up to 2.2e-4 (absolute, at |sim| up to 362) against the float64
    sum of the same fp32 final_proj rows, which alone moves exp(score) by 1.2e-5 of scale at 2048 x 2048.  They are asserted at the bar
    itself; the GPU tests of the new cases compare with float64, which is the tighter of the two references."""
    c, ref = C.assign_case(name), C.assign_ref(name)
    scores, _ = O.log_assignment(c["sd"], C.LAYER, c["d0"], c["d1"])
    m0, m1, ms0, ms1 = O.filter_matches(scores, c["th"])
    e0, e1 = C.exempt(ref)
    print(f"[exempt] {name}: {int(e0.sum())} rows, {int(e1.sum())} columns")
    assert e0.float().mean() <= 0.01 and e1.float().mean() <= 0.01          # base_2048: one row of 4096; the others: none
    assert torch.equal(m0[~e0], ref["m0"][~e0]) and torch.equal(m1[~e1], ref["m1"][~e1])
    for what, a, b, ok, bar in (("log_assignment", scores, ref["scores"], None, 1e-5), ("mscores0", ms0, ref["ms0"], ~e0, 2e-5),
                                ("mscores1", ms1, ref["ms1"], ~e1, 2e-5)):
        f = _frac(a.double() if ok is None else a.double()[ok], b if ok is None else b[ok])
        print(f"[oracle vs float64] {name} {what}: {f:.3e} of scale (asserted below {bar:g})")
        assert f < bar, (name, what, f)


@pytest.mark.parametrize("name", C.EDGE_CASES)
def test_assign_case_properties(name):
    c, ref = C.assign_case(name), C.assign_ref(name)
    B, M, N, th = c["B"], c["M"], c["N"], c["th"]
    assert ref["scores"].shape == (B, M + 1, N + 1) and torch.isfinite(ref["scores"]).all()
    # ---- tie groups: exactly the planted duplicates
    tied_rows, tied_cols = ref["size0"] > 1, ref["size1"] > 1
    if not c["dup"]:
        assert not tied_rows.any() and not tied_cols.any()
    else:
        side = c["dup"][0][0]
        # duplicate columns (side 1) tie in the ROW arg-max of every row whose best column is the lower one of a pair, and vice versa
        arg, tied, other, size = ((ref["arg0"], tied_rows, tied_cols, ref["size0"]) if side == 1 else
                                  (ref["arg1"], tied_cols, tied_rows, ref["size1"]))
        assert not other.any()
        core = ref["scores"][:, :M, :N] if side == 1 else ref["scores"][:, :M, :N].transpose(1, 2)
        ntied = 0
        for b in range(B):
            pairs = {j: jj for s, bb, j, jj in c["dup"] if bb == b}
            assert not set(arg[b].tolist()) & set(pairs.values()), "the higher index of a duplicate pair won an arg-max"
            for i in range(arg.shape[1]):
                j = int(arg[b, i])
                assert bool(tied[b, i]) == (j in pairs), (b, i, j)
                if j in pairs:
                    assert int(size[b, i]) == 2
                    assert abs(float(core[b, i, j] - core[b, i, pairs[j]])) <= C.TIE_EPS
                    ntied += 1
        assert ntied >= len(c["dup"]), "every planted pair must decide at least one arg-max"
        tiles = [(j // 128, jj // 128) for _, _, j, jj in c["dup"]]
        assert any(a == b for a, b in tiles) and any(a != b and b < 2 for a, b in tiles) and any(b == 2 for _, b in tiles)
        # expected behaviour: the lower index takes the match, the higher gets -1 / score 0
        mm, ms = (ref["m1"], ref["ms1"]) if side == 1 else (ref["m0"], ref["ms0"])
        for _, b, j, jj in c["dup"]:
            assert int(mm[b, jj]) == -1 and float(ms[b, jj]) == 0.0 and int(mm[b, j]) > -1
    # ---- gap condition
    lg0, lg1 = C.low_gap(ref)
    share = (int(lg0.sum()) + int(lg1.sum())) / (B * (M + N))
    print(f"[low gap] {name}: {int(lg0.sum())} rows + {int(lg1.sum())} columns of {B * (M + N)} = {share:.4f}")
    assert share <= 0.01, (name, share)
    # ---- match-rich / no match
    nvalid = int((ref["m0"] > -1).sum())
    if c.get("rich"):
        assert nvalid > B * min(M, N) / 8, (name, nvalid)
    if c.get("none"):
        assert nvalid == 0 and int((ref["m1"] > -1).sum()) == 0 and (ref["ms0"] > 0).any()
    # ---- thresholds: no score within 1e-4 (relative) of it; at threshold 0 no mutual score that fp32 expf could flush to zero
    ms0 = ref["ms0"]
    assert not ((ms0 - th).abs() <= 1e-4 * th).any() if th > 0 else True
    mutual = ms0 > 0
    if th == 0.0:
        assert (torch.log(ms0[mutual]) > -80).all() and nvalid == int(mutual.sum())
    if name == "empty_middle":
        per = [(int((ref["m0"][b] > -1).sum())) for b in range(B)]
        assert per[1] == 0 and per[0] > 0 and per[2] > 0, per
    if name == "filter_1100":
        for b in range(B):
            rows = torch.where(ref["m0"][b] > -1)[0]
            assert (rows < 1024).sum() > 50 and (rows >= 1024).sum() > 20, "matches on both sides of the filter's second round"
    if name == "unscaled":
        assert ref["ms0"].max() > 0.9, "the peaked regime: matching scores near 1"
