"""GPU: the dense-match aggregation (csrc/dense_agg.hip through gim_amd/dense_sfm.py) against gim_amd.hloc_formats, the host
restatement of hloc/match_dense.py, on the scenarios of tests/dense_agg_cases.py.  The oracle alone says which cells, points and
matches it cannot decide (fp32 sums in arrival order there, exact integer sums here); tests/test_dense_agg_cpu.py pins their shares
below 1 %.  Everything else must agree exactly; scores within votes * 2^-24 relative, and exactly where fp32 sums are exact."""
import functools

import numpy as np
import pytest
import torch

import dense_agg_cases as C
from gim_amd import hloc_formats as H

pytestmark = pytest.mark.gpu

BIG = 100000                                            # a max_kps beyond every cell count
SCENARIOS = "ABCDE"


def _run(name, max_kps, reverse=False, max_error=C.MAX_ERROR, cell_size=C.CELL):
    from gim_amd.dense_sfm import DenseMatchAggregator
    images, pairs = C.scenario(name)
    agg = DenseMatchAggregator(max_error=max_error, cell_size=cell_size, device="cuda", capacity_matches=256)
    for n, (w, h) in images.items():
        agg.add_image(n, w, h)
    for n0, n1, k0, k1, sc in (pairs[::-1] if reverse else pairs):
        agg.add_pair(n0, n1, torch.from_numpy(k0).cuda(), torch.from_numpy(k1).cuda(), torch.from_numpy(sc).cuda())
    return agg, agg.finalize(max_kps)


@functools.lru_cache(maxsize=None)
def run(name, max_kps):
    return _run(name, max_kps)


@pytest.mark.parametrize("mode", ["all", "top", "big"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_keypoints_match_the_oracle(name, mode):
    max_kps = {"all": None, "top": C.MAX_KPS[name], "big": BIG}[mode]
    agg, final = run(name, max_kps)
    o = C.oracle(name)
    for n, (w, h) in o.images.items():
        kps, score = final[n]
        cells = [tuple(c) for c in agg.cells(n).tolist()]
        _, _, want_cells, band = o.top(n, max_kps)
        assert kps.dtype == np.float32 and score.dtype == np.float64 and kps.shape == (len(cells), 2) and score.shape == (len(cells),)
        assert len(set(cells)) == len(cells)
        assert set(cells) - band == set(want_cells) - band
        if not band:
            assert len(cells) == (len(o.cells[n]) if not max_kps else min(max_kps, len(o.cells[n])))
        for c, kp, s in zip(cells, kps, score):
            want_kp, want_s, votes, _ = o.cells[n][c]
            if c not in o.undecidable[n]:
                assert np.array_equal(kp, want_kp), (n, c, kp, want_kp)
            assert abs(s - want_s) <= votes * 2.0 ** -24 * want_s, (n, c, s, want_s, votes)
            if name == "E":
                assert s == want_s
        # the documented id order
        gw = w // C.PATCH + 2
        raster = np.array([cy * gw + cx for cx, cy in cells], dtype=np.int64)
        if not max_kps:
            assert np.all(np.diff(raster) > 0)
        else:
            d = np.diff(score)
            assert np.all(d <= 0) and np.all(np.diff(raster)[d == 0] > 0)
    if name == "D":
        assert agg.dropped() == C.D_DROPPED


@pytest.mark.parametrize("mode", ["all", "top"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_assignment_matches_the_oracle(name, mode):
    max_kps = None if mode == "all" else C.MAX_KPS[name]
    agg, _ = run(name, max_kps)
    exp = C.expected_matches(name, max_kps)
    out = list(agg.assign())
    assert len(out) == len(exp) == len(agg.pairs)
    skipped = 0
    for (n0, n1), (m0, s16), e in zip(agg.pairs, out, exp):
        assert m0.dtype == np.int32 and s16.dtype == np.float16 and m0.shape == s16.shape and m0.ndim == 1
        c0, c1 = agg.cells(n0), agg.cells(n1)
        assert len(m0) <= len(c0) and (len(m0) == 0 or m0[-1] >= 0)             # the row ends at the last matched id0
        assert np.all(m0 >= -1) and np.all(m0 < max(len(c1), 1)) and np.all(s16[m0 < 0] == 0)
        got = {tuple(c0[i]): (tuple(c1[m0[i]]), s16[i]) for i in np.flatnonzero(m0 >= 0)}
        partners = [v[0] for v in got.values()]
        assert len(set(partners)) == len(partners)                                # one-to-one
        if not e["match"] and not e["und0"]:
            assert len(m0) == 0
        for c in set(got) | set(e["match"]):
            a, b = got.get(c), e["match"].get(c)
            if a is not None and b is not None and a[0] == b[0] and a[1].view(np.uint16) == b[1].view(np.uint16):
                continue
            if c in e["und0"] or (a is not None and a[0] in e["und1"]) or (b is not None and b[0] in e["und1"]):
                skipped += 1
                continue
            raise AssertionError((name, mode, n0, n1, c, a, b))
    total = sum(int(k.sum()) for k in C.oracle(name).keep)
    print(f"scenario {name} {mode}: {skipped} matches0 entries left out of {total} dense matches")
    assert skipped <= C.CAP * total


def test_empty_pairs_give_empty_arrays():
    agg, _ = run("D", None)
    m0, s16 = list(agg.assign())[1]
    assert agg.pairs[1] == ("a", "c") and m0.shape == (0,) and s16.shape == (0,) and m0.dtype == np.int32 and s16.dtype == np.float16


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("name", ["A", "D"])
def test_order_and_launch_shape_do_not_matter(name):
    max_kps = C.MAX_KPS[name]
    agg, final = run(name, max_kps)
    again, final2 = _run(name, max_kps)
    rev, final3 = _run(name, max_kps, reverse=True)
    for n in final:
        for other, ag in ((final2, again), (final3, rev)):
            assert np.array_equal(final[n][0], other[n][0]) and np.array_equal(final[n][1], other[n][1])
            assert np.array_equal(agg.cells(n), ag.cells(n))
    one, every, second = list(agg.assign(batch_pairs=1)), list(agg.assign(batch_pairs=len(agg.pairs))), list(again.assign(batch_pairs=2))
    assert len(one) == len(every) == len(second) == len(agg.pairs)
    for a, b, c in zip(one, every, second):
        assert _same(a, b) and _same(a, c)
    # the pairs arrived the other way round: the same matches, pair by pair
    back = list(rev.assign())[::-1]
    for a, b in zip(one, back):
        assert _same(a, b)


def test_one_vote_launch_over_a_ragged_batch_gives_the_same_sums():
    """gim_agg_vote with all pairs of D in one launch (empty pairs in the offsets) against the sums of one launch per pair"""
    from gim_amd import ops
    agg, _ = run("D", None)
    st = agg._state()
    fresh = st._replace(votes=torch.zeros_like(st.votes), cell_n=torch.zeros_like(st.cell_n))
    s0, s1 = zip(*agg.pair_slots)
    dropped = ops.agg_vote(fresh, ops.agg_batch(agg.offsets, s0, s1, len(agg.sizes), st.scores.shape[0], "cuda"))
    assert torch.equal(fresh.votes, st.votes) and torch.equal(fresh.cell_n, st.cell_n) and dropped.tolist() == C.D_DROPPED
    assert int(st.cell_n.sum()) == 2 * sum(int(k.sum()) for k in C.oracle("D").keep)


def test_odd_bin_ratio_against_the_oracle():
    """cell_size 6, max_error 2: r = 3 is odd, a cell has 5 x 5 bins and its outermost ones lie in the neighbour's range"""
    images, pairs = C.scenario("B")
    agg, final = _run("B", None, cell_size=6)
    host = {n: H.ImageKeypoints() for n in images}
    votes = {n: {} for n in images}
    for n0, n1, k0, k1, sc in pairs:
        for n, k in ((n0, k0), (n1, k1)):
            for i in host[n].add(k, sc, 2, 6):
                votes[n][int(i)] = votes[n].get(int(i), 0) + 1
    for n in images:
        kps, score = host[n].finalize()
        cell = {kid: tuple(np.rint((np.array(cp, dtype=np.float32) + np.float32(0.5)) / np.float32(6)).astype(int)) for cp, kid in host[n].cells.items()}
        want = {cell[k]: (kps[k], score[k], votes[n][k], sorted(host[n].votes[k].values(), reverse=True)) for k in range(len(kps))}
        got_cells = [tuple(c) for c in agg.cells(n).tolist()]
        assert set(got_cells) == set(want)
        for c, kp, s in zip(got_cells, *final[n]):
            wkp, ws, m, sums = want[c]
            sums = [float(v) for v in sums] + [0.0]
            if sums[0] - sums[1] > 2 * m * 2.0 ** -24 * sums[0] + m * 2.0 ** -32:
                assert np.array_equal(kp, wkp), (n, c, kp, wkp)
            assert abs(s - ws) <= m * 2.0 ** -24 * ws


class _FakeH5(dict):
    """the slice of h5py's group protocol the writers use"""

    def create_group(self, name):
        self[name] = _FakeH5()
        return self[name]

    def create_dataset(self, name, data):
        self[name] = np.asarray(data)


class _Recorded:
    """a matcher with the plugins' dict contract that returns recorded device tensors"""

    def __init__(self, pairs):
        self.table = {(n0, n1): tuple(torch.from_numpy(a).cuda() for a in (k0, k1, sc)) for n0, n1, k0, k1, sc in pairs}

    def __call__(self, data):
        assert data["image0"].is_cuda and data["image1"].is_cuda
        k0, k1, sc = self.table[(data["name0"], data["name1"])]
        return {"keypoints0": k0, "keypoints1": k1, "scores": sc}


@pytest.mark.parametrize("through_plugin", [False, True])
def test_pair_list_ends_in_hlocs_datasets(through_plugin):
    from gim_amd.dense_sfm import DenseMatchAggregator, match_dense_pair_list
    images, pairs = C.scenario("B")
    tensors = {n: torch.zeros(1, 3, h, w, device="cuda") for n, (w, h) in images.items()}
    names = [(p[0], p[1]) for p in pairs]
    ffd, mfd = _FakeH5(), _FakeH5()
    if through_plugin:
        from gim_amd.hloc_matchers.gim_dkm_hip import GimDkmHip
        agg = GimDkmHip.match_and_assign_from_images(_Recorded(pairs), tensors, names, ffd, mfd, max_kps=C.MAX_KPS["B"])
    else:
        agg = DenseMatchAggregator(device="cuda")
        assert match_dense_pair_list(_Recorded(pairs), tensors, names, agg) is None
        agg.finalize(C.MAX_KPS["B"])
        agg.write(ffd, mfd, write_dense=True)
    # the driver's k + 0.5 - 0.5 (match_dense.py:242-243 with a scale of 1) rounds a few coordinates by an ulp before they vote: the
    # same points, rounded on the host, through add_pair
    ref = DenseMatchAggregator(device="cuda")
    for n, (w, h) in images.items():
        ref.add_image(n, w, h)
    for n0, n1, k0, k1, sc in pairs:
        ref.add_pair(n0, n1, *(torch.from_numpy(a).cuda() for a in ((k0 + np.float32(0.5)) - np.float32(0.5), (k1 + np.float32(0.5)) - np.float32(0.5), sc)))
    ref_final = ref.finalize(C.MAX_KPS["B"])
    assert set(ffd) == set(images)
    for n in images:
        assert ffd[n]["keypoints"].dtype == np.float32 and ffd[n]["keypoints"].shape == (C.MAX_KPS["B"], 2)
        assert ffd[n]["score"].shape == (C.MAX_KPS["B"],)
        assert np.array_equal(ffd[n]["keypoints"], ref_final[n][0]) and np.array_equal(ffd[n]["score"], ref_final[n][1])
        assert np.array_equal(agg.cells(n), ref.cells(n))
    assert set(mfd) == {H.pair_key(*p) for p in names}
    for (n0, n1, k0, k1, sc), (m0, s16) in zip(pairs, agg.assign()):
        g = mfd[H.pair_key(n0, n1)]
        assert set(g) == {"keypoints0", "keypoints1", "scores", "matches0", "matching_scores0"}
        assert g["matches0"].dtype == np.int32 and g["matching_scores0"].dtype == np.float16 and g["matches0"].shape == g["matching_scores0"].shape
        assert np.array_equal(g["matches0"], m0) and np.array_equal(g["matching_scores0"], s16) and 0 < len(m0) <= C.MAX_KPS["B"]
        assert g["keypoints0"].dtype == g["keypoints1"].dtype == g["scores"].dtype == np.float32
        assert np.array_equal(g["keypoints0"], (k0 + np.float32(0.5)) - np.float32(0.5)) and np.array_equal(g["scores"], sc)
        assert g["keypoints1"].shape == (len(sc), 2)
    # without the dense datasets: the match groups hold the two keypoint-indexed datasets only
    mfd2 = _FakeH5()
    agg.write(_FakeH5(), mfd2, write_dense=False)
    assert all(set(g) == {"matches0", "matching_scores0"} for g in mfd2.values()) and set(mfd2) == set(mfd)
