"""CPU tests of the dense-match aggregation (csrc/dense_agg.hip, gim_amd/dense_sfm.py): the exports and their signatures against the
header, the host-side argument checks, the resources of the new kernels, the aggregator's bookkeeping with the launches stubbed, the
rescale of `match_dense_pair_list`, and -- from the oracle alone -- that every scenario of tests/dense_agg_cases.py keeps the 1 % caps on
what the GPU tests may leave out."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import dense_agg_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_feature_bank_resources", os.path.join(ROOT, "tests", "test_feature_bank_resources_cpu.py"))
_fb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_fb)

NEW = ["gim_agg_bins", "gim_agg_vote", "gim_agg_finalize", "gim_agg_keypoints", "gim_agg_assign_ws_bytes", "gim_agg_assign"]

# (undecidable cells, points, matches) as the oracle gives them, per scenario and max_kps (None = every cell; the points of the
# re-assignment exist only with max_kps)
SHARES = {
    ("A", None): (0.00000, 0.00000, 0.00000), ("A", 200): (0.00000, 0.00083, 0.00056),
    ("B", None): (0.00000, 0.00000, 0.00000), ("B", 100): (0.00000, 0.00625, 0.00667),
    ("C", None): (0.00000, 0.00000, 0.00000), ("C", 200): (0.00000, 0.00639, 0.00611),
    ("D", None): (0.00000, 0.00000, 0.00000), ("D", 200): (0.00000, 0.00632, 0.00702),
    ("E", None): (0.00000, 0.00000, 0.00083), ("E", 100): (0.00000, 0.00000, 0.00000),
}


@pytest.mark.parametrize("name,max_kps", list(SHARES), ids=str)
def test_scenarios_keep_the_undecidable_caps(name, max_kps):
    cells, points, matches = C.shares(name, max_kps)
    o = C.oracle(name)
    dup = 0
    for n in o.images:
        kps = o.top(n, max_kps)[0]
        dup += len(kps) - len({tuple(k) for k in kps.tolist()})
    print(f"scenario {name} max_kps={max_kps}: undecidable cells {cells:.5f} points {points:.5f} matches {matches:.5f}; "
          f"{dup} duplicate final keypoint positions")
    assert max(cells, points, matches) <= C.CAP
    want = SHARES[(name, max_kps)]
    assert abs(cells - want[0]) < 5e-6 and abs(points - want[1]) < 5e-6 and abs(matches - want[2]) < 5e-6, (cells, points, matches)
    assert C.shares(name, 100000)[0] == 0.0                           # a max_kps beyond the cell count: the keypoint tests use it too
    if name == "D":
        assert [int((~k).sum()) for k in o.keep] == C.D_DROPPED
        assert [len(p[4]) for p in o.pairs] == [322, 0, 1, 150, 250] and set(o.images) == {"a", "b", "c", "d"}


@pytest.mark.parametrize("name", NEW)
def test_exports_have_the_headers_signature(name):
    from gim_amd import _lib
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib, name)                       # AttributeError: the symbol is missing from the library
    res, args = _fb._header_prototype(name)
    assert (res, args) == _lib.PROTOTYPES[name], (res, args, _lib.PROTOTYPES[name])
    assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.lib.gim_version() == _lib.ABI_VERSION == 115          # added exports: they moved no ABI revision


def _err():
    from gim_amd import _lib
    return _lib.lib.gim_last_error()


def test_host_argument_checks_need_no_gpu():
    from gim_amd import _lib
    L = _lib.lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    odd2 = ctypes.c_void_p(p.value + 2)
    # the geometry, shared by every entry point
    assert L.gim_agg_bins(2.0, 8) == 25 and L.gim_agg_bins(2.5, 8) == 25 and L.gim_agg_bins(3.0, 9) == 25 and L.gim_agg_bins(1.0, 8) == 81
    assert L.gim_agg_bins(2.0, 4) == 9 and L.gim_agg_bins(2.0, 6) == 25          # r = 2; r = 3 is odd: h = 2, five bins per axis
    assert L.gim_agg_bins(2.0, 7) == 0 and b"must be an integer in 1..8" in _err()
    assert L.gim_agg_bins(1.0, 9) == 0 and b"must be an integer in 1..8" in _err()
    assert L.gim_agg_bins(3.0, 3) == 0 and b"max_error=3 > patch / 2" in _err()
    assert L.gim_agg_bins(2.5, 4) == 0 and b"> patch / 2" in _err()
    assert L.gim_agg_bins(0.5, 8) == 0 and b"max_error=0.5" in _err()
    assert L.gim_agg_bins(float("nan"), 8) == 0 and L.gim_agg_bins(2.0, 0) == 0 and L.gim_agg_bins(2.0, -8) == 0

    # gim_agg_vote(kpts0, kpts1, scores, offsets, slot0, slot1, geom, votes, cell_n, dropped, P, row_lo, row_hi, pool_rows, n_slots,
    #              total_cells, max_error, patch, stream)
    def vote(k0=p, sc=p, off=p, votes=p, dropped=p, P=1, lo=0, hi=4, pool=8, S=2, cells=100, me=2.0, patch=8):
        return L.gim_agg_vote(k0, p, sc, off, p, p, p, votes, p, dropped, P, lo, hi, pool, S, cells, me, patch, None)
    assert vote(me=2.0, patch=7) != 0 and b"1..8" in _err()
    assert vote(me=5.0, patch=5) != 0 and b"patch / 2" in _err()
    assert vote(P=-1) != 0 and b"P=-1" in _err()
    assert vote(S=0) != 0 and b"n_slots=0" in _err()
    assert vote(cells=-1) != 0 and b"total_cells=-1" in _err()
    assert vote(cells=1 << 31) != 0 and b"int32 cell indices" in _err()
    assert vote(lo=-1) != 0 and b"rows [-1, 4)" in _err()
    assert vote(lo=5, hi=4) != 0 and b"rows [5, 4)" in _err()
    assert vote(hi=9) != 0 and b"of a pool of 8" in _err()
    assert vote(k0=None) != 0 and b"NULL" in _err()
    assert vote(off=None) != 0 and b"NULL" in _err()
    assert vote(dropped=None) != 0 and b"NULL" in _err()
    assert vote(k0=odd) != 0 and b"8-byte aligned" in _err()
    assert vote(votes=odd) != 0 and b"8-byte aligned" in _err()
    assert vote(sc=odd2) != 0 and b"misaligned" in _err()
    assert vote(P=0) == 0                                             # an empty batch: nothing to do, no launch

    # gim_agg_finalize(votes, cell_n, total_cells, max_error, patch, cell_key, cell_bin, stream)
    assert L.gim_agg_finalize(p, p, 0, 2.0, 8, p, p, None) == 0
    assert L.gim_agg_finalize(p, p, -1, 2.0, 8, p, p, None) != 0 and b"total_cells=-1" in _err()
    assert L.gim_agg_finalize(None, p, 10, 2.0, 8, p, p, None) != 0 and b"NULL" in _err()
    assert L.gim_agg_finalize(p, p, 10, 2.0, 8, odd, p, None) != 0 and b"aligned" in _err()
    assert L.gim_agg_finalize(p, p, 10, 2.0, 3, p, p, None) != 0 and b"1..8" in _err()

    # gim_agg_keypoints(votes, cell_bin, geom, sel, sel_slot, kp_off, n_sel, n_slots, total_cells, max_error, patch, id_grid, keypoints,
    #                   score, cells, stream)
    def kps(votes=p, grid=p, n_sel=4, S=2, cells=100, score=p, patch=8):
        return L.gim_agg_keypoints(votes, p, p, p, p, p, n_sel, S, cells, 2.0, patch, grid, p, score, p, None)
    assert kps(n_sel=-1) != 0 and b"n_sel=-1" in _err()
    assert kps(S=0) != 0 and b"n_slots=0" in _err()
    assert kps(grid=None) != 0 and b"id_grid" in _err()
    assert kps(grid=odd2) != 0 and b"id_grid" in _err()
    assert kps(patch=5) != 0 and b"1..8" in _err()
    assert kps(cells=0) == 0

    # gim_agg_assign(kpts0, kpts1, scores, offsets, slot0, slot1, geom, id_grid, keypoints, kp_off, koff0, koff1, P, row_lo, row_hi,
    #                pool_rows, n_slots, total_cells, n_kp, rows0, rows1, max_error, patch, nearest, matches0, scores_f16, row_len, ws, stream)
    def assign(k0=p, off=p, P=1, lo=0, hi=4, pool=8, S=2, n_kp=5, rows0=5, rows1=5, me=2.0, patch=8, m0=p, s16=p, ln=p, ws=p):
        return L.gim_agg_assign(k0, p, p, off, p, p, p, p, p, p, p, p, P, lo, hi, pool, S, 100, n_kp, rows0, rows1, me, patch, 1, m0, s16, ln,
                                ws, None)
    assert assign(me=3.0, patch=3) != 0 and b"patch / 2" in _err()
    assert assign(P=-2) != 0 and b"P=-2" in _err()
    assert assign(hi=9) != 0 and b"of a pool of 8" in _err()
    assert assign(S=-1) != 0 and b"n_slots=-1" in _err()
    assert assign(n_kp=-1) != 0 and b"n_kp=-1" in _err()
    assert assign(rows0=-1) != 0 and b"rows0=-1" in _err()
    assert assign(off=None) != 0 and b"NULL" in _err()
    assert assign(ln=None) != 0 and b"NULL" in _err()
    assert assign(m0=None) != 0 and b"NULL output rows" in _err()
    assert assign(k0=None) != 0 and b"NULL" in _err()
    assert assign(ws=None) != 0 and b"NULL" in _err()
    assert assign(k0=odd) != 0 and b"8-byte aligned" in _err()
    assert assign(ws=odd) != 0 and b"8-byte aligned" in _err()
    assert assign(s16=ctypes.c_void_p(p.value + 1)) != 0 and b"misaligned" in _err()
    assert assign(P=0) == 0
    f = L.gim_agg_assign_ws_bytes
    assert f(-1, 1, 1) == 0 and f(0, 0, 0) == 0 and f(8192, 100, 200) == 8 * 300 + 8 * 8192


def test_new_kernels_target_gfx950_without_scratch():
    ks = _fb._kr._kernels()          # asserts the gfx950 target of every code object it parses
    for name in ("agg_vote_kernel(", "agg_finalize_kernel(", "agg_keypoints_kernel(", "agg_ids_kernel(", "agg_emit_kernel("):
        hit = [(n, v) for n, v in ks.items() if name in n]
        assert hit, f"{name} not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
            assert regs <= 64, f"{n}: {regs} VGPRs"          # one match or one cell per lane: 8 waves per SIMD


class _StubLib:
    """the library with the launches stubbed (there is no device here): the geometry and size queries are the real ones"""

    def __init__(self, real):
        self.gim_agg_bins = real.gim_agg_bins
        self.gim_agg_assign_ws_bytes = real.gim_agg_assign_ws_bytes
        self.gim_last_error = real.gim_last_error
        self.calls = []

    def gim_agg_vote(self, *a):
        self.calls.append(("vote", a[10], a[11], a[12], a[13], a[14], a[15]))     # P, row_lo, row_hi, pool_rows, n_slots, total_cells
        return 0

    def gim_agg_finalize(self, *a):
        self.calls.append(("finalize", a[2]))
        ctypes.memset(a[5], 0, 8 * a[2])                                          # cell_key: no cell has votes
        return 0

    def gim_agg_keypoints(self, *a):
        self.calls.append(("keypoints", a[6], a[7], a[8]))
        return 0

    def gim_agg_assign(self, *a):
        self.calls.append(("assign", a[12], a[13], a[14], a[19], a[20], a[23]))   # P, row_lo, row_hi, rows0, rows1, nearest
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    from gim_amd import ops
    stub = _StubLib(ops.lib)
    monkeypatch.setattr(ops, "lib", stub)
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    return stub


def test_aggregator_bookkeeping(stubbed):
    from gim_amd._lib import GimHipError
    from gim_amd.dense_sfm import DenseMatchAggregator
    for me, cs, what in ((2, 7, "1..8"), (1, 9, "1..8"), (3, 3, "patch / 2"), (4.5, 8, "patch / 2"), (2, 8.5, "integer")):
        with pytest.raises(GimHipError, match=what):
            DenseMatchAggregator(max_error=me, cell_size=cs, device="cpu")
    agg = DenseMatchAggregator(device="cpu", capacity_matches=8)
    assert (agg.patch, agg.bins) == (8, 25) and len(agg) == 0
    assert agg.add_image("a", 160, 120) == 0 and agg.add_image("b", 100, 76) == 1 and agg.add_image("a", 160, 120) == 0
    assert agg.cell_off == [0, 22 * 17, 22 * 17 + 14 * 11] and "a" in agg and "c" not in agg
    with pytest.raises(GimHipError, match="resident with size"):
        agg.add_image("a", 161, 120)
    with pytest.raises(GimHipError, match="size 0 x 5"):
        agg.add_image("z", 0, 5)

    def pair(n):
        return torch.rand(n, 2), torch.rand(n, 2), torch.rand(n)
    with pytest.raises(GimHipError, match="'c' is unknown"):
        agg.add_pair("a", "c", *pair(3))
    with pytest.raises(GimHipError, match="kpts"):
        agg.add_pair("a", "b", torch.rand(3, 2), torch.rand(4, 2), torch.rand(3))
    assert not stubbed.calls and agg.pairs == []                      # refused before anything changed
    agg.add_pair("a", "b", *pair(5))
    agg.add_pair("b", "a", *pair(0))
    k0, k1, sc = pair(6)
    agg.add_pair("a", "a", k0.double(), k1, sc)                       # 11 rows: the pool of 8 doubles, the stored rows survive
    assert agg.offsets == [0, 5, 5, 11] and agg.pair_slots == [(0, 1), (1, 0), (0, 0)]
    cells = 22 * 17 + 14 * 11
    assert stubbed.calls == [("vote", 1, 0, 5, 8, 2, cells), ("vote", 1, 5, 5, 8, 2, cells), ("vote", 1, 5, 11, 16, 2, cells)]
    st = agg._state()
    assert st.scores.shape == (16,) and torch.equal(st.kpts0[5:11], k0) and torch.equal(st.scores[5:11], sc)
    assert st.votes.shape == (cells * 25,) and st.votes.dtype == torch.int64 and st.geom.tolist() == [[160, 120, 0, 0], [100, 76, 22 * 17, 0]]
    # an image that arrives after the first vote gets zeroed cells behind the others
    st.votes[3] = 7
    agg.add_image("c", 8, 8)
    st = agg._state()
    assert st.votes.shape == ((cells + 9) * 25,) and st.votes[3] == 7 and st.cell_n.shape == (cells + 9,) and st.geom.shape == (3, 4)
    with pytest.raises(GimHipError, match="finalize first"):
        list(agg.assign())
    with pytest.raises(GimHipError, match="max_kps=0"):
        agg.finalize(max_kps=0)
    out = agg.finalize(max_kps=50)
    assert stubbed.calls[-2:] == [("finalize", cells + 9), ("keypoints", 0, 3, cells + 9)] and set(out) == {"a", "b", "c"}
    with pytest.raises(GimHipError, match="add_pair after finalize"):
        agg.add_pair("a", "b", *pair(2))
    with pytest.raises(GimHipError, match="add_image after finalize"):
        agg.add_image("d", 8, 8)
    with pytest.raises(GimHipError, match="batch_pairs=0"):
        list(agg.assign(batch_pairs=0))
    # slots and offsets are checked on the host before a batch is uploaded
    from gim_amd import ops
    with pytest.raises(GimHipError, match="pair 1 names slot 3 outside"):
        ops.agg_batch([0, 2, 4], [0, 3], [1, 1], 3, 16, "cpu")
    with pytest.raises(GimHipError, match="pair 0 names slot -1 outside"):
        ops.agg_batch([0, 2], [0], [-1], 3, 16, "cpu")
    with pytest.raises(GimHipError, match="offsets must rise"):
        ops.agg_batch([0, 5, 4], [0, 1], [1, 1], 3, 16, "cpu")
    with pytest.raises(GimHipError, match="offsets must rise"):
        ops.agg_batch([0, 5, 17], [0, 1], [1, 1], 3, 16, "cpu")
    b = ops.agg_batch([2, 5, 5], [0, 1], [1, 2], 3, 16, "cpu")
    assert (b.P, b.row_lo, b.row_hi) == (2, 2, 5) and b.offsets.tolist() == [2, 5, 5] and b.slot0.tolist() == [0, 1] and b.slot1.tolist() == [1, 2]


class _StubMatcher:
    def __init__(self, table):
        self.table, self.seen = table, []

    def __call__(self, data):
        self.seen.append((data["name0"], data["name1"], tuple(data["image0"].shape), tuple(data["image1"].shape)))
        k0, k1, sc = self.table[(data["name0"], data["name1"])]
        return {"keypoints0": k0, "keypoints1": k1, "scores": sc}


def test_pair_list_driver_applies_the_reference_rescale(stubbed):
    """match_dense.py:242-243: scale_keypoints(k + 0.5, s) - 0.5 in fp32, the multiplication only where a scale is not 1"""
    from gim_amd._lib import GimHipError
    from gim_amd.dense_sfm import DenseMatchAggregator, match_dense_pair_list
    rng = np.random.default_rng(5)
    images = {"x": torch.zeros(1, 3, 48, 64), "y": torch.zeros(1, 3, 40, 56), "z": torch.zeros(1, 3, 48, 64)}
    scales = {"x": np.array([2.5, 2.25]), "y": np.array([1.0, 1.0])}                   # z: no entry = 1
    pairs = [("x", "y"), ("y", "z"), ("x", "z")]
    table = {p: (torch.from_numpy(rng.random((7, 2)).astype(np.float32) * 40), torch.from_numpy(rng.random((7, 2)).astype(np.float32) * 40),
                 torch.from_numpy(rng.random(7).astype(np.float32))) for p in pairs}
    agg = DenseMatchAggregator(device="cpu")
    m = _StubMatcher(table)
    assert match_dense_pair_list(m, images, pairs, agg, scales) is None
    assert agg.sizes == [(160, 108), (56, 40), (64, 48)] and agg.pairs == pairs
    assert m.seen == [("x", "y", (1, 3, 48, 64), (1, 3, 40, 56)), ("y", "z", (1, 3, 40, 56), (1, 3, 48, 64)), ("x", "z", (1, 3, 48, 64), (1, 3, 48, 64))]
    st = agg._state()
    for p, (n0, n1) in enumerate(pairs):
        for side, name in enumerate((n0, n1)):
            k = table[(n0, n1)][side].numpy() + np.float32(0.5)
            s = scales.get(name)
            if s is not None and np.any(s != 1.0):
                k = k * s.astype(np.float32)
            want = k - np.float32(0.5)
            assert want.dtype == np.float32
            assert np.array_equal(st[side][agg.offsets[p]:agg.offsets[p + 1]].numpy(), want)
        assert np.array_equal(st.scores[agg.offsets[p]:agg.offsets[p + 1]].numpy(), table[(n0, n1)][2].numpy())
    with pytest.raises(GimHipError, match="was not given"):
        match_dense_pair_list(m, images, [("x", "w")], DenseMatchAggregator(device="cpu"))


def test_plugin_has_the_pair_list_method():
    from gim_amd.hloc_matchers.gim_dkm_hip import GimDkmHip
    import inspect
    sig = inspect.signature(GimDkmHip.match_and_assign_from_images)
    assert list(sig.parameters)[:6] == ["self", "images", "pairs", "features", "matches", "max_kps"] and sig.parameters["max_kps"].default == 8192
