"""CPU tests of root_sift over a pair list (gim_nn_bank_put, gim_nn_match_pairs_plan, gim_nn_match_pairs, `DescriptorBank`): the exports and
their signatures against the header, the host-side argument checks, the linear workspace, the resources of the new kernels, the bank's
bookkeeping with the launches stubbed, the host-built work table on a hand-written ragged batch, and -- from the oracle alone -- the
condition under which the GPU parity test speaks (tests/nn_match_pairs_cases.py keeps the 2 % cap on undecidable rows)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import nn_match_oracle as O
import nn_match_pairs_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_feature_bank_resources", os.path.join(ROOT, "tests", "test_feature_bank_resources_cpu.py"))
_fb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_fb)

NEW = ["gim_nn_bank_put", "gim_nn_match_pairs_plan", "gim_nn_match_pairs_ws_bytes", "gim_nn_match_pairs"]

# pooled undecidable shares of the GPU parity test's banks, (ratio 0.8, ratio 0.0), as the oracle gives them
SHARES = {("A", True): (0.0071, 0.0053), ("A", False): (0.0173, 0.0169), ("B", True): (0.0015, 0.0007), ("B", False): (0.0149, 0.0112),
          ("C", True): (0.0064, 0.0038), ("C", False): (0.0229, 0.0229)}
POOLED_ROWS = {"A": 2254, "B": 1340, "C": 786}


@pytest.mark.parametrize("name,rootsift", list(SHARES), ids=str)
def test_banks_keep_the_undecidable_cap(name, rootsift):
    """the inputs, not the kernel, keep the cap on the pooled rows of every list the GPU oracle test runs; bank C without rootsift is over
    it (0.0229) and is therefore left to the bit-identity test alone"""
    for ratio, want in zip((0.8, 0.0), SHARES[(name, rootsift)]):
        f = C.pooled_oracle(name, rootsift, ratio)
        pool = f["pool"]
        assert int(pool.sum()) == POOLED_ROWS[name]
        und = 1.0 - f["decidable"][pool].float().mean().item()
        matched = (f["match0"][pool] >= 0).float().mean().item()
        print(f"bank {name} rootsift={rootsift} ratio={ratio}: undecidable {und:.4f} matched {matched:.3f}")
        assert abs(und - want) < 5e-5
        assert (und <= O.UNDECIDABLE_CAP) == ((name, rootsift) != ("C", False))
        assert 0.29 <= matched <= 0.53
    assert [d.shape[0] for d in C.images("A")] == [257, 130, 300, 1, 0, 65]
    assert [d.shape[0] for d in C.images("B")] == [300, 300, 70] and [d.shape[0] for d in C.images("C")] == [129, 64, 200]


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
    # gim_nn_bank_put(desc, n, D, rootsift, slot, bank_desc, bank_n, n_slots, max_rows, stream)
    for D in (8, 24, 272):
        assert L.gim_nn_bank_put(p, 4, D, 1, 0, p, p, 2, 8, None) != 0 and b"D=" in _err()
    assert L.gim_nn_bank_put(p, 4, 128, 1, 2, p, p, 2, 8, None) != 0 and b"slot 2" in _err()
    assert L.gim_nn_bank_put(p, 4, 128, 1, -1, p, p, 2, 8, None) != 0 and b"slot -1" in _err()
    assert L.gim_nn_bank_put(p, 9, 128, 1, 0, p, p, 2, 8, None) != 0 and b"max_rows=8" in _err()
    assert L.gim_nn_bank_put(p, -1, 128, 1, 0, p, p, 2, 8, None) != 0 and b"n=-1" in _err()
    assert L.gim_nn_bank_put(None, 4, 128, 1, 0, p, p, 2, 8, None) != 0 and b"NULL" in _err()
    assert L.gim_nn_bank_put(p, 4, 128, 1, 0, None, p, 2, 8, None) != 0 and b"NULL" in _err()
    assert L.gim_nn_bank_put(odd, 4, 128, 1, 0, p, p, 2, 8, None) != 0 and b"aligned" in _err()
    # gim_nn_match_pairs(bank_desc, bank_n, idx0, idx1, row_off, col_off, work, P, n_work, nsplit, rows0, rows1, n_slots, max_rows, D, ratio,
    #                    match0, score0, count, hloc, matches0_i16, scores_f16, ws, stream)
    def mp(bank=p, work=p, P=2, n_work=3, nsplit=4, rows0=10, rows1=10, n_slots=2, max_rows=8, D=128, match0=p, hloc=0, m16=None, ws=p):
        return L.gim_nn_match_pairs(bank, p, p, p, p, p, work, P, n_work, nsplit, rows0, rows1, n_slots, max_rows, D, 0.8, match0, p, p, hloc,
                                    m16, m16, ws, None)
    for D in (8, 24, 272):
        assert mp(D=D) != 0 and b"D=" in _err()
    assert mp(P=-1) != 0 and b"P=-1" in _err()
    assert mp(rows0=-5) != 0 and b"rows0=-5" in _err()
    assert mp(nsplit=0) != 0 and b"nsplit=0" in _err()
    assert mp(nsplit=17) != 0 and b"nsplit=17" in _err()
    assert mp(max_rows=32768, hloc=1, m16=p) != 0 and b"int16" in _err()
    assert mp(bank=None) != 0 and b"NULL" in _err()
    assert mp(work=None) != 0 and b"NULL work" in _err()
    assert mp(match0=None) != 0 and b"NULL" in _err()
    assert mp(hloc=1) != 0 and b"hloc" in _err()
    assert mp(bank=odd) != 0 and b"aligned" in _err()
    assert mp(ws=odd) != 0 and b"aligned" in _err()
    assert mp(rows1=0) != 0 and b"work items" in _err()
    assert mp(P=0) == 0                                               # an empty list: nothing to do, no launch
    # gim_nn_match_pairs_plan: slot range on the host table
    i0, i1, n = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int32 * 2)(1, 2), (ctypes.c_int32 * 2)(5, 7)
    ro, co, nw, ns = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int32(), ctypes.c_int32()
    a = ctypes.addressof
    assert L.gim_nn_match_pairs_plan(a(i0), a(i1), a(n), 2, 2, a(ro), a(co), None, 0, a(nw), a(ns)) != 0
    assert b"pair 1 names slot (1, 2) outside [0, 2)" in _err()
    i1[1] = 0
    assert L.gim_nn_match_pairs_plan(a(i0), a(i1), a(n), 2, 2, None, a(co), None, 0, a(nw), a(ns)) != 0 and b"NULL" in _err()
    n[0] = -3
    assert L.gim_nn_match_pairs_plan(a(i0), a(i1), a(n), 2, 2, a(ro), a(co), None, 0, a(nw), a(ns)) != 0 and b"negative count" in _err()
    n[0] = 5
    assert L.gim_nn_match_pairs_plan(a(i0), a(i1), a(n), 2, 2, a(ro), a(co), None, 0, a(nw), a(ns)) == 0
    assert list(ro) == [0, 5, 12] and list(co) == [0, 7, 12] and nw.value == 2 and ns.value == 16
    small = (ctypes.c_int32 * 4)()
    assert L.gim_nn_match_pairs_plan(a(i0), a(i1), a(n), 2, 2, a(ro), a(co), a(small), 1, a(nw), a(ns)) != 0 and b"work table" in _err()


def test_workspace_is_linear_in_the_rows_of_the_batch():
    from gim_amd import _lib
    f = _lib.lib.gim_nn_match_pairs_ws_bytes
    assert f(-1, 4) == 0 and f(0, 0) == 0
    for P, n in ((32, 2048), (32, 4800), (8, 1000), (1, 257)):
        rows = P * n
        ws = f(rows, rows)
        # the column maxima + 16 column splits x 3 row statistics, 4 bytes each, four aligned pieces
        assert 0 < ws <= 4 * (rows + 3 * 16 * rows) + 4 * 256
        assert f(2 * rows, 2 * rows) <= 2 * ws + 4 * 256              # doubling every count at most doubles it, plus alignment
        assert ws * 16 < P * n * n * 4 or n < 1024                    # far below the similarity matrices of the batch
    assert f(32 * 4800, 32 * 4800) * 90 < 32 * 4800 * 4800 * 4


def test_new_kernels_target_gfx950_without_scratch():
    ks = _fb._kr._kernels()          # asserts the gfx950 target of every code object it parses
    for name in ("nn_bank_put_kernel(", "nn_reset_pairs_kernel(", "nn_sweep_pairs_kernel<32>(", "nn_sweep_pairs_kernel<16>(",
                 "nn_final_pairs_kernel("):
        hit = [(n, v) for n, v in ks.items() if name in n]
        assert hit, f"{name} not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
            # the sweep runs 8 waves per workgroup, two per SIMD: 256 registers each; the others are one thread per row or piece
            assert regs <= (128 if "sweep" in n else 64), f"{n}: {regs} VGPRs"
    # the pair-list sweep is the single-pair tile: the same registers
    for kc in ("<32>(", "<16>("):
        one = [v for n, v in ks.items() if "nn_sweep_kernel" + kc in n]
        many = [v for n, v in ks.items() if "nn_sweep_pairs_kernel" + kc in n]
        assert one and many and abs(one[0][0] - many[0][0]) <= 8


def test_plan_of_a_hand_written_ragged_batch():
    """counts [257, 130, 0, 1]; pairs (0,1) (1,0) (0,2) (2,0) (3,0) (0,3).  Nine row blocks in all (3 + 2 + 0 + 0 + 1 + 3), so the split is
    512 // 9 = 56 -> the cap, 16, and every pair uses min(16, its column tiles):
      (0,1): 3 row blocks x 3 tiles of 130 columns          (1,0): 2 row blocks x 5 tiles of 257 columns
      (0,2), (2,0): an empty side, no item                  (3,0): 1 row block x 5 tiles      (0,3): 3 row blocks x 1 tile"""
    from gim_amd import ops
    pl = ops.nn_pairs_plan([0, 1, 0, 2, 3, 0], [1, 0, 2, 0, 0, 3], [257, 130, 0, 1])
    assert pl.row_off.tolist() == [0, 257, 387, 644, 644, 645, 902]
    assert pl.col_off.tolist() == [0, 130, 387, 387, 644, 901, 902]
    assert pl.nsplit == 16
    want = [(0, b, t, t + 1) for b in range(3) for t in range(3)] + [(1, b, t, t + 1) for b in range(2) for t in range(5)] + \
           [(4, 0, t, t + 1) for t in range(5)] + [(5, b, 0, 1) for b in range(3)]
    assert [tuple(w) for w in pl.work.tolist()] == want
    assert pl.row_off.dtype == pl.col_off.dtype == pl.work.dtype == pl.idx0.dtype == np.int32
    # many row blocks: the split comes from the TOTAL, 512 // 300 = 1 -> one item per row block, the whole column range
    big = ops.nn_pairs_plan([0] * 30, [1] * 30, [1280, 1000])
    assert big.nsplit == 1 and big.work.shape == (300, 4)
    assert [tuple(w) for w in big.work[:11].tolist()] == [(0, b, 0, 16) for b in range(10)] + [(1, 0, 0, 16)]
    # 8 row blocks in all: 512 // 8 = 64 -> the cap 16; 16 tiles of 1000 columns, one each.  40 blocks: 12 splits -> ceil(16 / 12) = 2
    # tiles per split and so 8 splits of 2 tiles: every split owns at least one tile, none is empty
    assert ops.nn_pairs_plan([0], [1], [1000, 1000]).work.shape == (8 * 16, 4)
    mid = ops.nn_pairs_plan([0] * 5, [1] * 5, [1000, 1000])
    assert mid.nsplit == 12 and [tuple(w) for w in mid.work[:9].tolist()] == [(0, 0, 2 * k, 2 * k + 2) for k in range(8)] + [(0, 1, 0, 2)]
    # every item covers its pair's tiles exactly once per row block
    for pl_ in (pl, big, mid):
        cover = {}
        for p, b, lo, hi in pl_.work.tolist():
            cover.setdefault((p, b), []).extend(range(lo, hi))
        for (p, b), tiles in cover.items():
            n1 = int(pl_.col_off[p + 1] - pl_.col_off[p])
            assert tiles == list(range((n1 + 63) // 64)) and b * 128 < int(pl_.row_off[p + 1] - pl_.row_off[p])
    from gim_amd._lib import GimHipError
    with pytest.raises(GimHipError, match="outside"):
        ops.nn_pairs_plan([0, 4], [1, 0], [257, 130, 0, 1])
    empty = ops.nn_pairs_plan([], [], [5, 5])
    assert empty.row_off.tolist() == [0] and empty.work.shape == (0, 4)


class _StubLib:
    """the library with the launches stubbed (there is no device here): the planner and the size query are the real ones"""
    calls = []

    def __init__(self, real):
        self.gim_nn_match_pairs_plan = real.gim_nn_match_pairs_plan
        self.gim_nn_match_pairs_ws_bytes = real.gim_nn_match_pairs_ws_bytes
        self.gim_last_error = real.gim_last_error
        self.calls = []

    def gim_nn_bank_put(self, desc, n, D, rootsift, slot, *rest):
        self.calls.append(("put", n, D, rootsift, slot))
        return 0

    def gim_nn_match_pairs(self, *a):
        self.calls.append(("match", a[7], a[8], a[9], a[10], a[11], a[19]))      # P, n_work, nsplit, rows0, rows1, hloc
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    from gim_amd import ops
    stub = _StubLib(ops.lib)
    monkeypatch.setattr(ops, "lib", stub)
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    return stub


def test_descriptor_bank_bookkeeping(stubbed):
    from gim_amd._lib import GimHipError
    from gim_amd.nn_match import DescriptorBank, RootSiftMatcher, match_descriptor_pair_list
    bank = DescriptorBank(3, 50, D=32, device="cpu")
    assert len(bank) == 0 and "a" not in bank and bank.nbytes == 3 * 50 * 32 * 4 + 3 * 50 * 2 * 4 + 3 * 4

    def img(n, D=32):
        return torch.rand(n, 2), torch.rand(n, D)
    sa, sb, sc = bank.put("a", *img(10)), bank.put("b", *img(0)), bank.put("c", *img(50))
    assert sorted((sa, sb, sc)) == [0, 1, 2] and len(bank) == 3 and bank.stats.misses == 3 and bank.stats.evictions == 0
    assert [c[1:] for c in stubbed.calls] == [(10, 32, 1, sa), (0, 32, 1, sb), (50, 32, 1, sc)]          # n = 0 is an image like any other
    assert bank.counts.tolist() == [{sa: 10, sb: 0, sc: 50}[s] for s in range(3)]
    # refused before anything changes: too many rows, another width, keypoints that do not belong
    for bad, what in ((img(51), "max_rows=50"), (img(5, 16), "width 32"), ((torch.rand(4, 2), torch.rand(5, 32)), "keypoints")):
        with pytest.raises(GimHipError, match=what):
            bank.put("d", *bad)
    assert "d" not in bank and len(stubbed.calls) == 3 and bank.stats.evictions == 0
    # LRU: naming a and c makes b the oldest; d takes its slot; a resident key keeps its slot
    assert bank.slots(["a", "c", "a"]) == [sa, sc, sa]
    assert bank.put("d", *img(7)) == sb and "b" not in bank and bank.stats.evictions == 1 and bank.counts[sb] == 7
    assert bank.put("a", *img(3)) == sa and bank.counts[sa] == 3 and bank.stats.evictions == 1
    with pytest.raises(GimHipError, match="'b' is not resident"):
        bank.slots(["a", "b"])
    with pytest.raises(GimHipError, match="not resident"):
        match_descriptor_pair_list(bank, [("a", "c"), ("b", "c")])
    with pytest.raises(GimHipError, match="outside"):
        RootSiftMatcher().match_pairs(bank, [0, 3], [1, 0])
    assert not [c for c in stubbed.calls if c[0] == "match"]                                            # nothing was launched
    with pytest.raises(GimHipError, match="D=24"):
        DescriptorBank(2, 8, D=24, device="cpu")


def test_wrapper_sizes_a_batch_from_the_host_mirror(stubbed, monkeypatch):
    """ops.nn_match_pairs with the launch stubbed: every size comes from the host counts, nothing of size n0 x n1 is requested, and the
    launch gets the planner's figures"""
    from gim_amd import ops
    from gim_amd.nn_match import DescriptorBank
    requests = []
    real_empty = torch.empty

    def spy(*size, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        requests.append(int(np.prod([int(x) for x in shape])) if len(shape) else 1)
        return real_empty(*size, **kw)
    bank = DescriptorBank(3, 4096, D=128, device="cpu")
    for k, n in (("x", 4096), ("y", 4000), ("z", 0)):
        bank.put(k, torch.zeros(n, 2), torch.ones(n, 128))
    monkeypatch.setattr(ops.torch, "empty", spy)
    s = bank.slots(["x", "y", "z", "x"])
    r = ops.nn_match_pairs(bank.desc, bank.n, bank.counts, [s[0], s[1], s[2], s[3]], [s[1], s[0], s[0], s[2]], hloc=True)
    assert r.row_off.tolist() == [0, 4096, 8096, 8096, 12192]
    assert r.match0.shape == r.score0.shape == r.matches0_i16.shape == r.matching_scores0_f16.shape == (12192,) and r.count.shape == (4,)
    assert r.matches0_i16.dtype == torch.int16 and r.matching_scores0_f16.dtype == torch.float16
    assert stubbed.calls[-1] == ("match", 4, 32 * 8 + 32 * 8, 8, 12192, 4000 + 4096 + 4096, 1)          # 64 row blocks -> 8 splits
    assert max(requests) < 4000 * 4096 // 4 and sum(requests) <= 4 * (17 * 12192 * 3 + 12192) + 4096 + 12192 * 4 + 4
