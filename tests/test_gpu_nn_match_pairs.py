"""GPU tests of root_sift over a pair list: the descriptor bank (gim_nn_bank_put), the batched matcher (gim_nn_match_pairs, ops.nn_match_pairs),
`DescriptorBank`, `RootSiftMatcher.match_pairs`, `match_descriptor_pair_list` and `NnRatioHip.match_pairs_from_features`.

Main bar: BIT-identity with the single-pair path (ops.nn_match on the raw descriptors of each pair): the ragged match0 slices are equal,
the score0 slices are equal as int32 views, the counts are equal -- no tolerance, the sweep is the same k-ordered fmaf chain and the row /
column reductions do not depend on how the columns are split.  Independently of the existing kernel, the pooled rows of a list are held
to the fp64 oracle (tests/nn_match_oracle.py) on decidable rows; tests/test_nn_match_pairs_cpu.py shows from the oracle alone that the
banks below keep the 2 % cap on undecidable rows (bank C without rootsift does not, 0.0229, and is covered by the bit-identity only).
"""
import numpy as np
import pytest
import torch

import nn_match_oracle as O
import nn_match_pairs_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_BANKS, _SINGLE = {}, {}


def _bank(name, rootsift):
    """the DescriptorBank of a case, built once and only read afterwards"""
    from gim_amd.nn_match import DescriptorBank
    key = (name, rootsift)
    if key not in _BANKS:
        imgs = C.images(name, rootsift)
        bank = DescriptorBank(len(imgs), max(d.shape[0] for d in imgs), D=C.BANKS[name]["D"], rootsift=rootsift, device=DEV)
        for i, d in enumerate(imgs):
            assert bank.put(i, C.keypoints(name, i).to(DEV), d.to(DEV)) == i
        _BANKS[key] = bank
    return _BANKS[key]


def _single(name, rootsift, ratio, i, j):
    """ops.nn_match on the raw descriptors of pair (i, j): the reference of the bit-identity, computed once"""
    from gim_amd import ops
    key = (name, rootsift, ratio, i, j)
    if key not in _SINGLE:
        imgs = C.images(name, rootsift)
        count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        m, s = ops.nn_match(imgs[i].to(DEV), imgs[j].to(DEV), rootsift=rootsift, ratio=ratio, count=count)
        _SINGLE[key] = (m.cpu(), s.cpu(), int(count[0]))
    return _SINGLE[key]


def _run(bank, pairs, ratio, hloc=False):
    from gim_amd import ops
    r = ops.nn_match_pairs(bank.desc, bank.n, bank.counts, [p[0] for p in pairs], [p[1] for p in pairs], ratio=ratio, hloc=hloc)
    torch.cuda.synchronize()
    return r


def _same_as_single(name, rootsift, ratio, pairs, r):
    m, s, cnt = r.match0.cpu(), r.score0.cpu(), r.count.cpu()
    assert m.dtype == torch.int32 and s.dtype == torch.float32 and cnt.dtype == torch.int32 and cnt.shape == (len(pairs),)
    assert r.row_off[-1] == m.shape[0] == s.shape[0]
    for p, (i, j) in enumerate(pairs):
        lo, hi = int(r.row_off[p]), int(r.row_off[p + 1])
        m1, s1, c1 = _single(name, rootsift, ratio, i, j)
        assert hi - lo == m1.shape[0], (p, i, j)
        assert torch.equal(m[lo:hi], m1), (p, i, j)
        assert torch.equal(s[lo:hi].view(torch.int32), s1.view(torch.int32)), (p, i, j)
        assert int(cnt[p]) == c1, (p, i, j)


@pytest.mark.parametrize("ratio", [0.8, 0.0])
@pytest.mark.parametrize("rootsift", [True, False], ids=["rootsift", "plain"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_bit_identical_to_the_single_pair_path(name, rootsift, ratio):
    bank, pairs = _bank(name, rootsift), C.PAIRS[name]
    r = _run(bank, pairs, ratio)
    _same_as_single(name, rootsift, ratio, pairs, r)
    # the list split across two launch sequences: another column split, the same bits
    cut = len(pairs) // 2 + 1
    _same_as_single(name, rootsift, ratio, pairs[:cut], _run(bank, pairs[:cut], ratio))
    _same_as_single(name, rootsift, ratio, pairs[cut:], _run(bank, pairs[cut:], ratio))
    # and run again: bit-equal
    r2 = _run(bank, pairs, ratio)
    assert torch.equal(r.match0, r2.match0) and torch.equal(r.score0.view(torch.int32), r2.score0.view(torch.int32))
    assert torch.equal(r.count, r2.count)


def test_stored_rows_are_the_single_pair_normalisation():
    """the bank holds sqrt(d / sum d) in fp32 as the oracle's fp32 restatement up to rounding, rows past n untouched by the count"""
    bank = _bank("A", True)
    imgs = C.images("A", True)
    assert bank.n.cpu().tolist() == [d.shape[0] for d in imgs] == bank.counts.tolist()
    for i, d in enumerate(imgs):
        got = bank.desc[i, :d.shape[0]].cpu()
        if d.shape[0]:
            assert (got - O.root_sift(d)).abs().max().item() <= 2.0 ** -22      # values in [0, 1]: a few ulp of division and square root
    plain = _bank("A", False)
    for i, d in enumerate(C.images("A", False)):
        assert torch.equal(plain.desc[i, :d.shape[0]].cpu(), d)


@pytest.mark.parametrize("ratio", [0.8, 0.0])
@pytest.mark.parametrize("name,rootsift", [("A", True), ("A", False), ("B", True), ("B", False), ("C", True)])
def test_parity_with_fp64_oracle(name, rootsift, ratio):
    pairs = C.PAIRS[name]
    r = _run(_bank(name, rootsift), pairs, ratio)
    f = C.pooled_oracle(name, rootsift, ratio)
    m, s = r.match0.cpu().long(), r.score0.cpu()
    d, pool = f["decidable"], f["pool"]
    assert m.shape == d.shape
    und = 1.0 - d[pool].float().mean().item()
    err = (s.double() - f["score0"]).abs()
    matched = (m[pool] >= 0).float().mean().item()
    print(f"bank {name} rootsift={rootsift} ratio={ratio}: pooled rows {int(pool.sum())} undecidable {und:.4f} flips on decidable "
          f"{int((m[d] != f['match0'][d]).sum())} max score err on decidable {err[d].max().item():.3e} (EPS {O.EPS:.3e}) matched {matched:.3f}")
    assert und <= O.UNDECIDABLE_CAP
    assert torch.equal(m[d], f["match0"][d])
    assert err[d].max().item() <= O.EPS
    assert matched >= 0.2 and 1.0 - matched >= 0.2
    assert r.count.cpu().tolist() == [int((m[int(r.row_off[p]):int(r.row_off[p + 1])] >= 0).sum()) for p in range(len(pairs))]


def test_degenerate_pairs():
    bank, pairs = _bank("A", True), C.PAIRS["A"]
    at = {p: k for k, p in enumerate(pairs)}
    r = _run(bank, pairs, 0.8)
    m, cnt = r.match0.cpu(), r.count.cpu()

    def rows(p):
        return m[int(r.row_off[at[p]]):int(r.row_off[at[p] + 1])]
    assert int(cnt[at[(0, 4)]]) == 0 and rows((0, 4)).shape[0] == 257 and (rows((0, 4)) == -1).all()      # an empty image on the right
    assert int(cnt[at[(4, 0)]]) == 0 and rows((4, 0)).shape[0] == 0                                         # and on the left
    for p in ((0, 3), (1, 3)):                                                                              # n1 = 1: no second neighbour
        assert int(cnt[at[p]]) == 0 and (rows(p) == -1).all() and rows(p).shape[0] > 0
    r0 = _run(bank, pairs, 0.0)
    m0 = r0.match0.cpu()[int(r0.row_off[at[(0, 3)]]):int(r0.row_off[at[(0, 3)] + 1])]
    imgs = C.images("A", True)
    sim = O.nn_match(imgs[0], imgs[3], True, 0.0, fp32=False)[2][:, 0]
    top = torch.topk(sim, 2).values
    if top[0] - top[1] > O.EPS:
        assert int(r0.count[at[(0, 3)]]) == 1 and int(torch.nonzero(m0 >= 0)[0, 0]) == int(sim.argmax())
    # only degenerate pairs: no work item at all
    e = _run(bank, [(0, 4), (4, 0), (4, 4)], 0.8)
    assert e.count.cpu().tolist() == [0, 0, 0] and e.match0.shape[0] == 257 and (e.match0 == -1).all() and (e.score0 == 0).all()
    # an empty list
    z = _run(bank, [], 0.8)
    assert z.match0.shape == z.score0.shape == z.count.shape == (0,) and z.row_off.tolist() == [0]
    from gim_amd.nn_match import RootSiftMatcher, match_descriptor_pair_list
    out = RootSiftMatcher().match_pairs(bank, [], [])
    assert out["mkpts0_f"].shape == (0, 2) and out["m_bids"].shape == (0,) and out["m_bids"].dtype == torch.int64
    assert match_descriptor_pair_list(bank, []) == []


@pytest.mark.parametrize("ratio", [0.8, 0.0])
def test_hloc_emit(ratio):
    r = _run(_bank("A", True), C.PAIRS["A"], ratio, hloc=True)
    m, s = r.match0.cpu(), r.score0.cpu()
    assert r.matches0_i16.dtype == torch.int16 and r.matching_scores0_f16.dtype == torch.float16
    assert torch.equal(r.matches0_i16.cpu(), m.short())
    want = torch.where(m >= 0, (s + 1) / 2, torch.zeros_like(s)).half()
    assert torch.equal(r.matching_scores0_f16.cpu().view(torch.int16), want.view(torch.int16))
    assert int((m >= 0).sum()) > 100


def test_hloc_emit_refuses_rows_beyond_int16():
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    from gim_amd.nn_match import DescriptorBank
    bank = DescriptorBank(2, 32768, D=16, device=DEV)
    bank.put(0, torch.rand(5, 2, device=DEV), torch.rand(5, 16, device=DEV) + 0.01)
    with pytest.raises(GimHipError, match="int16"):
        ops.nn_match_pairs(bank.desc, bank.n, bank.counts, [0], [0], hloc=True)
    import ctypes
    one = ctypes.c_void_p(16)      # never dereferenced: the library refuses on the sizes, before any launch
    rc = ops.lib.gim_nn_match_pairs(one, one, one, one, one, one, one, 1, 1, 1, 5, 5, 2, 32768, 16, 0.8, one, one, one, 1, one, one, one, None)
    assert rc != 0 and b"int16" in ops.lib.gim_last_error()


def test_match_pairs_equals_match_descriptors_per_pair():
    from gim_amd.nn_match import RootSiftMatcher
    bank, pairs = _bank("A", True), C.PAIRS["A"]
    imgs = C.images("A", True)
    P = len(pairs)
    g = torch.Generator().manual_seed(5)
    scale0, scale1 = torch.rand(P, 2, generator=g) + 0.5, torch.rand(P, 2, generator=g) + 0.5
    mt = RootSiftMatcher()
    out = mt.match_pairs(bank, [p[0] for p in pairs], [p[1] for p in pairs], scale0.to(DEV), scale1.to(DEV))
    assert set(out) == {"mkpts0_f", "mkpts1_f", "m_bids", "mconf"} and all(v.is_cuda for v in out.values())
    assert out["mkpts0_f"].dtype == out["mkpts1_f"].dtype == out["mconf"].dtype == torch.float32 and out["m_bids"].dtype == torch.int64
    M = out["m_bids"].shape[0]
    assert out["mkpts0_f"].shape == out["mkpts1_f"].shape == (M, 2) and out["mconf"].shape == (M,)
    bids = out["m_bids"].cpu()
    assert (bids[1:] >= bids[:-1]).all() and M > 100
    total = 0
    for p, (i, j) in enumerate(pairs):
        one = mt.match_descriptors(C.keypoints("A", i).to(DEV), imgs[i].to(DEV), C.keypoints("A", j).to(DEV), imgs[j].to(DEV),
                                   scale0[p].to(DEV), scale1[p:p + 1].to(DEV))
        sel = out["m_bids"] == p
        for k in ("mkpts0_f", "mkpts1_f", "mconf"):
            assert torch.equal(out[k][sel], one[k]), (p, k)
        total += one["mconf"].shape[0]
    assert total == M
    # one scale for every pair, and none
    same = mt.match_pairs(bank, [0, 1], [1, 0], torch.tensor([[2.0, 0.5]]), None)
    bare = mt.match_pairs(bank, [0, 1], [1, 0])
    assert torch.equal(same["mkpts0_f"], bare["mkpts0_f"] * torch.tensor([[2.0, 0.5]], device=DEV))
    assert torch.equal(same["mkpts1_f"], bare["mkpts1_f"])


class FakeH5(dict):
    def create_group(self, name):
        self[name] = FakeH5()
        return self[name]

    def create_dataset(self, name, data):
        self[name] = np.asarray(data)


@pytest.mark.parametrize("layout", ["DN", "ND"])
def test_plugin_pair_list_writes_what_the_per_pair_loop_writes(layout):
    from hloc.utils.base_model import dynamic_load

    import gim_amd.hloc_matchers as matchers
    from gim_amd import hloc_formats as H
    Model = dynamic_load(matchers, "nn_ratio_hip")
    imgs = C.images("A", True)
    names = [f"img{i}.jpg" for i in range(len(imgs))]
    features = {n: {"keypoints": C.keypoints("A", i).numpy(), "descriptors": (d.t() if layout == "DN" else d).contiguous().numpy()}
                for i, (n, d) in enumerate(zip(names, imgs))}
    pairs = [(names[i], names[j]) for i, j in C.PAIRS["A"]]
    model = Model({"ratio_threshold": 0.8, "root_sift": True, "batch_pairs": 5})
    fast = FakeH5()
    rows = model.match_pairs_from_features(features, pairs, fast, device=DEV)
    assert [(a, b) for a, b, _, _ in rows] == pairs
    st = model.bank.stats
    assert st.misses == len(names) == len(model.bank) and st.evictions == 0          # every image was put exactly once
    slow = FakeH5()
    for (a, b), (i, j) in zip(pairs, C.PAIRS["A"]):
        if imgs[i].shape[0] == 0 or imgs[j].shape[0] == 0:
            continue        # the per-pair plugin call takes no empty descriptor set; the fast path's rows for these are all -1 (below)
        pred = model({"descriptors0": imgs[i].t()[None].to(DEV), "descriptors1": imgs[j].t()[None].to(DEV)})
        H.write_sparse_matches(slow, a, b, pred["matches0"][0].cpu().short().numpy(), pred["matching_scores0"][0].cpu().half().numpy())
    assert len(slow) >= 9
    for key, grp in slow.items():
        assert set(fast[key]) == {"matches0", "matching_scores0"}
        assert fast[key]["matches0"].dtype == np.int16 and fast[key]["matching_scores0"].dtype == np.float16
        assert np.array_equal(fast[key]["matches0"], grp["matches0"]), key
        assert np.array_equal(fast[key]["matching_scores0"].view(np.int16), grp["matching_scores0"].view(np.int16)), key
    assert len(fast) == len(pairs)
    for key in set(fast) - set(slow):
        assert (fast[key]["matches0"] == -1).all() and (fast[key]["matching_scores0"] == 0).all()


def test_evicted_image_is_refused_before_any_launch(monkeypatch):
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    from gim_amd.nn_match import DescriptorBank, match_descriptor_pair_list
    bank = DescriptorBank(2, 64, D=16, device=DEV)
    g = torch.Generator().manual_seed(9)
    for k in ("a", "b", "c"):
        bank.put(k, torch.rand(40, 2, generator=g).to(DEV), (torch.rand(40, 16, generator=g) + 0.01).to(DEV))
    assert "a" not in bank and "b" in bank and "c" in bank and len(bank) == 2 and bank.stats.evictions == 1

    def no_launch(*a):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(ops.lib, "gim_nn_match_pairs", no_launch, raising=False)
    with pytest.raises(GimHipError, match="not resident"):
        bank.slots(["b", "a"])
    with pytest.raises(GimHipError, match="not resident"):
        match_descriptor_pair_list(bank, [("b", "c"), ("a", "c")])
    with pytest.raises(GimHipError, match="never inserted"):
        match_descriptor_pair_list(bank, [("zzz", "c")])
