"""GPU tests of the root_sift descriptor matcher (gim_amd/csrc/nn_match.hip, ops.nn_match, gim_amd/nn_match.py, the hloc plugin
nn_ratio_hip) against the CPU oracle tests/nn_match_oracle.py.

Parity bar: on DECIDABLE rows (all three fp64 margins above EPS = 2 * 128 * 2^-24, nn_match_oracle.margins_f64) match0 equals the fp64
oracle's index exactly and score0 is within EPS of it; undecidable rows are at most 2 % of a case (test_nn_match_cpu.py shows from the
oracles alone that the chosen seeds keep that cap).  The tie rule (lowest column index among bit-equal row maxima) is tested on its own.
"""
import numpy as np
import pytest
import torch

import nn_match_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(desc0, desc1, rootsift, ratio=O.RATIO):
    from gim_amd import ops
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    m, s = ops.nn_match(desc0.to(DEV), desc1.to(DEV), rootsift=rootsift, ratio=ratio, count=count)
    torch.cuda.synchronize()
    assert m.dtype == torch.int32 and s.dtype == torch.float32 and m.shape == s.shape == (desc0.shape[0],)
    return m.cpu().long(), s.cpu(), int(count[0])


def _check_parity(k, m, s, cnt):
    f = k["f64"]
    d = f["decidable"]
    n = len(d)
    und = 1.0 - d.float().mean().item()
    err = (s.double() - f["score0"]).abs()
    print(f"rows {n} decidable {int(d.sum())} undecidable {und:.4f} index flips on decidable {int((m[d] != f['match0'][d]).sum())} "
          f"flips on all rows {int((m != f['match0']).sum())} max score err {err.max().item():.3e} (EPS {O.EPS:.3e}) valid {cnt}")
    assert und <= O.UNDECIDABLE_CAP
    assert torch.equal(m[d], f["match0"][d])
    assert err[d].max().item() <= O.EPS
    assert cnt == int((m >= 0).sum())
    assert ((m >= -1) & (m < k["desc1"].shape[0])).all()


@pytest.mark.parametrize("rootsift", [True, False], ids=["rootsift", "plain"])
@pytest.mark.parametrize("shape", O.CASES, ids=str)
def test_parity_with_fp64_oracle(shape, rootsift):
    k = O.case(*shape, rootsift)
    m, s, cnt = _run(k["desc0"], k["desc1"], rootsift)
    _check_parity(k, m, s, cnt)
    n0 = shape[0]
    if n0 >= 5:     # a single row cannot be 20 % valid and 20 % rejected at once; from 7 rows on both kinds exist in quantity
        valid = (m >= 0).float().mean().item()
        assert valid >= 0.2 and 1.0 - valid >= 0.2, valid


@pytest.mark.parametrize("shape", [(257, 130, 128), (1000, 777, 128), (300, 300, 16)], ids=str)
def test_ratio_off_is_mutual_nearest_neighbour(shape):
    for ratio in (0.0, -1.0):
        k = O.case(*shape, True, ratio)
        m, s, cnt = _run(k["desc0"], k["desc1"], True, ratio)
        _check_parity(k, m, s, cnt)
    with_ratio = O.case(*shape, True)["f64"]["match0"]
    assert int((m >= 0).sum()) > int((with_ratio >= 0).sum())       # the ratio test had been rejecting mutual neighbours


def test_zero_sum_rows_never_match():
    """a zero-sum row under rootsift is 0 / 0: it gets match0 = -1 as a desc0 row and is never the argument of a match as a desc1 row; the
    other rows match as if the zero rows were not there (the reference's column maxima would all be NaN: nn_match.hip header)"""
    n0, n1, D = 257, 130, 128
    k = O.case(n0, n1, D, True)
    desc0, desc1 = k["desc0"].clone(), k["desc1"].clone()
    z0 = torch.tensor([0, 31, 32, 128, 256])
    z1 = torch.tensor([0, 63, 64, 129])
    desc0[z0] = 0
    desc1[z1] = 0
    m, s, cnt = _run(desc0, desc1, True)
    assert (m[z0] == -1).all()
    assert not np.isin(m.numpy(), z1.numpy()).any()
    keep0 = torch.ones(n0, dtype=torch.bool)
    keep0[z0] = False
    keep1 = torch.ones(n1, dtype=torch.bool)
    keep1[z1] = False
    f = O.margins_f64(desc0[keep0], desc1[keep1], True)
    old = torch.nonzero(keep1)[:, 0]
    want = torch.where(f["match0"] >= 0, old[f["match0"].clamp_min(0)], f["match0"])
    d = f["decidable"]
    assert d.float().mean().item() >= 1 - O.UNDECIDABLE_CAP
    assert torch.equal(m[keep0][d], want[d])
    assert cnt == int((m >= 0).sum()) and cnt > 0


@pytest.mark.parametrize("n0,n1", [(0, 5), (5, 0), (0, 0), (5, 1), (200, 1)])
def test_degenerate_sizes_are_empty(n0, n1):
    g = torch.Generator().manual_seed(n0 * 10 + n1)
    desc0, desc1 = torch.rand(n0, 128, generator=g) + 0.01, torch.rand(n1, 128, generator=g) + 0.01
    m, s, cnt = _run(desc0, desc1, True)
    assert cnt == 0 and (m == -1).all()
    if n1 == 1 and n0:
        # with the ratio test off the single column goes to the row that is nearest to it
        m, s, cnt = _run(desc0, desc1, True, 0.0)
        sim = O.nn_match(desc0, desc1, True, 0.0, fp32=False)[2][:, 0]
        top = torch.topk(sim, 2).values if n0 > 1 else None
        if top is None or top[0] - top[1] > O.EPS:
            assert cnt == 1 and int(torch.nonzero(m >= 0)[0, 0]) == int(sim.argmax())


def test_duplicate_descriptors_report_the_lowest_index():
    """tie rule of the kernel header: among bit-equal row maxima the lowest column; with ratio <= 0 the row then matches when it holds the
    column maximum.  Columns 3, 70 (another column group of the same sweep step) and 200 (a later step) of desc1 are copies of one row."""
    k = O.case(300, 300, 16, False)
    desc0, desc1 = k["desc0"].clone(), k["desc1"].clone()
    desc1[[3, 70, 200]] = desc0[5]
    m, s, cnt = _run(desc0, desc1, False, 0.0)
    assert int(m[5]) == 3
    assert abs(float(s[5]) - 1.0) <= O.EPS
    m2, _, cnt2 = _run(desc0, desc1, False, O.RATIO)        # best == second: sqrt(0) / sqrt(0) (or a ratio of 1) fails the ratio test
    assert int(m2[5]) == -1
    # rows 9 and 140 of desc0 equal and column 7 of desc1 a copy of them: the two rows tie for the column bit-exactly, both are mutual
    desc0[140] = desc0[9]
    desc1 = k["desc1"].clone()
    desc1[7] = desc0[9]
    m3, _, _ = _run(desc0, desc1, False, 0.0)
    assert int(m3[9]) == 7 and int(m3[140]) == 7


def test_tie_rule_differs_from_the_reference_as_documented():
    """the 3 x 3 case worked by hand in test_nn_match_cpu.py (exact products): row0 = e1 ties columns 1 and 2 bit-exactly and holds column 2
    only.  The reference's mask.max(1) picks the mutual column (2); the kernel reports the lowest (1), which row1 holds -> -1."""
    def v(*x):
        r = torch.zeros(16)
        r[:4] = torch.tensor(x)
        return r
    e0, e1, h, g, kk = v(1, 0, 0, 0), v(0, 1, 0, 0), v(.5, .5, .5, .5), v(.5, .5, -.5, -.5), v(.5, -.5, .5, -.5)
    desc0, desc1 = torch.stack([e1, h, kk]), torch.stack([e0, h, g])
    assert O.nn_match(desc0, desc1, False, 0.0)[0].tolist() == [2, 1, 0]
    m, s, cnt = _run(desc0, desc1, False, 0.0)
    assert m.tolist() == [-1, 1, 0] and s.tolist() == [.5, 1, .5] and cnt == 2
    m, s, cnt = _run(torch.stack([e0, e1, h, kk]), desc1, False, O.RATIO)       # the 4 x 3 case: no tie decides anything
    assert m.tolist() == [0, -1, 1, -1] and cnt == 2


def test_two_calls_are_bit_identical():
    k = O.case(1000, 777, 128, True)
    a = _run(k["desc0"], k["desc1"], True)
    b = _run(k["desc0"], k["desc1"], True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and a[2] == b[2]


def test_rejects_bad_descriptor_width():
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    for D in (8, 24, 272):
        with pytest.raises(GimHipError):
            ops.nn_match(torch.rand(4, D, device=DEV), torch.rand(4, D, device=DEV))


def test_match_descriptors_contract():
    from gim_amd.nn_match import RootSiftMatcher
    n0, n1, D = 257, 130, 128
    k = O.case(n0, n1, D, True)
    g = torch.Generator().manual_seed(3)
    kpts0, kpts1 = torch.rand(n0, 2, generator=g) * 640, torch.rand(n1, 2, generator=g) * 480
    scale0, scale1 = torch.tensor([[1.5, 2.0]]), torch.tensor([[0.5, 0.25]])
    out = RootSiftMatcher().match_descriptors(kpts0.to(DEV), k["desc0"].to(DEV), kpts1.to(DEV), k["desc1"].to(DEV), scale0.to(DEV),
                                              scale1.to(DEV))
    assert set(out) == {"mkpts0_f", "mkpts1_f", "m_bids", "mconf"}
    assert all(v.is_cuda for v in out.values())
    m, s, cnt = _run(k["desc0"], k["desc1"], True)
    rows = torch.nonzero(m >= 0)[:, 0]                       # ascending desc0 order, as kpts0[valid] gives
    M = len(rows)
    assert M == cnt and M > 0
    assert out["mkpts0_f"].dtype == out["mkpts1_f"].dtype == out["mconf"].dtype == torch.float32 and out["m_bids"].dtype == torch.int64
    assert out["mkpts0_f"].shape == out["mkpts1_f"].shape == (M, 2) and out["m_bids"].shape == out["mconf"].shape == (M,)
    assert torch.equal(out["mkpts0_f"].cpu(), kpts0[rows] * scale0)
    assert torch.equal(out["mkpts1_f"].cpu(), kpts1[m[rows]] * scale1)
    assert torch.equal(out["mconf"].cpu(), s[rows])
    assert (out["m_bids"] == 0).all()
    bare = RootSiftMatcher().match_descriptors(kpts0.to(DEV), k["desc0"].to(DEV), kpts1.to(DEV), k["desc1"].to(DEV))
    assert torch.equal(bare["mkpts0_f"].cpu(), kpts0[rows])


def test_hloc_plugin_round_trip():
    """nn_ratio_hip through the hloc plugin protocol (tests/hloc_stub) into hloc_formats.write_sparse_matches"""
    from hloc.utils.base_model import dynamic_load

    import gim_amd.hloc_matchers as matchers
    from gim_amd import hloc_formats as H

    class FakeH5(dict):
        def create_group(self, name):
            self[name] = FakeH5()
            return self[name]

        def create_dataset(self, name, data):
            self[name] = np.asarray(data)

    Model = dynamic_load(matchers, "nn_ratio_hip")
    with pytest.raises(NotImplementedError):
        Model({"do_mutual_check": False})
    k = O.case(513, 1025, 256, False)                        # unit-norm 256-d rows: SuperPoint's layout [1, D, N]
    model = Model({"ratio_threshold": 0.8})
    pred = model({"descriptors0": k["desc0"].t()[None].to(DEV), "descriptors1": k["desc1"].t()[None].to(DEV)})
    m0, sc = pred["matches0"], pred["matching_scores0"]
    assert m0.shape == sc.shape == (1, 513) and m0.dtype == torch.int64 and sc.dtype == torch.float32
    f = k["f64"]
    d = f["decidable"]
    assert torch.equal(m0[0].cpu()[d], f["match0"][d])
    hit = m0[0].cpu() >= 0
    assert (sc[0].cpu()[~hit] == 0).all()
    assert ((sc[0].cpu()[hit].double() - (f["score0"][hit] + 1) / 2).abs() <= O.EPS).all()
    fd = FakeH5()
    grp = H.write_sparse_matches(fd, "a.jpg", "b.jpg", m0[0].cpu().short().numpy(), sc[0].cpu().half().numpy())
    assert grp["matches0"].dtype == np.int16 and grp["matching_scores0"].dtype == np.float16
    assert np.array_equal(grp["matches0"].astype(np.int64), m0[0].cpu().numpy())
    plain = Model({"ratio_threshold": None})
    assert int((plain({"descriptors0": k["desc0"].t()[None].to(DEV), "descriptors1": k["desc1"].t()[None].to(DEV)})["matches0"] >= 0).sum()) > int(hit.sum())



def test_inference_with_opencv_sift():
    """root_sift_inference end to end where OpenCV is installed: SIFT on a synthetic pair (the second image is the first shifted by
    (6, 4) pixels), the contract's keys, and matches that follow the shift"""
    cv2 = pytest.importorskip("cv2")
    if not hasattr(cv2, "SIFT_create"):
        pytest.skip("this OpenCV build has no SIFT")
    from gim_amd.nn_match import RootSiftMatcher
    g = torch.Generator().manual_seed(11)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, 34, 44, generator=g), size=(136, 176), mode="bicubic").clamp(0, 1)
    c0, c1 = base[..., 4:132, 6:166].contiguous(), base[..., :128, :160].contiguous()       # a point (x, y) of c0 is (x + 6, y + 4) in c1
    data = {"color0": c0.to(DEV), "color1": c1.to(DEV), "image0": c0[:, :1].to(DEV), "image1": c1[:, :1].to(DEV),
            "scale0": torch.tensor([[2.0, 2.0]], device=DEV), "scale1": torch.tensor([[1.0, 1.0]], device=DEV)}
    out = RootSiftMatcher()(data)
    assert out is data and tuple(data["hw0_i"]) == (128, 160) and tuple(data["hw1_i"]) == (128, 160)
    mk0, mk1 = data["mkpts0_f"].cpu(), data["mkpts1_f"].cpu()
    assert mk0.shape == mk1.shape and mk0.shape[1] == 2 and data["m_bids"].shape == data["mconf"].shape == (mk0.shape[0],)
    assert (data["m_bids"] == 0).all() and mk0.shape[0] >= 8
    d = mk1 - mk0 / 2.0
    assert ((d - torch.tensor([6.0, 4.0])).abs().max(1).values < 1.0).float().mean().item() > 0.8
