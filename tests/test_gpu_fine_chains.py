"""The sparse fine head of gim_loftr as two pair-range chains on parallel streams (gim_amd/loftr/fine_head.py: `fine_chains`, _fine_tail_sparse).

forward() with fine_chains = 2 against forward() with fine_chains = 1 (the launch sequence it had before), same weights, one process, fp16:
every output tensor torch.equal -- eager, graph capture, and three replays on changing inputs.  Shapes: bs = 2 at 64 x 128 and bs = 3
(an odd batch: chains of 1 and 2 pairs) at 128 x 256 -- 128 x 192 has a 32 x 48 quarter-level map, not whole 8 x 32 patches, so the module
keeps that size's quarter level dense (tests/test_gpu_quarter_sparse.py) and the chains never start; 128 x 256 is the next width that is
whole patches.  The test asserts that the chained path really ran there (two ranged list launches per forward).  `force_big_tile`
sends the small fixture's launches onto the 256 x 256 tile in BOTH models, as in tests/test_gpu_quarter_sparse.py.

One case fills the six maps the chains write with NaN in front of every forward (as tests/test_gpu_quarter_lists.py poisons its buffers):
no stale or unwritten value reaches an output.  One case keeps all matches of a step inside one chain's pairs: the other chain's seven
launches see count 0."""
import pytest
import torch

from tools import synth_loftr as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT = ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f")


def _forward(model, c0, c1):
    d = {"image0": c0[:, :1], "image1": c1[:, :1], "color0": c0, "color1": c1}
    model(d)
    torch.cuda.synchronize()
    return {k: d[k].clone() for k in OUT}


def _same(got, ref, what):
    for k in OUT:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (what, k)


@pytest.fixture(scope="module")
def models():
    """(fine_chains = 2, fine_chains = 1, fine_chains = 2 without graphs), the same weights"""
    two, sd = S.synthetic_model("fp16", fine_chains=2)
    out = [two]
    for over in ({"fine_chains": 1}, {"fine_chains": 2, "graph": False}):
        m, _ = S.synthetic_model("fp16", **over)
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        out.append(m)
    two, one, eager = (m.to(DEV) for m in out)
    assert two.fine_chains == 2 and one.fine_chains == 1 and eager.fine_chains == 2 and not eager.use_graph and two.use_graph
    return two, one, eager


def _spy(monkeypatch):
    """counts the launches of the ranged list entry itself"""
    from gim_amd import ops
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    took = []
    real = ops.lib.gim_fine_tile_lists4_range
    monkeypatch.setattr(ops.lib, "gim_fine_tile_lists4_range", lambda *a: (took.append((a[-3], a[-2])), real(*a))[1])
    return took


@pytest.mark.parametrize("bs,hw,must_chain", [(2, (64, 128), False), (3, (128, 256), True)], ids=["bs2-64x128", "bs3-128x256"])
def test_two_chains_are_bit_identical_to_one(models, bs, hw, must_chain, monkeypatch):
    two, one, _ = models
    took = _spy(monkeypatch)
    c0, c1 = (t.to(DEV) for t in S.textured_pairs(bs, *hw, seed=3, frac=0.5))
    P = two._prepack(torch.device(DEV))
    x = two._to_nhwc([c0, c1], two._img_dt())
    chained = two._quarter_sparse_ok(P, [x])
    print(f"bs {bs} {hw}: fine_sparse {two._fine_sparse_ok(P, [x])}, quarter_sparse {chained}")
    assert chained or not must_chain
    ref = _forward(one, c0, c1)
    assert not took, "the one-chain model launched the ranged list entry"
    print(f"  {int(ref['b_ids'].numel())} matches, per pair {torch.bincount(ref['b_ids'], minlength=bs).tolist()}")
    if must_chain:
        assert ref["b_ids"].numel() > 50 and bool((torch.bincount(ref["b_ids"], minlength=bs) > 0).all())
    for rep in range(2):   # eager, graph capture
        _same(_forward(two, c0, c1), ref, f"forward {rep}")
    if chained:
        lo, hi = (0, bs // 2), (bs // 2, bs)                      # an odd bs as bs // 2 and the rest
        assert set(took) == {lo, hi} and took.count(lo) == took.count(hi) >= 2, took   # both chains, in the eager run and in the capture
    else:
        assert not took
    # three replays on changing inputs: mirrored (the matches move to the other side of both frames), noise (few matches or none), the first again
    g = torch.Generator().manual_seed(4)
    z0, z1 = torch.rand(bs, 3, *hw, generator=g).to(DEV), torch.rand(bs, 3, *hw, generator=g).to(DEV)
    n_graphs, n_took = len(two._graphs), len(took)
    for what, (a, b) in (("mirrored", (c0.flip(-1).contiguous(), c1.flip(-1).contiguous())), ("noise", (z0, z1)), ("first again", (c0, c1))):
        _same(_forward(two, a, b), _forward(one, a, b), what)
    assert len(two._graphs) == n_graphs and len(took) == n_took   # replays: no new capture, no new launch from the host


def test_no_stale_value_reaches_an_output(models, monkeypatch):
    """the six maps between the trunk and the fused fine kernel hold NaN when the chains start"""
    _, one, eager = models
    took = _spy(monkeypatch)
    bs, hw = 3, (128, 256)
    poisoned = []
    real = eager._fine_head_maps

    def maps(*a):
        ms = real(*a)
        for m in ms:
            m.fill_(float("nan"))
        poisoned.append(len(ms))
        return ms

    monkeypatch.setattr(eager, "_fine_head_maps", maps)
    c0, c1 = (t.to(DEV) for t in S.textured_pairs(bs, *hw, seed=3, frac=0.5))
    ref = _forward(one, c0, c1)
    assert ref["b_ids"].numel() > 50
    got = _forward(eager, c0, c1)
    assert poisoned == [6] and len(took) == 2
    for k in ("mkpts0_f", "mkpts1_f", "expec_f", "mconf"):
        assert bool(torch.isfinite(got[k].float()).all()), k
    _same(got, ref, "poisoned maps")
    m0, m1 = c0.flip(-1).contiguous(), c1.flip(-1).contiguous()
    _same(_forward(eager, m0, m1), _forward(one, m0, m1), "poisoned maps, mirrored")
    assert poisoned == [6, 6]


def test_all_matches_in_one_chain(models, monkeypatch):
    """pair 1 has no match: chain 1's list launch writes five zero counts and its six launches walk empty lists"""
    two, one, _ = models
    took = _spy(monkeypatch)
    bs, hw = 2, (128, 256)
    c0, c1 = S.textured_pairs(bs, *hw, seed=3, frac=0.5)
    g = torch.Generator().manual_seed(6)
    ref = None
    for what, fill in (("flat", lambda t: torch.full_like(t, 0.5)), ("noise", lambda t: torch.rand(t.shape, generator=g))):
        a, b = c0.clone(), c1.clone()
        a[1], b[1] = fill(a[1]), fill(b[1])
        a, b = a.to(DEV), b.to(DEV)
        ref = _forward(one, a, b)
        per = torch.bincount(ref["b_ids"], minlength=bs).tolist()
        print(f"pair 1 {what}: matches per pair {per}")
        if per[0] > 50 and per[1] == 0:
            break
    assert per[0] > 50 and per[1] == 0, per
    for rep in range(3):   # eager, capture, replay
        _same(_forward(two, a, b), ref, f"forward {rep}")
    assert set(took) == {(0, 1), (1, 2)} and took.count((0, 1)) == took.count((1, 2)) >= 2, took
    # ... and the other way round on the same graph: pair 0's images in pair 1's place
    a2, b2 = a.flip(0).contiguous(), b.flip(0).contiguous()
    ref2 = _forward(one, a2, b2)
    per2 = torch.bincount(ref2["b_ids"], minlength=bs).tolist()
    assert per2[0] == 0 and per2[1] > 50, per2
    _same(_forward(two, a2, b2), ref2, "all matches in the second chain")
