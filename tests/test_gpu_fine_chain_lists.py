"""The pair range of the fine head's patch-list kernel (gim_fine_tile_lists4_range, ops.fine_tile_lists(depth=3, b_range=...)): what the two
pair-range chains of gim_loftr's sparse fine head (loftr.py: `fine_chains`) build their lists with.

Synthetic match lists (fixed seed) on bs = 2 and 3 pairs, half-level map 32 x 64 (4 x 2 patches per image), quarter-level map 16 x 32.  For
every split point s in 0 .. bs the lists of [0, s) and [s, bs) are computed; for each of the five lists (+-3, +-4, A, B, C) the two
outputs are disjoint, their sorted concatenation is the full-range list exactly, and the counts add up.  [0, bs) equals the entry point
without a range byte for byte (lists up to their counts, and the counts).  Every buffer is prefilled with a sentinel: nothing is written
behind a count, and an empty range writes five zero counts and no list entry.

The match sets: cells on every border and corner of every image; a pair without a match; a set where the +-3 and the +-4 list differ
(odd coarse rows: 4 cy + 4 = 8 k reaches the next patch row through the fourth pixel only).  A set where the quarter-level lists A, B and C
differ from one another does not exist at a size the entry accepts (H = 2 h, whole patches): the sources staged for half-level patch
row 2 k are the quarter rows 8 k - 1 .. 8 k + 4, for row 2 k + 1 they are 8 k + 3 .. 8 k + 8 (columns alike with 32 in place of 8), so
S already touches both quarter patches that a dilation by 2 could reach -- the numpy staging model of tests/test_gpu_quarter_lists.py
gives A = B = C for every single match at 32 x 64, 64 x 128 and 240 x 320.  The three lists are still checked one by one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 32, 64
HC, WC = H // 4, W // 4
SENTINEL = -7
NAMES = ("+-3", "+-4", "A", "B", "C")


def _match_sets(bs):
    """name -> int64 [3, M] (pair, cell of image 0, cell of image 1)"""
    g = np.random.default_rng(20)
    cell = lambda cy, cx: cy * WC + cx   # noqa: E731
    border = ([cell(0, x) for x in range(WC)] + [cell(HC - 1, x) for x in range(WC)] + [cell(y, 0) for y in range(HC)]
              + [cell(y, WC - 1) for y in range(HC)])   # the corners are in it twice
    sets = {}
    rows = [(b, c, border[(k + 5 * b + 7) % len(border)]) for b in range(bs) for k, c in enumerate(border)]
    sets["borders"] = [rows[k] for k in g.permutation(len(rows))]   # pairs interleaved, as coarse matching's atomics leave them
    empty = bs // 2   # this pair has no match: its images list nothing, in either range
    sets["empty pair"] = [(b, int(g.integers(HC * WC)), int(g.integers(HC * WC))) for b in range(bs) if b != empty for _ in range(3)]
    # odd cy, and cx = 7 (4 cx + 4 = 32): the +-4 reach touches a patch the +-3 reach does not; one match per image side, sides differ
    sets["+-3 and +-4 differ"] = [(b, cell(1, 7 if b % 2 else 3), cell(5 if b % 2 else 3, 2)) for b in range(bs)]
    sets["none"] = []
    return {k: np.array(v, dtype=np.int64).reshape(-1, 3).T for k, v in sets.items()}


def _lists(ids, cnt, bs, b_range):
    """the five lists (numpy, up to their counts) and what lies behind the counts, from sentinel-filled buffers of the C entry itself"""
    from gim_amd import ops
    total, totq = 2 * bs * (H // 8) * (W // 32), 2 * bs * (H // 16) * (W // 64)
    t = torch.full((2 * total + 3 * totq,), SENTINEL, dtype=torch.int32, device=DEV)
    n = torch.full((5,), SENTINEL, dtype=torch.int32, device=DEV)
    p = ops._p
    args = (p(ids[0]), p(ids[1]), p(ids[2]), p(cnt), ids.shape[1], bs, WC, WC, 4, H, W, p(t[:total]), p(n[0:1]), p(t[total:2 * total]), p(n[1:2]),
            total, p(t[2 * total:]), p(n[2:5]), totq)
    if b_range is None:
        ops.check(ops.lib.gim_fine_tile_lists4(*args, ops._stream()), "gim_fine_tile_lists4")
    else:
        ops.check(ops.lib.gim_fine_tile_lists4_range(*args, b_range[0], b_range[1], ops._stream()), "gim_fine_tile_lists4_range")
    torch.cuda.synchronize()
    t, n = t.cpu().numpy(), n.cpu().numpy()
    bufs = [t[:total], t[total:2 * total]] + [t[2 * total + k * totq:2 * total + (k + 1) * totq] for k in range(3)]
    assert all(0 <= n[k] <= len(bufs[k]) for k in range(5)), n
    for k in range(5):
        assert np.all(bufs[k][n[k]:] == SENTINEL), f"list {NAMES[k]}: an entry behind the count {n[k]} was written"
    return [bufs[k][:n[k]].copy() for k in range(5)], n


@pytest.mark.parametrize("which", ["borders", "empty pair", "+-3 and +-4 differ", "none"])
@pytest.mark.parametrize("bs", [2, 3])
def test_pair_ranges_partition_the_lists(bs, which):
    from gim_amd import ops
    assert ops.fine_tile_lists4_fits(bs, H, W)
    m = _match_sets(bs)[which]
    M = m.shape[1]
    ids = torch.full((3, M + 3), 10 ** 12, dtype=torch.int64)   # rows beyond the count are never read
    ids[:, :M] = torch.from_numpy(m)
    ids = ids.to(DEV)
    cnt = torch.tensor([M, 0, 0, 0], dtype=torch.int32, device=DEV)
    full, nfull = _lists(ids, cnt, bs, None)
    whole, nwhole = _lists(ids, cnt, bs, (0, bs))
    for k in range(5):
        assert full[k].tobytes() == whole[k].tobytes() and nfull[k] == nwhole[k], f"list {NAMES[k]}: [0, bs) differs from the entry without a range"
        assert np.all(np.diff(full[k]) > 0)
    print(f"bs {bs} {which}: {M} matches, counts {nfull.tolist()}")
    if which == "none":
        assert not nfull.any()
    else:
        assert nfull.all()
    if which == "+-3 and +-4 differ":
        assert nfull[1] > nfull[0]
    per, perq = (H // 8) * (W // 32), (H // 16) * (W // 64)
    if which == "empty pair":
        for k in range(5):
            img = full[k] // (per if k < 2 else perq)
            assert not np.isin(img, [bs // 2, bs + bs // 2]).any()
    for s in range(bs + 1):
        lo, nlo = _lists(ids, cnt, bs, (0, s))
        hi, nhi = _lists(ids, cnt, bs, (s, bs))
        for k in range(5):
            what = f"list {NAMES[k]}, split {s}"
            assert not np.intersect1d(lo[k], hi[k]).size, what
            assert np.array_equal(np.sort(np.concatenate([lo[k], hi[k]])), full[k]), what
            assert nlo[k] + nhi[k] == nfull[k], what
            # a range lists patches of its own pairs' images only: b in [0, s) -> images b and bs + b
            pairs = (lo[k] // (per if k < 2 else perq)) % bs
            assert np.all(pairs < s), what
        if s == 0:
            assert not nlo.any() and all(len(x) == 0 for x in lo)      # the empty range: five zero counts, no entry (sentinels checked in _lists)
        if s == bs:
            assert not nhi.any() and all(len(x) == 0 for x in hi)


def test_the_wrapper_takes_the_range_and_the_entry_refuses_a_bad_one():
    from gim_amd import ops
    bs = 2
    m = _match_sets(bs)["borders"]
    ids = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    cnt = torch.tensor([m.shape[1], 0, 0, 0], dtype=torch.int32, device=DEV)
    ref, nref = _lists(ids, cnt, bs, (1, 2))
    t3, n3, t4, n4, tq, nq = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, WC, WC, 4, H, W, depth=3, b_range=(1, 2))
    torch.cuda.synchronize()
    got = [t3[:int(n3)], t4[:int(n4)]] + [tq[k, :int(nq[k])] for k in range(3)]
    for k in range(5):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), NAMES[k]
    for bad in ((-1, 1), (1, 3), (2, 1)):
        with pytest.raises(Exception, match="pair range"):
            ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, WC, WC, 4, H, W, depth=3, b_range=bad)
