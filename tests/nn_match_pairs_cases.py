"""Banks and pair lists of the pair-list tests of the root_sift matcher (test_nn_match_pairs_cpu.py, test_gpu_nn_match_pairs.py), built from
tests/nn_match_oracle.py and computed once.

Bank image 0 is `desc0` of O.make_descriptors(n0, size, D, seed) (the same for every size: it is drawn first from the seeded generator),
images 1.. are its `desc1` for the listed sizes; size 0 is an image without keypoints.  The shapes reach partial row blocks (257, 300, 130,
65), partial column tiles and a count one past a tile (65), more than one row block, n1 = 1, an empty image on either side, a slot that many
pairs share in both roles, and the three ranges of D (16: the KC = 16 sweep; 128; 256).
"""
import torch

import nn_match_oracle as O

BANKS = {
    "A": {"D": 128, "seed": 211, "n0": 257, "sizes": [130, 300, 1, 0, 65]},
    "B": {"D": 16, "seed": 212, "n0": 300, "sizes": [300, 70]},
    "C": {"D": 256, "seed": 213, "n0": 129, "sizes": [64, 200]},
}
PAIRS = {
    "A": [(0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (0, 5), (5, 0), (2, 5), (0, 3), (3, 0), (1, 3), (0, 4), (4, 0)],
    "B": [(i, j) for i in range(3) for j in range(3) if i != j],
    "C": [(i, j) for i in range(3) for j in range(3) if i != j],
}
_CACHE = {}


def images(name, rootsift=True):
    """the raw descriptors of the bank's images as `put` takes them: SIFT-like counts with rootsift, unit-norm rows (O.l2_rows) without"""
    key = ("img", name, bool(rootsift))
    if key not in _CACHE:
        b = BANKS[name]
        out = []
        for size in b["sizes"]:
            if size == 0:
                out.append(torch.zeros(0, b["D"]))
                continue
            d0, d1, _ = O.make_descriptors(b["n0"], size, b["D"], b["seed"])
            if out:
                assert torch.equal(d0, out[0])
            else:
                out.append(d0)
            out.append(d1)
        _CACHE[key] = out if rootsift else [O.l2_rows(d) if d.shape[0] else d for d in out]
    return _CACHE[key]


def keypoints(name, i):
    key = ("kp", name)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(BANKS[name]["seed"])
        _CACHE[key] = [torch.rand(d.shape[0], 2, generator=g) * 640 for d in images(name)]
    return _CACHE[key][i]


def pooled_oracle(name, rootsift, ratio):
    """O.margins_f64 of every pair of the bank's list, the rows concatenated in list order: match0, score0, decidable, and pool = the
    rows that count in the pooled shares (all but those of a pair whose second image is empty: they can only be -1, and counting them
    would dilute the undecidable share; test_degenerate_pairs holds them)"""
    key = ("f64", name, bool(rootsift), float(ratio))
    if key not in _CACHE:
        imgs = images(name, rootsift)
        per = [O.margins_f64(imgs[i], imgs[j], rootsift, ratio) for i, j in PAIRS[name]]
        _CACHE[key] = {k: torch.cat([f[k] for f in per]) for k in ("match0", "score0", "decidable")}
        _CACHE[key]["pool"] = torch.cat([torch.full((imgs[i].shape[0],), imgs[j].shape[0] > 0) for i, j in PAIRS[name]])
    return _CACHE[key]
