"""Oracle of the root_sift descriptor matcher: the five lines of the reference's root_sift_inference (trainer/lightning.py:215-226)
restated from their meaning on the CPU, in fp32 and in fp64, plus the fp64 margins that say which rows two correct fp32 evaluations
must agree on.

    desc = sqrt(desc / desc.sum(1))                      RootSIFT
    sim = desc0 @ desc1.T
    mutual = (sim == rowmax) & (sim == colmax);  valid, index = mutual.max(1)
    r = sqrt(2 - 2 top2(sim));  valid &= r[:, 0] / r[:, 1] < ratio
    score = rowmax

EPS is the parity budget: for unit-norm rows of D = 128 elements two correct fp32 evaluations of one dot product differ from the exact
value by at most D 2^-24 each, so from one another by 2 * 128 * 2^-24.  A row is DECIDABLE when none of its three decisions (which column
is the row maximum, whether that entry is the column maximum, which side of the ratio threshold) can change under a perturbation of EPS
of every similarity; on decidable rows every correct evaluation returns the same index.
"""
import numpy as np
import torch

EPS = 2 * 128 * 2.0 ** -24          # 1.53e-5
RATIO = 0.8
UNDECIDABLE_CAP = 0.02

# (n0, n1, D) of the GPU parity tests and the seed of each: partial row blocks, partial column tiles, both orders of n0 and n1, more than
# one row block and sweep step, the three ranges of D
CASES = [(1, 2, 128), (7, 5, 128), (257, 130, 128), (1000, 777, 128), (513, 1025, 256), (300, 300, 16)]
SEEDS = {c: 100 + i for i, c in enumerate(CASES)}


def sift_like(n, D, rng):
    """integer descriptors 0..255, non-negative, about half the bins empty: what cv2's SIFT returns"""
    d = rng.gamma(0.6, 40.0, size=(n, D))
    d[rng.random((n, D)) < 0.45] = 0.0
    d = np.clip(np.rint(d), 0, 255)
    d[np.arange(n), rng.integers(0, D, n)] += 1.0          # no all-zero row
    return np.minimum(d, 255).astype(np.float32)


def make_descriptors(n0, n1, D, seed):
    """desc0 [n0,D] SIFT-like; desc1 [n1,D] = a permuted subset of desc0 with integer noise, plus a second noisy copy ("twin") of a
    quarter of that subset -- repeated structure: the row still has a mutual nearest neighbour but two columns at nearly the same
    distance, so the ratio test rejects it -- plus unrelated rows.  Returns (desc0, desc1, truth [n0]: first planted column or -1)."""
    rng = np.random.default_rng(seed)
    desc0 = sift_like(n0, D, rng)
    m = min(max(1, int(0.7 * min(n0, n1))), n1)
    t = min(m // 4, n1 - m)
    src = rng.permutation(n0)[:m]
    src = np.concatenate([src, src[:t]])

    def noisy(rows, amp):
        noise = np.rint(rng.uniform(-1.0, 1.0, size=rows.shape) * amp)
        return np.clip(rows + noise * (rows > 0), 0, 255)

    amp = np.where(rng.random(m + t) < 0.75, 3, 12)[:, None]
    amp[:t], amp[m:] = 3, 3
    desc1 = np.concatenate([noisy(desc0[src], amp), sift_like(n1 - m - t, D, rng)], 0).astype(np.float32)
    perm = rng.permutation(n1)
    desc1 = desc1[perm]
    inv = np.empty(n1, dtype=np.int64)
    inv[perm] = np.arange(n1)
    truth = np.full(n0, -1, dtype=np.int64)
    truth[src[:m]] = inv[:m]
    return torch.from_numpy(desc0), torch.from_numpy(desc1), torch.from_numpy(truth)


def root_sift(desc):
    return (desc / desc.sum(dim=1, keepdim=True)).sqrt()


def l2_rows(desc):
    """unit-norm fp32 rows for the cases that run with rootsift off"""
    d = desc.double()
    return (d / d.norm(dim=1, keepdim=True)).float()


def nn_match(desc0, desc1, rootsift=True, ratio=RATIO, fp32=True):
    """The reference's lines on the CPU.  fp32=True evaluates like the reference (float32 throughout), False in float64.
    Returns (match0 int64 [n0] with -1 for no match, score0 [n0] = row maximum, sim)."""
    dt = torch.float32 if fp32 else torch.float64
    d0, d1 = desc0.to(dt), desc1.to(dt)
    if rootsift:
        d0, d1 = root_sift(d0), root_sift(d1)
    sim = d0 @ d1.t()
    n0, n1 = sim.shape
    if n0 == 0 or n1 == 0:
        return torch.full((n0,), -1, dtype=torch.int64), torch.zeros(n0, dtype=dt), sim
    rowmax = sim.max(dim=1, keepdim=True).values
    mutual = (sim == rowmax) & (sim == sim.max(dim=0, keepdim=True).values)
    valid, index = mutual.max(dim=1)
    if ratio > 0:
        if n1 < 2:
            valid = torch.zeros_like(valid)          # topk(2) raises in the reference: no second neighbour, no match
        else:
            top2 = torch.topk(sim, k=2, dim=1).values
            r = (-2 * top2 + 2).sqrt()
            valid = valid & ((r[:, 0] / r[:, 1]) < ratio)
    match0 = torch.where(valid, index, torch.full_like(index, -1))
    return match0, rowmax[:, 0], sim


def margins_f64(desc0, desc1, rootsift=True, ratio=RATIO, eps=EPS):
    """fp64 evaluation with the per-row margins of the three decisions.  Returns a dict of [n0] tensors:
      match0, score0     the fp64 answer
      row_margin         best - second best similarity of the row
      col_margin         |best - colmax[arg]| when they differ; when the row holds the column maximum, its lead over the column's second
                         value (the perturbation that would hand the column to another row)
      ratio_margin       |ratio value - ratio|
      decidable          row_margin > eps, col_margin > eps, and the interval of the ratio value under a perturbation of eps of both
                         similarities (propagated through sqrt(2 - 2 s) here) does not contain the threshold"""
    match0, score0, sim = nn_match(desc0, desc1, rootsift, ratio, fp32=False)
    n0, n1 = sim.shape
    inf = torch.full((n0,), float("inf"), dtype=torch.float64)
    if n1 < 2 or n0 == 0:
        col = inf.clone()
        if n1 == 1 and n0 > 1:
            s = sim[:, 0]
            top = torch.topk(s, 2).values
            col = torch.where(s == top[0], top[0] - top[1], top[0] - s)
        return {"match0": match0, "score0": score0, "row_margin": inf, "col_margin": col, "ratio_margin": inf,
                "decidable": col > eps}
    top2, arg2 = torch.topk(sim, k=2, dim=1)
    best, second, arg = top2[:, 0], top2[:, 1], arg2[:, 0]
    row_margin = best - second
    if n0 >= 2:
        ctop = torch.topk(sim, k=2, dim=0).values            # [2, n1]
        cmax, csec = ctop[0][arg], ctop[1][arg]
    else:
        cmax, csec = sim[0][arg], torch.full_like(best, -float("inf"))
    col_margin = torch.where(best == cmax, best - csec, cmax - best)
    u, w = 2 - 2 * best, 2 - 2 * second
    r = (u.clamp_min(0) / w).sqrt()
    if ratio > 0:
        r_lo = ((u - 2 * eps).clamp_min(0) / (w + 2 * eps)).sqrt()
        r_hi = ((u + 2 * eps) / (w - 2 * eps).clamp_min(1e-300)).sqrt()
        ratio_ok = (ratio < r_lo) | (ratio > r_hi)
        ratio_margin = (r - ratio).abs()
    else:
        ratio_ok = torch.ones_like(best, dtype=torch.bool)
        ratio_margin = inf
    decidable = (row_margin > eps) & (col_margin > eps) & ratio_ok
    return {"match0": match0, "score0": score0, "row_margin": row_margin, "col_margin": col_margin, "ratio_margin": ratio_margin,
            "decidable": decidable}


_CACHE = {}


def case(n0, n1, D, rootsift, ratio=RATIO):
    """inputs + fp32 / fp64 oracle results of one test case, computed once and shared (read-only) by the tests that need them.
    With rootsift off the descriptors are the unit-norm rows the parity budget speaks of."""
    key = (n0, n1, D, bool(rootsift), float(ratio))
    if key not in _CACHE:
        desc0, desc1, truth = make_descriptors(n0, n1, D, SEEDS[(n0, n1, D)])
        if not rootsift:
            desc0, desc1 = l2_rows(desc0), l2_rows(desc1)
        m32, s32, _ = nn_match(desc0, desc1, rootsift, ratio, fp32=True)
        _CACHE[key] = {"desc0": desc0, "desc1": desc1, "truth": truth, "match32": m32, "score32": s32,
                       "f64": margins_f64(desc0, desc1, rootsift, ratio)}
    return _CACHE[key]
