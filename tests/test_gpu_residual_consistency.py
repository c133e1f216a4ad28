"""GPU test of the contract csrc/two_view_residual.h guarantees: for one model and one pair, the count of the step kernel that made
the model, the scorer's count, the MAGSAC count, the sum of the mask and the refit's starting count are the same integer -- one
residual and one inlier rule under all of them.  array_equal throughout.  Shapes: a ragged batch of three pairs with 65, 0 and 257
points and single pairs of 1, 63, 64 and 256 points, K = 3 samples per pair (a 64-point tile edge, a 256-lane pass edge, an empty
pair), and one call with K = 257 (a 256-model tile edge).  Inputs: the planted scenes of tests/fundamental_cases.py and
tests/homography_cases.py."""
import functools

import numpy as np
import pytest
import torch

import fundamental_cases as FC
import homography_cases as HC
from gim_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FOCAL, CENTRE = 500.0, np.array([320.0, 240.0])            # the camera of fundamental_cases
SHAPES = [((65, 0, 257), 3), ((1,), 3), ((63,), 3), ((64,), 3), ((256,), 3), ((256,), 257)]
# step -> (kind, sample size, models per sample, thr2)
STEPS = {"homography": (0, 4, 1, HC.THR2), "fundamental": (1, 7, 3, 1.0), "essential": (1, 5, 10, 1.0 / FOCAL ** 2)}


@functools.lru_cache(maxsize=None)
def _scene(step):
    """the 300 matches of the step's decidable scene and which of them are exact (the essential step takes them in normalised
    camera coordinates)"""
    if step == "homography":
        return HC.ransac_scene()[1:]
    _, p0, p1, truth = FC.ransac_scene()
    return ((p0 - CENTRE) / FOCAL, (p1 - CENTRE) / FOCAL, truth) if step == "essential" else (p0, p1, truth)


def _inputs(step, sizes, K):
    """the pairs' points cut from the scene (pair i starts 43 matches after pair i - 1), and K samples of distinct indices per pair:
    the first among the pair's exact matches (a valid model of many inliers), the others among all of them (outliers included:
    models of few inliers, refused samples); a pair with fewer points than a sample gets indices the kernel refuses"""
    m = STEPS[step][1]
    a, b, truth = _scene(step)
    rng = np.random.default_rng(1000 * len(sizes) + sizes[-1] + K)
    starts = [min(43 * i, len(a) - n) for i, n in enumerate(sizes)]
    x0 = np.concatenate([a[s:s + n] for s, n in zip(starts, sizes)])
    x1 = np.concatenate([b[s:s + n] for s, n in zip(starts, sizes)])
    idx = np.zeros((len(sizes), K, m), dtype=np.int32)
    for i, (s, n) in enumerate(zip(starts, sizes)):
        if n >= m:
            idx[i] = np.stack([rng.permutation(n)[:m] for _ in range(K)])
            idx[i, 0] = rng.permutation(np.flatnonzero(truth[s:s + n]))[:m]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return x0, x1, idx, offsets


@pytest.mark.parametrize("sizes,K", SHAPES)
@pytest.mark.parametrize("step", list(STEPS))
def test_every_count_of_a_model_is_one_integer(step, sizes, K):
    kind, m, k, thr2 = STEPS[step]
    x0, x1, idx, offsets = _inputs(step, sizes, K)
    B, single = len(sizes), len(sizes) == 1
    dx0, dx1 = torch.from_numpy(x0).to(DEV), torch.from_numpy(x1).to(DEV)
    doff = None if single else torch.from_numpy(offsets).to(DEV)
    didx = torch.from_numpy(idx[0] if single else idx).to(DEV)
    models, valid, counts = getattr(ops, step + "_step")(dx0, dx1, didx, thr2, offsets=doff)
    lead = (K * k,) if single else (B, K * k)
    models, valid = models.reshape(*lead, 3, 3).contiguous(), valid.reshape(lead).contiguous()
    step_counts = counts.reshape(B, K * k).cpu().numpy()
    ok = valid.reshape(B, K * k).cpu().numpy()
    for i, n in enumerate(sizes):
        assert ok[i].any() == (n >= m), (i, n)                # an exact scene: a pair that can be sampled gives models
    assert (step_counts[~ok] == 0).all()
    # the scorers: every model in one launch each
    _, ms = ops.magsac_score(kind, models, dx0, dx1, thr2, valid=valid, offsets=doff)
    assert np.array_equal(ms.reshape(B, K * k).cpu().numpy(), step_counts)
    if kind == 1:
        rs = ops.ransac_score(models, dx0, dx1, thr2, valid=valid, offsets=doff)
        assert np.array_equal(rs.reshape(B, K * k).cpu().numpy(), step_counts)
    # the mask and the refit take one model per pair: every slot that is valid in some pair
    mask_fn = ops.homography_mask if kind == 0 else ops.ransac_mask
    slots = np.flatnonzero(ok.any(0))
    sums, starts = [], []
    for j in slots:
        mj = (models[j] if single else models[:, j]).contiguous()
        sums.append(mask_fn(mj, dx0, dx1, thr2, offsets=doff))
        starts.append(ops.model_refit(kind, dx0, dx1, mj, thr2, mask=None, offsets=doff)[2].reshape(B, 2)[:, 0])
    if len(slots):
        sums = torch.stack(sums).cpu().numpy()                # [slots, Ptot]
        starts = torch.stack(starts).cpu().numpy()            # [slots, B]
        per_pair = np.stack([sums[:, offsets[i]:offsets[i + 1]].sum(1) for i in range(B)], 1)
        want = step_counts[:, slots].T
        sel = ok[:, slots].T
        assert np.array_equal(per_pair[sel], want[sel])
        assert np.array_equal(starts[sel], want[sel])
    n_valid = int(ok.sum())
    print(f"{step} sizes {sizes} K {K}: {n_valid} valid models, counts {step_counts[ok].min() if n_valid else 0} .. "
          f"{step_counts[ok].max() if n_valid else 0}")
