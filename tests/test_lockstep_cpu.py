"""The device-solve lockstep driver of gim_amd/pose.py (`_lockstep_device`: one `_ransac_steps` generator per pair, one launch per
round for all of them, one mask call or `finish` at the end) without a GPU: a numpy stand-in takes the place of the step class
(`DeviceFundamental` / `DeviceEssential`), solving with pose.seven_point_ge / pose.five_point_ge -- the arithmetic of the kernels --
and counting with pose.sampson_error.  Every pair of a batch must then come out bit-equal to the single host call with solve="ge"."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import essential_cases as EC
import fundamental_cases as FC
from gim_amd import pose


class NumpyStep:
    """the interface of a step class over concatenated points and offsets [B + 1]: solve(idx [B, K, m]) -> (models [B, K, k, 3, 3],
    valid [B, K, k]), a row with an index of -1 left zero and invalid; counts of that launch; mask(models [B, 3, 3]) -> [Ptot]"""
    m = k = solver = None
    made = []                     # every object constructed, in order

    def __init__(self, x0, x1, thr2, device, offsets=None):
        assert device is None and offsets is not None and offsets[-1] == len(x0) == len(x1)
        self.x0, self.x1, self.thr2, self.offsets = x0, x1, thr2, offsets
        self.solve_calls = self.mask_calls = 0
        self.live = []            # per solve call: {pair: its real samples}, K
        type(self).made.append(self)

    def _pair(self, b):
        o = self.offsets
        return self.x0[o[b]:o[b + 1]], self.x1[o[b]:o[b + 1]]

    def solve(self, idx):
        self.solve_calls += 1
        B, K, m = idx.shape
        assert m == self.m and B == len(self.offsets) - 1 and idx.dtype == np.int32
        models, valid = np.zeros((B, K, self.k, 3, 3)), np.zeros((B, K, self.k), dtype=bool)
        self._counts = np.zeros((B, K, self.k), dtype=np.int64)
        self.live.append(({}, K))
        for b in range(B):
            rows = np.flatnonzero((idx[b] >= 0).all(1))
            if rows.size:
                self.live[-1][0][b] = rows.size
                a, c = self._pair(b)
                M, v = type(self).solver(a[idx[b, rows]], c[idx[b, rows]])
                models[b, rows], valid[b, rows] = M, v
                self._counts[b, rows] = np.where(v, (pose.sampson_error(M, a, c) <= self.thr2).sum(-1), 0)
        return models, valid

    def counts(self, Ms, valid):
        return self._counts

    def mask(self, M):
        self.mask_calls += 1
        assert M.shape == (len(self.offsets) - 1, 3, 3)
        return np.concatenate([pose.sampson_error(M[b], *self._pair(b)) <= self.thr2 for b in range(M.shape[0])])


class NumpyFundamental(NumpyStep):
    m, k, solver, made = 7, 3, staticmethod(pose.seven_point_ge), []


class NumpyEssential(NumpyStep):
    m, k, solver, made = 5, 10, staticmethod(pose.five_point_ge), []


class NoInliers(NumpyFundamental):
    """a step whose every count is 0: the run ends without a model"""
    made = []

    def counts(self, Ms, valid):
        return np.zeros_like(self._counts)


F_ARGS = dict(threshold=1.0, prob=0.999999, max_iters=10000, seed=2)
E_ARGS = dict(threshold=EC.THR, prob=0.999, max_iters=1000, seed=0)


@functools.lru_cache(maxsize=None)
def f_pairs():
    _, p0, p1, _ = FC.ransac_scene()
    return ((p0, p1), (p0[:6], p1[:6]), (p0[40:], p1[40:]), (p0[:0], p1[:0]))


@functools.lru_cache(maxsize=None)
def e_pairs():
    _, x0, x1, _ = EC.ransac_scene()
    return ((x0, x1), (x0[:4], x1[:4]), (x0[30:], x1[30:]))


def _same_as_single(got, pairs, single, inliers):
    assert len(got) == len(pairs)
    for (M, mask), (a, b), want_n in zip(got, pairs, inliers):
        M1, mask1 = single(a, b)
        assert (M is None) == (M1 is None) == (want_n is None)
        assert M is None or np.array_equal(M, M1)
        assert mask.dtype == bool and mask.shape == (len(a),) and np.array_equal(mask, mask1)
        assert int(mask.sum()) in (want_n or (0,))


@pytest.mark.parametrize("sampler", ("host", "philox"))
def test_fundamental_batch_is_the_single_ge_calls(sampler):
    pairs = f_pairs()
    got, dev = pose._lockstep_device(list(pairs), NumpyFundamental, F_ARGS["threshold"], F_ARGS["prob"], F_ARGS["max_iters"], F_ARGS["seed"],
                                     None, sampler)
    assert dev is NumpyFundamental.made[-1] and dev.mask_calls == 1
    _same_as_single(got, pairs, lambda a, b: pose.find_fundamental_mat(a, b, solve="ge", sampler=sampler, **F_ARGS),
                    ((180,), None, (159, 160), None))
    # more than one launch; the pairs without a sample are -1 throughout, and so is the tail of the shorter step of the last launch
    assert dev.solve_calls > 1 and dev.live[0] == ({0: 250, 2: 250}, 250)
    rows, K = dev.live[-1]
    assert set(rows) == {0, 2} and max(rows.values()) == K > min(rows.values())


@pytest.mark.parametrize("sampler", ("host", "philox"))
def test_essential_batch_is_the_single_ge_calls(sampler):
    pairs = e_pairs()
    got, dev = pose._lockstep_device(list(pairs), NumpyEssential, E_ARGS["threshold"], E_ARGS["prob"], E_ARGS["max_iters"], E_ARGS["seed"],
                                     None, sampler)
    assert dev is NumpyEssential.made[-1] and dev.mask_calls == 1
    _same_as_single(got, pairs, lambda a, b: pose.find_essential_mat(a, b, solve="ge", sampler=sampler, **E_ARGS), ((180,), None, (162,)))


def test_no_pair_with_a_sample_makes_no_step_object():
    _, p0, p1, _ = FC.ransac_scene()
    made = len(NumpyFundamental.made)
    got, dev = pose._lockstep_device([(p0[:6], p1[:6]), (p0[:0], p1[:0]), (p0[:3], p1[:3])], NumpyFundamental, 1.0, 0.999999, 10000, 2, None)
    assert dev is None and len(NumpyFundamental.made) == made
    assert [M for M, _ in got] == [None] * 3
    assert [mask.shape for _, mask in got] == [(6,), (0,), (3,)] and all(mask.dtype == bool and not mask.any() for _, mask in got)
    assert pose._lockstep_device([], NumpyFundamental, 1.0, 0.999999, 10000, 2, None) == ([], None)


def test_no_model_calls_neither_mask_nor_finish():
    pairs = f_pairs()
    calls = []
    got, dev = pose._lockstep_device(list(pairs), NoInliers, 1.0, 0.999999, 250, 2, None, finish=lambda *a: calls.append(a))
    assert dev is NoInliers.made[-1] and dev.solve_calls == 1 and dev.mask_calls == 0 and not calls
    assert [M for M, _ in got] == [None] * 4
    assert [mask.shape for _, mask in got] == [(len(a),) for a, _ in pairs] and not any(mask.any() for _, mask in got)


def test_finish_replaces_models_and_masks():
    pairs = f_pairs()
    Ptot = sum(len(a) for a, _ in pairs)
    plain, _ = pose._lockstep_device(list(pairs), NumpyFundamental, F_ARGS["threshold"], F_ARGS["prob"], F_ARGS["max_iters"], F_ARGS["seed"], None)
    calls = []
    new_masks = np.arange(Ptot) % 3 == 0

    def finish(dev, models):
        calls.append((dev, models.copy()))
        return models + 1.0, new_masks

    got, dev = pose._lockstep_device(list(pairs), NumpyFundamental, F_ARGS["threshold"], F_ARGS["prob"], F_ARGS["max_iters"], F_ARGS["seed"], None,
                                     finish=finish)
    assert len(calls) == 1 and calls[0][0] is dev and dev.mask_calls == 0
    sent = calls[0][1]
    assert sent.shape == (4, 3, 3) and not sent[1].any() and not sent[3].any()      # a pair without a model goes up as zeros
    offsets = np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs])])
    for b, ((M, mask), (M0, _)) in enumerate(zip(got, plain)):
        if M0 is None:
            assert M is None and not mask.any() and mask.shape == (len(pairs[b][0]),)
        else:
            assert np.array_equal(sent[b], M0) and np.array_equal(M, M0 + 1.0)
            assert np.array_equal(mask, new_masks[offsets[b]:offsets[b + 1]])


def test_importing_pose_leaves_torch_alone():
    """the device classes import torch and ops when one is constructed, not when the module is imported"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys, gim_amd.pose; assert 'torch' not in sys.modules and 'gim_amd.ops' not in sys.modules"
    assert subprocess.run([sys.executable, "-W", "error", "-c", code], cwd=root).returncode == 0
