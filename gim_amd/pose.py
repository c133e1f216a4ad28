"""Robust two-view geometry on the host without OpenCV (numpy, batched minimal solvers).

The reference calls OpenCV for the pose half of its metric and for the demo's geometry filter:
  * tools/metrics.py:77-103   cv2.findEssentialMat(RANSAC, threshold, prob) + cv2.recoverPose(E, ..., 1e9, mask)
  * demo.py:514-517           cv2.findFundamentalMat(USAC_MAGSAC, 1.0 px, 0.999999, 10000)
OpenCV (`opencv-python`, a pip dependency of the reference, not vendored under /root/reference) is absent from the build
container and from the GPU boxes, so `gim_amd.zeb.estimate_pose` / `gim_amd.demo` could not run their robust-fitting step at
all.  north_star keeps RANSAC on the host; this module is that host step when cv2 does not import (cv2 stays the first choice
when it does: `GIM_POSE_BACKEND=auto|cv2|numpy`).

What is restated (OpenCV 4.x, modules/calib3d/src/five-point.cpp and ptsetreg.cpp, published algorithms):
  * five-point essential matrix (Nister 2004 in the Stewenius-Engels-Nister 2006 formulation): null space of the 5 x 9
    epipolar constraints, the ten cubic constraints det(E) = 0 and 2 E E^T E - tr(E E^T) E = 0 on E = xX + yY + zZ + W,
    Gauss-Jordan on the 10 x 20 coefficient matrix, 10 x 10 action matrix of multiplication by x, real eigenvectors
    -> up to 10 candidates;
  * RANSAC as `RANSACPointSetRegistrator::run`: 5-point samples, Sampson error (x1^T E x0)^2 / (|E x0|_xy^2 + |E^T x1|_xy^2)
    against threshold^2, the model with the most inliers wins, the iteration bound shrinks with
    log(1 - conf) / log(1 - w^5) (at most 1000 iterations, cv2.findEssentialMat's default maxIters), NO final re-fit;
  * `recoverPose`: SVD decomposition into (R1 | R2, +-t), DLT triangulation of the masked points, the candidate with the most
    points in front of both cameras (depth < distanceThresh) wins; its count is returned.
  * seven-point fundamental matrix inside the same RANSAC loop for the demo (plain RANSAC with the Sampson distance in pixels by
    default; the inlier mask is RANSAC's, which is what the demo prints and draws).
  * `score="magsac"`: the MAGSAC++ loss (Barath et al., CVPR 2020) that the reference's cv2.USAC_MAGSAC calls name, as a scoring
    mode of the F and H loops -- the closed form for 4 degrees of freedom and k = 3.64 (`magsac_gain`), quantised per point and
    summed in int64 (`magsac_quality`; csrc/ransac_score.hip on the device).  Not cv2's bytes, no sigma-consensus polish, not for E.
  * four-point homography inside the same loop for the demo's warp (demo.py:180-227 cv2.findHomography; fundam.cpp): forward transfer
    error, re-fit on the inliers by normalised DLT, no Levenberg-Marquardt polish.  This solver also runs on the device, fused with
    the scoring (`find_homography(device=)`, csrc/homography.hip): a step uploads sample indices only.
  * the seven-point solver by elimination and a closed-form cubic (`seven_point_ge`), the arithmetic of the device step that solves
    and scores in one launch (`find_fundamental_mat(solve="device")`, `find_fundamental_mat_batch`, `verify_pairs`;
    csrc/fundamental.hip).  `seven_point` and the default path are unchanged.
  * the five-point solver by elimination and a real QR iteration (`five_point_ge`), the arithmetic of the device step that solves
    and scores in one launch (`find_essential_mat(solve="device")`, `find_essential_mat_batch(solve="device")`; csrc/essential.hip).
    `five_point` and the default path are unchanged.
  * `sampler=`: who draws the samples.  "host" (the default) is numpy's default_rng, as ever.  "philox" is a counter-based draw
    (`device_samples`: Philox4x32-10 words, Floyd's m distinct indices) made on the host; "device" makes the same draw on the GPU
    (csrc/ransac_sample.hip) and reduces every step there to the samples that set a new best count (csrc/ransac_records.hip,
    `step_records`): nothing of a step is read back but those records and the 72 bytes of a newly best model.  Same seed, same
    device: "device" and "philox" give the same model bytes and mask.  Neither walks the trajectory of "host".

Parity: UNPINNED against cv2 (no OpenCV here to record vectors from; sampling is random in both).  tests/test_pose_cpu.py pins
the solvers on exact synthetic geometry (every ground-truth E / F is among the candidates to 1e-9, recovered poses within 1e-6
of the truth on noise-free data, sub-degree on noisy data with 50 % outliers) and compares with cv2 under `importorskip`.
Batched numpy: 250 samples (2 500 candidate models) are solved and scored per step.  Scoring was most of a step, and it can run on
the GPU (`device=` / `DeviceScorer`, csrc/ransac_score.hip; sampling, the iteration bound and recover_pose stay here, and so do
the solvers unless `solve="device"` is asked for; the result for a seed is then the host's).  Measured on one MI355X box (tools/bench_pose.py, profiles/r12_pose_score.txt; 2 000
matches, 50 % outliers): one scoring step 53.6 ms on the host against 0.23 ms on the device, estimate_pose 242 ms per pair on the
host against 53 ms with `device=`.
"""
import collections
import os

import numpy as np

from .pose_math import _check_seed64, _count_inliers, _epipolar_rows, _triangulate  # noqa: F401  (the last three also for callers of `pose._<name>` from before the split)
from .pose_math import *  # noqa: F401,F403  (every public name of the maths, solvers and constants, stays reachable as pose.<name>)


class _DevicePoints:
    """The matched points of one pair, or of several pairs concatenated with `offsets` [B + 1], uploaded once as fp64 [P, 2] and kept
    on `device` for every later call.  A subclass names its mask op (looked up on `ops` at call time) and its refit kind.
    max_thr2 (score="magsac"): the squared band of gim_magsac_score."""
    _mask, _kind = "ransac_mask", 1          # the Sampson error; gim_model_refit's fundamental matrices in pixels

    def __init__(self, x0, x1, thr2, device, offsets=None, max_thr2=None):
        import torch
        from . import ops
        self._torch, self._ops = torch, ops
        self.device = torch.device(device)
        self.thr2, self.max_thr2 = float(thr2), max_thr2
        with torch.cuda.device(self.device):
            self.x0, self.x1 = self._up(x0, np.float64), self._up(x1, np.float64)
            self.offsets = None if offsets is None else self._up(offsets, np.int32)

    def _up(self, a, dtype):
        return self._torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def mask(self, M):
        """one model [3, 3], or with offsets one per pair [B, 3, 3] -> the inlier mask bool [Ptot]"""
        with self._torch.cuda.device(self.device):
            return getattr(self._ops, self._mask)(self._up(M, np.float64), self.x0, self.x1, self.thr2, offsets=self.offsets).cpu().numpy()

    def refit(self, M, rounds=1):
        """gim_model_refit (ops.model_refit) over the points and offsets held here, from the models' own masks: M [3,3] / [B,3,3]
        -> numpy (models [B,3,3], mask bool [Ptot], counts [B,2], accepted [B]); ONE copy brings all four back"""
        torch = self._torch
        with torch.cuda.device(self.device):
            d_M = self._up(M, np.float64)
            models, mask, counts, accepted = self._ops.model_refit(self._kind, self.x0, self.x1, d_M, self.thr2, offsets=self.offsets, rounds=rounds)
            B = 1 if self.offsets is None else d_M.shape[0]
            down = torch.cat([models.reshape(-1).view(torch.uint8), torch.cat([counts.reshape(B, 2), accepted.reshape(B, 1)], 1).reshape(-1).view(torch.uint8),
                              mask.view(torch.uint8)]).cpu().numpy()
        ca = down[72 * B:84 * B].view(np.int32).reshape(B, 3)
        return down[:72 * B].view(np.float64).reshape(B, 3, 3).copy(), down[84 * B:].view(bool).copy(), ca[:, :2].copy(), ca[:, 2].copy()


class DeviceScorer(_DevicePoints):
    """The scoring half of a RANSAC step on the GPU (csrc/ransac_score.hip through ops.ransac_score / ops.ransac_mask): every step
    uploads its candidate models and reads the counts back, the final mask is one more call.  Same fp64 arithmetic as
    `sampson_error`, so a RANSAC run scored here walks the trajectory of the host run with the same seed.
    One pair: models [K, 3, 3] / valid [K].  Several pairs in lockstep (`find_essential_mat_batch`): models [B, K, 3, 3] / valid [B, K]."""

    def counts(self, Ms, valid):
        with self._torch.cuda.device(self.device):
            c = self._ops.ransac_score(self._up(Ms, np.float64), self.x0, self.x1, self.thr2, valid=self._up(valid, np.uint8), offsets=self.offsets)
            return c.cpu().numpy().astype(np.int64)

    def quality(self, Ms, valid):
        """score="magsac": (qualities, counts) of uploaded models through ops.magsac_score, shaped like `counts`"""
        with self._torch.cuda.device(self.device):
            q, c = self._ops.magsac_score(self._kind, self._up(Ms, np.float64), self.x0, self.x1, self.thr2, self.max_thr2,
                                          valid=self._up(valid, np.uint8), offsets=self.offsets)
            return q.cpu().numpy(), c.cpu().numpy().astype(np.int64)


class _DeviceStep(_DevicePoints):
    """A whole RANSAC step on the GPU: a step uploads only its sample indices and reads back the models, flags and counts of ONE
    launch that solves and scores.  A subclass declares m (points per sample), k (models per sample) and the name of its step op.
    `solve` is the `solve_idx` hook of `_ransac_steps`, `counts` / `mask` the scorer interface of `_ransac` (the counts are those of
    the launch that made the models).  One pair: idx [K, m].  Several pairs in lockstep: idx [B, K, m] relative to each pair (an
    index of -1 marks padding: invalid)."""
    _counts = None

    def solve(self, idx):
        """idx [..., m] -> (models [..., k, 3, 3], valid [..., k]) on the host"""
        lead = np.shape(idx)[:-1] + (self.k,)
        with self._torch.cuda.device(self.device):
            models, valid, counts = getattr(self._ops, self._step)(self.x0, self.x1, self._up(idx, np.int32), self.thr2, offsets=self.offsets)
            self._resident = (models, valid)                                  # for `quality`: the step's models stay where they are
            self._counts = counts.cpu().numpy().astype(np.int64).reshape(lead)
            return models.cpu().numpy().reshape(lead + (3, 3)), valid.cpu().numpy().reshape(lead)      # homography_step has no k axis

    def counts(self, Ms, valid):
        return self._counts.reshape(-1) if self.offsets is None else self._counts

    def quality_on_device(self, models, valid):
        """gim_magsac_score over models and flags the device holds (any leading shape; with offsets the first axis is the pair)
        -> (quality int64, counts int32) of B * K * k entries on the device"""
        lead = (-1,) if self.offsets is None else (models.shape[0], -1)
        return self._ops.magsac_score(self._kind, models.reshape(*lead, 3, 3), self.x0, self.x1, self.thr2, self.max_thr2,
                                      valid=valid.reshape(*lead), offsets=self.offsets)

    def quality(self, Ms, valid):
        """score="magsac": the scorer interface of `_ransac` -- (qualities, counts) of the models the last `solve` left on the
        device, shaped like `counts`; the step's own counts are not used"""
        with self._torch.cuda.device(self.device):
            q, c = self.quality_on_device(*self._resident)
            q, c = q.cpu().numpy().reshape(self._counts.shape), c.cpu().numpy().astype(np.int64).reshape(self._counts.shape)
        return (q.reshape(-1), c.reshape(-1)) if self.offsets is None else (q, c)

    def step_on_device(self, idx, flags=False):
        """the step's launch alone, for `_ransac_on_device`: idx int32 [B, K, m] on the device -> (models, counts int32) of
        B * K * k entries on the device -- flags=True: (models, valid) instead; nothing is read back"""
        models, valid, counts = getattr(self._ops, self._step)(self.x0, self.x1, idx, self.thr2, offsets=self.offsets)
        return (models, valid) if flags else (models, counts)


class DeviceFundamental(_DeviceStep):
    """The fundamental-matrix step (csrc/fundamental.hip through ops.fundamental_step; the mask through ops.ransac_mask, the same
    Sampson error): points in pixels, up to three models per sample."""
    _step = "fundamental_step"
    m, k = 7, 3


class DeviceHomography(_DeviceStep):
    """The homography step (csrc/homography.hip through ops.homography_step / ops.homography_mask, the forward transfer error):
    dst ~ H src in pixels, one model per sample; the points are held as `x0` (src) and `x1` (dst)."""
    _step, _mask, _kind = "homography_step", "homography_mask", 0
    m, k = 4, 1


class DeviceEssential(_DeviceStep):
    """The essential-matrix step (csrc/essential.hip through ops.essential_step; the mask through ops.ransac_mask): points in
    normalised camera coordinates, up to ten models per sample.
    recover=True: `mask` also runs recoverPose on the points held here (`recover`: gim_recover_pose takes gim_ransac_mask's output
    where it lies) and brings the RANSAC mask, R, t, the four counts and the winner back in ONE copy; the poses are left in
    `self.poses` = (n_good [B, 4], best [B], R [B, 3, 3], t [B, 3]) as numpy arrays (B = 1 for a single pair)."""
    _step = "essential_step"
    m, k = 5, 10

    def __init__(self, x0, x1, thr2, device, offsets=None, recover=False, distance_thresh=1e9, max_thr2=None):
        super().__init__(x0, x1, thr2, device, offsets, max_thr2)
        self.recover_too, self.distance_thresh, self.poses = bool(recover), float(distance_thresh), None

    def refit(self, M, rounds=1):
        raise TypeError("essential matrices are not refitted (cv2.findEssentialMat(RANSAC) does not either)")

    def recover(self, models, masks=None):
        """gim_recover_pose over the points and offsets held here: models fp64 [3,3] / [B,3,3] and masks bool / uint8 [Ptot] (or
        None) on the device -> ops.recover_pose's tensors, on the device"""
        return self._ops.recover_pose(models, self.x0, self.x1, mask=masks, offsets=self.offsets, distance_thresh=self.distance_thresh)

    def mask(self, M):
        if not self.recover_too:
            return super().mask(M)
        torch = self._torch
        with torch.cuda.device(self.device):
            d_M = self._up(M, np.float64)
            d_mask = self._ops.ransac_mask(d_M, self.x0, self.x1, self.thr2, offsets=self.offsets)
            n_good, best, R, t, _ = self.recover(d_M, d_mask)
            B = 1 if self.offsets is None else d_M.shape[0]
            # one copy: [R | t] as bytes, [n_good | best] as bytes, the mask
            down = torch.cat([torch.cat([R.reshape(B, 9), t.reshape(B, 3)], 1).reshape(-1).view(torch.uint8),
                              torch.cat([n_good.reshape(B, 4), best.reshape(B, 1)], 1).reshape(-1).view(torch.uint8),
                              d_mask.view(torch.uint8)]).cpu().numpy()
        Rt = down[:96 * B].view(np.float64).reshape(B, 12)
        nb = down[96 * B:116 * B].view(np.int32).reshape(B, 5)
        self.poses = (nb[:, :4].copy(), nb[:, 4].copy(), Rt[:, :9].reshape(B, 3, 3).copy(), Rt[:, 9:].copy())
        return down[116 * B:].view(bool).copy()

    def pose_of(self, b=0):
        """(n_good of the winner, R, t) of pair b after `mask`; an invalid model: (0, zero R, zero t)"""
        n_good, best, R, t = self.poses
        return (int(n_good[b, best[b]]) if best[b] >= 0 else 0), R[b], t[b]


# ---- the arguments the entry points share: each rule is written once and raises before anything is uploaded or launched -------------
SAMPLERS = ("host", "philox", "device")
SCORES = ("count", "magsac")
REFITS = ("host", "device", "ge")
RECOVERS = ("host", "device")
RECORDS_FIRST_COPY = 32      # records per pair that the first device-to-host copy of a step carries


def _check_solve(solve, device, allowed=("host", "device", "ge")):
    """the `solve=` rules, `allowed` the names this entry point takes"""
    if solve not in allowed:
        raise ValueError(f"solve={solve!r}: {' or '.join(allowed)}")
    if solve == "device" and device is None:
        raise ValueError("solve='device' needs a device")
    if solve == "ge" and device is not None:
        raise ValueError("solve='ge' runs on the host: device must be None")


def check_sampler(sampler, device, solve="device"):
    """the `sampler=` rules"""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler={sampler!r}: host, philox or device")
    if sampler == "device" and (device is None or solve != "device"):
        raise ValueError("sampler='device' draws and reduces on the GPU: it needs a device" + ("" if solve == "device" else " and solve='device'"))


def check_recover(recover, device):
    """the `recover=` rules"""
    if recover not in RECOVERS:
        raise ValueError(f"recover={recover!r}: host or device")
    if recover == "device" and device is None:
        raise ValueError("recover='device' runs gim_recover_pose: it needs a device")


def check_refit(refit, device):
    """the `refit=` rules of find_homography"""
    if refit not in REFITS:
        raise ValueError(f"refit={refit!r}: host, device or ge")
    if refit == "device" and device is None:
        raise ValueError("refit='device' runs gim_model_refit: it needs a device")
    if refit == "ge" and device is not None:
        raise ValueError("refit='ge' runs on the host: device must be None")


def _check_refine(refine):
    refine = int(refine)
    if not 0 <= refine <= MR_MAX_ROUNDS:
        raise ValueError(f"refine={refine}: 0 (none) or 1 .. {MR_MAX_ROUNDS} rounds")
    return refine


def _check_score(score, sampler, threshold, max_threshold):
    """the `score=` / `max_threshold=` rules shared by the entry points; raises before anything is launched
    -> None for score="count", else max_threshold^2 (max_threshold defaults to threshold)"""
    if score not in SCORES:
        raise ValueError(f"score={score!r}: count or magsac")
    if score == "count":
        if max_threshold is not None:
            raise ValueError("max_threshold belongs to score='magsac'")
        return None
    if sampler == "host":
        raise ValueError("score='magsac' takes sampler='philox' or sampler='device' (the default_rng path has no quality walk)")
    mt = float(threshold if max_threshold is None else max_threshold)
    if not (np.isfinite(mt) and mt > 0.0):
        raise ValueError(f"max_threshold={mt}: finite and positive")
    return mt * mt


class _Walk:
    """The bookkeeping of RANSACPointSetRegistrator::run for one pair, and the only place where its acceptance test, its bound
    update and its break condition are written: the best count (and quality) so far, the shrinking bound `niters`, the samples
    consumed.  `plan` says how many samples the next step takes (0: the run is over) and the floor a sample has to beat; `offer`
    takes a candidate of that step -- sample s (ascending), its best slot j, that slot's count c -- and `close` ends the step.
    `_ransac_steps` offers every sample of a step, `_ransac_on_device` (through `replay`) only a step's records, the samples above
    every earlier one of their step: the walk accepts exactly those of them that it reaches (a record beyond the break point,
    s > niters - done - 1, is ignored), so both end on the same sample, the same bound and the same number of samples consumed.
    quality=True: the walk of score="magsac".  The floor is the best quality so far (0 at the start); a candidate carries the
    quality q of its slot, is eligible iff c >= m and accepted iff q is strictly above the floor; the bound is updated with c."""

    def __init__(self, P, m, conf, max_iters, batch=250, quality=False):
        self.P, self.m, self.batch = int(P), int(m), int(batch)
        self.lconf = np.log(max(1.0 - conf, 1e-300))
        self.best_n, self.niters, self.done, self.nb = 0, int(max_iters), 0, 0
        self.quality, self.best_q = bool(quality), 0

    def plan(self):
        self.nb = max(0, min(self.batch, self.niters - self.done))
        return self.nb, (self.best_q if self.quality else max(self.best_n, self.m - 1))

    def offer(self, s, j, c, q=0):
        """-> True: accepted, the new best; False: not; None: the walk ended before sample s (the bound shrank below it)"""
        if s >= self.nb or self.done + s >= self.niters:
            return None
        if not ((c >= self.m and q > self.best_q) if self.quality else c > max(self.best_n, self.m - 1)):
            return False
        self.best_n, self.best_q = c, q
        den = 1.0 - (c / self.P) ** self.m
        self.niters = min(self.niters, self.done + s + 1 if den < 1e-12 else max(self.done + s + 1, int(np.ceil(self.lconf / np.log(den)))))
        return True

    def close(self):
        self.done += self.nb

    def replay(self, records):
        """a whole step from its records, int [n_rec, 3] (s, j, c) or [n_rec, 4] (s, j, c, Q) -> the (s, j) of the last one accepted | None"""
        last = None
        for rec in records.tolist():
            hit = self.offer(*rec)
            if hit is None:
                break
            if hit:
                last = (rec[0], rec[1])
        self.close()
        return last


def _ransac_steps(P, solver, m, conf, max_iters, rng, s0, s1, batch=250, solve_idx=None, draw=None, quality=False):
    """The sampling / solving half of RANSACPointSetRegistrator::run as a generator (the bookkeeping is a `_Walk`): every step yields its candidate
    models (Ms [nb * k, 3, 3], valid [nb * k]) and is sent their inlier counts [nb * k]; the generator's return value is the best
    model [3, 3] or None.  Who counts (the host, a device, one launch for many pairs in lockstep) is the driver's business.
    solve_idx: a hook that receives the step's sample indices idx [nb, m] and returns (Ms [nb, k, 3, 3], valid [nb, k]) in place of
    solver(s0[idx], s1[idx]) -- a solver that lives where the points already are (`_DeviceStep.solve`).  The
    arrays it returns are read only after the counts have been sent, so a lockstep driver may hand out empty ones and fill them in
    place from one launch for many pairs (`_lockstep_device`).
    draw: None draws from `rng` as ever; otherwise draw(first, nb) -> the samples number first .. first + nb - 1 of the run
    (sampler="philox": `device_samples`) and `rng` is not used.
    quality=True (score="magsac"): a step is sent (qualities [nb * k], counts [nb * k]) instead; a slot is eligible iff its count
    is at least m, a sample's quality is the largest of its eligible slots' (the lowest such slot), it is accepted iff that is
    strictly above the best so far (0 at the start), and the bound is updated with the accepted slot's count."""
    walk = _Walk(P, m, conf, max_iters, batch, quality)
    best_M = None
    while True:
        nb, _ = walk.plan()
        if nb == 0:
            return best_M
        # m distinct indices per sample: the m smallest of P random keys
        if draw is not None:
            idx = draw(walk.done, nb)
        else:
            idx = np.argsort(rng.random((nb, P)), axis=1)[:, :m] if P <= 4096 else \
                np.stack([rng.choice(P, m, replace=False) for _ in range(nb)])
        Ms, valid = solver(s0[idx], s1[idx]) if solve_idx is None else solve_idx(idx)
        k = Ms.shape[1]
        Ms = Ms.reshape(-1, 3, 3)
        sent = yield Ms, valid.reshape(-1)
        # a sample's slot: the most inliers, or the largest quality among the slots of at least m inliers; the lowest slot on ties
        if quality:
            per = np.asarray(sent[1]).reshape(nb, k)
            key = np.where(per >= m, np.asarray(sent[0], dtype=np.int64).reshape(nb, k), 0)
        else:
            per = key = sent.reshape(nb, k)
        slot, rows = key.argmax(1), np.arange(nb)
        # walk the batch in sample order so that the shrinking iteration bound behaves like the sequential loop
        for s, (j, c, q) in enumerate(zip(slot.tolist(), per[rows, slot].tolist(), key[rows, slot].tolist())):
            hit = walk.offer(s, j, c, q)
            if hit is None:
                break
            if hit:
                best_M = Ms[s * k + j]
        walk.close()


def _draw(sampler, seed, P, m):
    """the `draw` hook of `_ransac_steps` for a `sampler`: None for "host" (default_rng), otherwise `device_samples` under `seed`"""
    if sampler == "host":
        return None
    seed = _check_seed64(seed)
    return lambda first, nb: device_samples(seed, first, nb, P, m)


def _ransac(x0, x1, solver, m, thr, conf, max_iters, rng, s0=None, s1=None, batch=250, scorer=None, solve_idx=None, error=None,
            draw=None, max_thr2=None, kind=1):
    """RANSACPointSetRegistrator::run with `solver` on samples of m points; the error is evaluated on (x0, x1), the solver sees
    (s0, s1) when given (normalised copies of the same points).  `scorer`: None counts inliers and takes the final mask on the host
    (`_count_inliers`, `sampson_error`); otherwise an object with counts(Ms [K,3,3], valid [K]) -> int64 [K] and
    mask(M [3,3]) -> bool [P] over the same points and threshold (`DeviceScorer`).  solve_idx: the hook of `_ransac_steps`.
    error: the host error in place of `sampson_error`, error(Ms [..., 3, 3], x0, x1) -> [..., P] (`transfer_error`).
    draw: the sampling hook of `_ransac_steps` (`_draw`).
    max_thr2: None ranks the models by their inlier counts; a number runs the quality walk of `_ransac_steps` over
    `magsac_quality` under that band (score="magsac"), or over scorer.quality(Ms, valid) -> (int64 [K], int64 [K]).
    kind: `magsac_quality`'s, for the host scoring of that walk -- 1 with `sampson_error`, 0 with `transfer_error`.
    -> (model [3,3] or None, mask [P] bool)"""
    P = x0.shape[0]
    if P < m:
        return None, np.zeros(P, dtype=bool)
    s0 = x0 if s0 is None else s0
    s1 = x1 if s1 is None else s1
    thr2 = float(thr) ** 2
    steps = _ransac_steps(P, solver, m, conf, max_iters, rng, s0, s1, batch, solve_idx, draw, quality=max_thr2 is not None)
    error = sampson_error if error is None else error
    try:
        Ms, valid = next(steps)
        while True:
            if max_thr2 is not None:       # (qualities, counts)
                scores = magsac_quality(kind, Ms, valid, x0, x1, thr2, max_thr2) if scorer is None else scorer.quality(Ms, valid)
            else:                          # counts
                scores = _count_inliers(Ms, valid, x0, x1, thr2, error=error) if scorer is None else scorer.counts(Ms, valid)
            Ms, valid = steps.send(scores)
    except StopIteration as stop:
        best_M = stop.value
    if best_M is None:
        return None, np.zeros(P, dtype=bool)
    return best_M, (error(best_M, x0, x1) <= thr2) if scorer is None else scorer.mask(best_M)


def find_essential_mat(x0, x1, threshold, prob=0.999, max_iters=1000, seed=0, device=None, solve="host", sampler="host"):
    """cv2.findEssentialMat(x0, x1, eye(3), method=RANSAC, prob, threshold) on normalised points -> (E [3,3] | None, mask [P]).
    solve="host": `five_point` (SVD null space, a linear solve, LAPACK's eigenvectors); device: score the candidates on that GPU
    (`DeviceScorer`); same trajectory, model and mask as the host run of the same seed.
    solve="device" (needs `device`): the same indices are drawn on the host and uploaded; models, flags and counts come from one
    gim_essential_step per step (`DeviceEssential`: elimination and a real QR iteration; it rounds differently from `five_point`,
    so its trajectory need not be the host's), the mask from gim_ransac_mask.
    solve="ge" (host only): the same RANSAC over `five_point_ge`, the numpy restatement of the device solver -- its CPU oracle.
    sampler: "host" draws from default_rng(seed) (the default; every seeded result so far); "philox" draws `device_samples` on the
    host, with any `solve` (with solve="ge" it is the CPU oracle of the next); "device" (needs `device` and solve="device") draws
    on the GPU and reads back only each step's record samples (`_ransac_on_device`): same model bytes and mask as "philox" there."""
    _check_solve(solve, device)
    check_sampler(sampler, device, solve)
    return _run_pair(_E, *_points64(x0, x1), threshold, prob, max_iters, seed, device, solve, sampler)[:2]


def find_essential_pose(x0, x1, threshold, prob=0.999, max_iters=1000, seed=0, device=None, solve="host", sampler="host",
                        distance_thresh=1e9):
    """`find_essential_mat` followed by recoverPose ON `device` (needs one) -> (E | None, mask, (n_good, R, t) | None): E and the
    RANSAC mask are find_essential_mat's of the same arguments.  solve="device": gim_recover_pose runs on the points the RANSAC
    left on the device, on gim_ransac_mask's output where it lies, and ONE copy brings the mask, R, t and the counts back
    (`DeviceEssential(recover=True)`).  solve="host": E, the points and the mask are uploaded for the recover alone
    (`recover_pose(device=)`).  Without a model nothing is launched for the recover."""
    check_recover("device", device)
    _check_solve(solve, device)
    check_sampler(sampler, device, solve)
    x0, x1 = _points64(x0, x1)
    E, mask, dev = _run_pair(_E, x0, x1, threshold, prob, max_iters, seed, device, solve, sampler,
                             step_kw=dict(recover=True, distance_thresh=distance_thresh))
    if E is None:
        return None, mask, None
    if solve == "device":
        return E, mask, dev.pose_of(0)
    return E, mask, recover_pose(E, x0, x1, distance_thresh, mask=mask, device=device)[:3]


def find_essential_pose_batch(pairs, threshold, prob=0.999, max_iters=1000, seed=0, device=None, solve="host", sampler="host",
                              distance_thresh=1e9):
    """`find_essential_mat_batch` followed by recoverPose ON `device` for every pair with a model, in ONE gim_recover_pose launch ->
    [(E | None, mask, (n_good, R, t) | None)]; a pair's result is find_essential_pose's.  solve="device": the launch runs on the
    lockstep run's points and mask (one copy for the batch); solve="host": the pairs with a model are uploaded for it."""
    check_recover("device", device)
    pairs, _ = _pairs64(pairs)
    _check_solve(solve, device, ("host", "device"))
    check_sampler(sampler, device, solve)
    found, dev = _run_batch(_E, pairs, threshold, prob, max_iters, seed, device, solve, sampler,
                            step_kw=dict(recover=True, distance_thresh=distance_thresh))
    if solve == "device":
        return [(E, mask, dev.pose_of(b) if E is not None else None) for b, (E, mask) in enumerate(found)]
    have = [b for b, (E, _) in enumerate(found) if E is not None]
    out = [(E, mask, None) for E, mask in found]
    if have:
        import torch
        from . import ops
        offsets = np.concatenate([[0], np.cumsum([pairs[b][0].shape[0] for b in have])]).astype(np.int32)
        with torch.cuda.device(torch.device(device)):
            up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(device)   # noqa: E731  (a copy: `a` may be read-only)
            n_good, best, R, t, _ = ops.recover_pose(up(np.stack([found[b][0] for b in have]), np.float64),
                                                     up(np.concatenate([pairs[b][0] for b in have]), np.float64),
                                                     up(np.concatenate([pairs[b][1] for b in have]), np.float64),
                                                     mask=up(np.concatenate([found[b][1] for b in have]), np.uint8), offsets=up(offsets, np.int32),
                                                     distance_thresh=distance_thresh)
            n_good, best, R, t = n_good.cpu().numpy(), best.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()
        for i, b in enumerate(have):
            out[b] = found[b] + (((int(n_good[i, best[i]]) if best[i] >= 0 else 0), R[i], t[i]),)
    return out


def find_essential_mat_batch(pairs, threshold, prob=0.999, max_iters=1000, seed=0, device=None, scorer=None, solve="host", sampler="host"):
    """`find_essential_mat(x0, x1, threshold, prob, max_iters, seed)` for every (x0, x1) of `pairs`, run in lockstep (`_lockstep`): a
    round solves the samples of every unfinished pair on the host and scores all of them in ONE launch (ragged point sets through
    offsets), and one mask call for all pairs ends the run (`_batch_results`); a pair's result is that of the single call.
    scorer: an object like DeviceScorer over the concatenated points (counts(models [B,K,3,3], valid [B,K]) -> [B,K],
    mask(models [B,3,3]) -> bool [Ptot]); default DeviceScorer on `device`; neither: the pairs run one by one on the host.
    solve="device" (needs `device`, takes no `scorer`): `_lockstep_device` with `DeviceEssential`, ONE gim_essential_step launch
    per round; a pair's result is that of find_essential_mat(..., device=device, solve="device").
    sampler: as in find_essential_mat, every pair's ordinals running from 0 under the shared seed ("device" needs solve="device").
    -> [(E [3,3] | None, mask [P_b] bool)] in the order of `pairs`."""
    _check_solve(solve, device, ("host", "device"))
    check_sampler(sampler, device, solve)
    if solve == "device" and scorer is not None:
        raise ValueError("solve='device' takes no scorer")
    return _run_batch(_E, pairs, threshold, prob, max_iters, seed, device, solve, sampler, scorer=scorer)[0]


def find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000, seed=0, device=None, solve="host", sampler="host",
                         refine=0, score="count", max_threshold=None):
    """RANSAC over seven-point samples with the Sampson distance in pixels (the demo's geometry filter, demo.py:514-517): plain
    inlier counting by default; score="magsac" ranks the hypotheses by the MAGSAC++ loss the reference's USAC_MAGSAC names (the
    published closed form, not cv2's bytes; below).  -> (F [3,3] | None, mask [P])
    solve="host": `seven_point` (SVD null space, eigenvalues) on points Hartley-normalised once per call, the candidates mapped back
    to pixel units for scoring (on `device` when given, as in find_essential_mat: same trajectory as the host run).
    solve="device" (needs `device`): the same indices are drawn on the host and uploaded; models, flags and counts come from one
    gim_fundamental_step per step (`DeviceFundamental`: elimination, a closed-form cubic, normalisation per sample; it rounds
    differently from `seven_point`, so its trajectory need not be the host's), the mask from gim_ransac_mask.
    solve="ge" (host only): the same RANSAC over `seven_point_ge`, the numpy restatement of the device solver -- its CPU oracle.
    sampler: "host", "philox" or "device", as in find_essential_mat ("device" needs `device` and solve="device").
    refine: 0 returns the RANSAC's best seven-point model and its mask (the default; every seeded result so far).  R in 1 .. 8 then
    runs up to R rounds of local optimisation on it, the step USAC ends with: the normalised eight-point fit on the current inliers,
    a fresh mask, kept while the inlier count does not fall (`refit_ge`).  With a device it is ONE gim_model_refit launch on the
    points already there (with sampler="device" it also replaces the gim_ransac_mask call), with device=None `refit_ge` itself.
    score: "count" (the default; every seeded result so far) accepts the sample with the most inliers.  "magsac" (needs
    sampler="philox" or "device") accepts a sample iff it has at least 7 inliers and its quality -- the int64 sum over the points
    of the quantised MAGSAC++ gain (`magsac_quality`, gim_magsac_score) -- is strictly above the best so far; the iteration bound
    is updated with the accepted model's inlier count, the mask is the same mask call, and `refine` composes unchanged.
    max_threshold (score="magsac"): the k sigma bound the gain is marginalised up to, in pixels; None: `threshold`."""
    _check_solve(solve, device)
    check_sampler(sampler, device, solve)
    max_thr2 = _check_score(score, sampler, threshold, max_threshold)
    refine = _check_refine(refine)
    p0, p1 = _points64(p0, p1)
    F, mask, dev = _run_pair(_F, p0, p1, threshold, prob, max_iters, seed, device, solve, sampler, max_thr2=max_thr2,
                             finish=_refit_finish(refine) if refine else None)
    if not refine or F is None or sampler == "device":         # sampler="device": `finish` has refined it already
        return F, mask
    if dev is None:
        return refit_ge(1, p0, p1, F, float(threshold) ** 2, rounds=refine)[:2]
    models, mask, _, _ = dev.refit(F, refine)
    return models[0], mask


def _points64(a, b):
    """the two sides of a pair as contiguous fp64 [P, 2] arrays"""
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 2), np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 2)


def _pairs64(pairs):
    """[(x0, x1)] -> (the pairs as contiguous fp64 [P_b, 2] arrays, offsets int64 [B + 1] of their concatenation)"""
    pairs = [_points64(a, b) for a, b in pairs]
    return pairs, np.concatenate([[0], np.cumsum([a.shape[0] for a, _ in pairs])]).astype(np.int64)


def _over_pairs(cls, pairs, offsets, threshold, device, max_thr2=None, **kw):
    """a `_DevicePoints` class (or a stand-in with its constructor) over the concatenated points of `_pairs64`'s pairs; max_thr2: if set"""
    kw.update({} if max_thr2 is None else {"max_thr2": max_thr2})
    return cls(np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs]), float(threshold) ** 2, device, offsets=offsets, **kw)


def _lockstep(B, steps, launch):
    """Runs the `_ransac_steps` generators steps {b: generator} of a batch of B pairs in lockstep: every pair has its own generator
    (its own draws and its own shrinking iteration bound, so its result is that of the single call), and every round serves all
    unfinished pairs with ONE launch: launch({b: what pair b's step yielded}) -> {b: the counts to send it}.  A step shorter than
    the longest is padded by the launch, a finished pair no longer takes part.  -> [best model | None] * B"""
    best, pending = [None] * B, {}

    def advance(b, counts):
        try:
            pending[b] = next(steps[b]) if counts is None else steps[b].send(counts)
        except StopIteration as stop:
            best[b] = stop.value
            pending.pop(b, None)

    for b in steps:
        advance(b, None)
    while pending:
        counts = launch(pending)
        for b in sorted(pending):
            advance(b, counts[b])
    return best


def _batch_results(best, offsets, dev, finish=None):
    """The tail of every batched run: best [model | None] * B, `dev` the object that holds the concatenated points -> [(model | None,
    mask [P_b] bool)].  The models go up as one [B, 3, 3] array (zeros where a pair has none) for ONE dev.mask call, whose result is
    cut by `offsets`; a pair without a model gets an all-False mask, and a batch without any model calls nothing.
    finish: None, or finish(dev, models [B,3,3]) -> (models [B,3,3], masks [Ptot]) in place of that call (`_refit_finish`)."""
    B = len(best)
    found = [b for b in range(B) if best[b] is not None]
    masks = np.zeros(offsets[-1], dtype=bool)
    if found:
        models = np.zeros((B, 3, 3))
        for b in found:
            models[b] = best[b]
        if finish is None:
            masks = np.asarray(dev.mask(models), dtype=bool)
        else:
            models, masks = finish(dev, models)
            best = [models[b] if b in found else None for b in range(B)]
    return [(best[b], masks[offsets[b]:offsets[b + 1]] if best[b] is not None else np.zeros(offsets[b + 1] - offsets[b], dtype=bool))
            for b in range(B)]


class _DeferredSolve:
    """The `solve_idx` hook of one pair of a device-solve lockstep run: it keeps the step's indices and hands out empty arrays (k
    models per sample), which the launch that serves every pair fills in place before the counts are sent."""

    def __init__(self, k):
        self.k = k

    def __call__(self, idx):
        self.idx = idx
        self.models, self.valid = np.zeros((idx.shape[0], self.k, 3, 3)), np.zeros((idx.shape[0], self.k), dtype=bool)
        return self.models, self.valid


def _lockstep_device(pairs, step_cls, threshold, prob, max_iters, seed, device, sampler="host", step_kw=None, finish=None, max_thr2=None):
    """`_lockstep` with the solve on the device: a round uploads the sample indices of every unfinished pair and solves and scores
    all of them in ONE launch of `step_cls` (DeviceFundamental, DeviceEssential) over the concatenated points (ragged point sets
    through offsets; a finished pair and the padding of a shorter step are index -1: invalid).  The step object is made when the
    first round needs it: a batch in which no pair has `step_cls.m` points uploads nothing.  step_kw: further keywords of `step_cls`;
    finish: that of `_batch_results`.  max_thr2: a number runs the quality walk (score="magsac"): a round then also scores the
    resident models with ONE gim_magsac_score launch.  -> ([(model | None, mask)], the step object or None)"""
    m, k = step_cls.m, step_cls.k
    pairs, offsets = _pairs64(pairs)
    B = len(pairs)
    hooks = {b: _DeferredSolve(k) for b, (a, _) in enumerate(pairs) if a.shape[0] >= m}
    steps = {b: _ransac_steps(pairs[b][0].shape[0], None, m, prob, max_iters, np.random.default_rng(seed), *pairs[b], solve_idx=hook,
                              draw=_draw(sampler, seed, pairs[b][0].shape[0], m), quality=max_thr2 is not None) for b, hook in hooks.items()}
    dev = None

    def launch(pending):
        nonlocal dev
        if dev is None:
            dev = _over_pairs(step_cls, pairs, offsets, threshold, device, max_thr2, **(step_kw or {}))
        K = max(hooks[b].idx.shape[0] for b in pending)
        idx = np.full((B, K, m), -1, dtype=np.int32)
        for b in pending:
            idx[b, :hooks[b].idx.shape[0]] = hooks[b].idx
        models, valid = dev.solve(idx)
        if max_thr2 is not None:
            qual, counts = dev.quality(models, valid)
        else:
            counts = dev.counts(models, valid)
        out = {}
        for b in pending:
            nb = hooks[b].idx.shape[0]
            hooks[b].models[...], hooks[b].valid[...] = models[b, :nb], valid[b, :nb]
            out[b] = counts[b, :nb].reshape(-1) if max_thr2 is None else (qual[b, :nb].reshape(-1), counts[b, :nb].reshape(-1))
        return out

    best = _lockstep(B, steps, launch)
    return _batch_results(best, offsets, dev, finish), dev


# The control block of a `_ransac_on_device` step, uploaded as ONE int32 array: (field, 32-bit words per pair) in upload order, every
# field B entries long.  A field of two words is an int64 (the first ordinal; the quality floor); those come first: 8-byte aligned.
_CTL_COUNT = (("first", 2), ("count", 1), ("floor", 1))
_CTL_MAGSAC = (("first", 2), ("floor", 2), ("count", 1))


def _ctl_fields(ctl, layout, B, int64):
    """the fields of a control block `ctl` (a numpy array or a tensor of int32, `int64` its library's 64-bit type) -> {name: view}"""
    at = np.cumsum([0] + [words * B for _, words in layout]).tolist()
    return {name: ctl[at[i]:at[i + 1]] if words == 1 else ctl[at[i]:at[i + 1]].view(int64) for i, (name, words) in enumerate(layout)}


def _ransac_on_device(pairs, step_cls, threshold, prob, max_iters, seed, device, batch=250, step_kw=None, finish=None, max_thr2=None):
    """sampler="device": the RANSAC runs of `pairs` in lockstep with sampling, solving, scoring and the reduction of every step on
    the GPU.  A step is three launches of this library -- gim_ransac_sample, the step kernel of `step_cls` (DeviceHomography,
    DeviceFundamental, DeviceEssential), gim_ransac_records -- fed by ONE upload of 4 B words (`_CTL_COUNT`: first as int64, count,
    floor) and read by ONE copy of n_rec and the first RECORDS_FIRST_COPY triples of every pair (a second copy when some pair has
    more).  The host replays the records (`_Walk.replay`: the one rule and bound of every walk) and reads the 72 bytes of a pair's model
    only in a step that accepted a record of that pair; models, flags and counts are never read back in bulk.  A pair's ordinals run
    from 0 under the shared seed: its result is that of the single call, and that of sampler="philox" on the same device.
    When no pair has m points, nothing is uploaded or launched.  The run ends with `_batch_results`; finish: its hook.
    max_thr2: a number runs the quality walk (score="magsac"): a step is then four launches -- the sampler, the untouched step
    kernel (its counts are unused), gim_magsac_score on the step's resident models, gim_ransac_records64 with min_count = m -- fed
    by 5 B words (`_CTL_MAGSAC`: the floor is an int64 quality) and read by n_rec and the first RECORDS_FIRST_COPY quadruples of every pair.
    -> ([(model [3,3] | None, mask [P_b] bool)], the step object or None -- `find_homography` takes its re-fit mask from it)"""
    m, k = step_cls.m, step_cls.k
    seed = _check_seed64(seed)
    pairs, offsets = _pairs64(pairs)
    B = len(pairs)
    magsac = max_thr2 is not None
    walks = {b: _Walk(a.shape[0], m, prob, max_iters, batch, quality=magsac) for b, (a, _) in enumerate(pairs) if a.shape[0] >= m}
    best = [None] * B
    if not walks:
        return _batch_results(best, offsets, None), None
    import torch
    from . import ops
    dev = _over_pairs(step_cls, pairs, offsets, threshold, device, max_thr2, **(step_kw or {}))
    layout = _CTL_MAGSAC if magsac else _CTL_COUNT
    ctl = np.zeros(B * sum(w for _, w in layout), dtype=np.int32)        # one upload per step
    host = _ctl_fields(ctl, layout, B, np.int64)
    w_rec = 4 if magsac else 3
    head = 1 + w_rec * RECORDS_FIRST_COPY
    with torch.cuda.device(dev.device):
        while True:
            host["count"][:] = 0
            for b, w in walks.items():
                host["first"][b] = w.done
                host["count"][b], host["floor"][b] = w.plan()
            K = int(host["count"].max())
            if K == 0:
                break
            on = _ctl_fields(torch.from_numpy(ctl).to(dev.device), layout, B, torch.int64)
            idx = ops.ransac_sample(dev.offsets, on["first"], on["count"], K, m, seed)
            if magsac:
                models, flags = dev.step_on_device(idx, flags=True)
                qual, counts = dev.quality_on_device(models, flags)
                rec = ops.ransac_records64(qual.view(B, K, k), counts.view(B, K, k), on["count"], on["floor"], m)
            else:
                models, counts = dev.step_on_device(idx)
                rec = ops.ransac_records(counts.view(B, K, k), on["count"], on["floor"])
            h = rec[:, :head].cpu().numpy()
            if (h[:, 0] > RECORDS_FIRST_COPY).any():
                h = np.concatenate([h, rec[:, head:].cpu().numpy()], 1)
            models = models.view(B, K, k, 3, 3)
            for b, w in walks.items():
                if host["count"][b]:
                    hit = w.replay(h[b, 1:1 + w_rec * h[b, 0]].reshape(-1, w_rec))
                    if hit is not None:
                        best[b] = models[b, hit[0], hit[1]].cpu().numpy()
    return _batch_results(best, offsets, dev, finish), dev


# ---- the three models, described once, and the two runners every entry point goes through -----------------------------------------
def _hartley_seven_point(p0, p1):
    """-> (`seven_point` with its candidates mapped back to pixel units for scoring, the points Hartley-normalised once per call for it)"""
    def norm_T(p):
        c = p.mean(0)
        s = np.sqrt(2.0) / max(np.sqrt(((p - c) ** 2).sum(1)).mean(), 1e-12)
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    T0, T1 = norm_T(p0), norm_T(p1)

    def solver(a, b):
        F, v = seven_point(a, b)
        Fp = T1.T @ F @ T0
        nrm = np.linalg.norm(Fp.reshape(*Fp.shape[:-2], 9), axis=-1)
        return Fp / np.where(nrm > 0, nrm, 1.0)[..., None, None], v

    return solver, p0 * T0[0, 0] + T0[:2, 2], p1 * T1[0, 0] + T1[:2, 2]


# step: the device step class -- it carries m, k and the refit / MAGSAC kind; host(a, b) -> (the LAPACK solver, the points it samples
# from); ge: the numpy restatement of the device solver; error: the host error of the model
_Model = collections.namedtuple("_Model", "step host ge error")
_E = _Model(DeviceEssential, lambda a, b: (five_point, a, b), five_point_ge, sampson_error)
_F = _Model(DeviceFundamental, _hartley_seven_point, seven_point_ge, sampson_error)
_H = _Model(DeviceHomography, lambda a, b: (homography_4pt, a, b), homography_4pt, transfer_error)


def _run_pair(model, x0, x1, threshold, prob, max_iters, seed, device, solve, sampler, max_thr2=None, finish=None, step_kw=None):
    """One pair (`_points64`'s arrays, arguments already checked) through the ladder of a `_Model` -> (model [3,3] | None, mask [P]
    bool, the object that holds the points on the device | None).  sampler="device": `_ransac_on_device` (finish: its hook; no
    other path takes one).  Otherwise `_ransac` over `_draw`'s samples: solve="device" with the model's step class (step_kw: its
    further keywords), "ge" with the restated solver, "host" with the LAPACK solver and a `DeviceScorer` when there is a device.
    Fewer than m points: (None, all-False, None), after the seed was checked and before anything is uploaded."""
    P, m = x0.shape[0], model.step.m
    if sampler == "device":
        found, dev = _run_batch(model, [(x0, x1)], threshold, prob, max_iters, seed, device, solve, sampler, None, max_thr2, finish, step_kw)
        return found[0] + (dev,)
    draw, rng = _draw(sampler, seed, P, m), np.random.default_rng(seed)
    if P < m:
        return None, np.zeros(P, dtype=bool), None
    dev, solver, s0, s1, thr2 = None, model.ge, None, None, float(threshold) ** 2
    if solve == "device":
        dev, solver = model.step(x0, x1, thr2, device, max_thr2=max_thr2, **(step_kw or {})), None
    elif solve == "host":
        solver, s0, s1 = model.host(x0, x1)
        dev = DeviceScorer(x0, x1, thr2, device, max_thr2=max_thr2) if device is not None else None
    return _ransac(x0, x1, solver, m, threshold, prob, max_iters, rng, s0=s0, s1=s1, scorer=dev, solve_idx=dev.solve if solver is None else None,
                   error=model.error, draw=draw, max_thr2=max_thr2, kind=model.step._kind) + (dev,)


def _run_batch(model, pairs, threshold, prob, max_iters, seed, device, solve, sampler, scorer=None, max_thr2=None, finish=None, step_kw=None):
    """A pair list (arguments already checked) through the ladder of a `_Model` -> ([(model | None, mask [P_b] bool)], the object
    that holds the concatenated points | None); a pair's result is `_run_pair`'s.  solve="device": `_ransac_on_device` for
    sampler="device", else `_lockstep_device` (max_thr2, finish, step_kw: theirs).  solve="host", counts only: the pairs one by one
    without a device or scorer; else `_lockstep`, a round's host-solved candidates scored in ONE scorer.counts launch for all pairs."""
    if solve == "device" and sampler == "device":
        return _ransac_on_device(pairs, model.step, threshold, prob, max_iters, seed, device, step_kw=step_kw, finish=finish, max_thr2=max_thr2)
    if solve == "device":
        return _lockstep_device(pairs, model.step, threshold, prob, max_iters, seed, device, sampler, step_kw, finish, max_thr2)
    pairs, offsets = _pairs64(pairs)
    if scorer is None and device is None:
        return [_run_pair(model, a, b, threshold, prob, max_iters, seed, None, solve, sampler)[:2] for a, b in pairs], None
    B, m = len(pairs), model.step.m
    if B == 0:
        return [], None
    if scorer is None:
        scorer = _over_pairs(DeviceScorer, pairs, offsets, threshold, device)
    steps = {}
    for b, (a, c) in enumerate(pairs):
        if a.shape[0] >= m:
            solver, s0, s1 = model.host(a, c)
            steps[b] = _ransac_steps(a.shape[0], solver, m, prob, max_iters, np.random.default_rng(seed), s0, s1, draw=_draw(sampler, seed, a.shape[0], m))

    def launch(pending):
        K = max(Ms.shape[0] for Ms, _ in pending.values())
        models, valid = np.zeros((B, K, 3, 3)), np.zeros((B, K), dtype=bool)   # finished pairs and padding: valid = 0
        for b, (Ms, v) in pending.items():
            models[b, :Ms.shape[0]], valid[b, :Ms.shape[0]] = Ms, v
        counts = scorer.counts(models, valid)
        return {b: counts[b, :Ms.shape[0]] for b, (Ms, _) in pending.items()}

    return _batch_results(_lockstep(B, steps, launch), offsets, scorer), scorer


def find_fundamental_mat_batch(pairs, threshold=1.0, prob=0.999999, max_iters=10000, seed=0, device=None, solve="device", sampler="host",
                               refine=0, score="count", max_threshold=None):
    """`find_fundamental_mat(p0, p1, threshold, prob, max_iters, seed, device, solve="device")` for every (p0, p1) of `pairs`:
    `_lockstep_device` with `DeviceFundamental`, ONE gim_fundamental_step launch per round and one gim_ransac_mask call for all
    pairs at the end; a pair's result is that of the single call.
    sampler: "philox" draws every pair's samples with `device_samples` on the host, "device" on the GPU, where each step is then
    reduced to its record samples (`_ransac_on_device`); a pair's result is again that of the single call with that sampler.
    refine: that of find_fundamental_mat; R > 0 replaces the run's gim_ransac_mask call with ONE gim_model_refit launch over all
    pairs (a pair without a model is skipped there, and a batch without any model launches nothing).
    score, max_threshold: those of find_fundamental_mat; "magsac" adds ONE gim_magsac_score launch over all pairs to every round.
    -> [(F [3,3] | None, mask [P_b] bool)] in the order of `pairs`."""
    _check_solve(solve, device, ("device",))
    check_sampler(sampler, device, solve)
    max_thr2 = _check_score(score, sampler, threshold, max_threshold)
    refine = _check_refine(refine)
    return _run_batch(_F, pairs, threshold, prob, max_iters, seed, device, solve, sampler, max_thr2=max_thr2,
                      finish=_refit_finish(refine) if refine else None)[0]


def verify_pairs(pairs_of_points, threshold=1.0, device=None, prob=0.999999, max_iters=10000, seed=0, batch=32, sampler="host", refine=0,
                 score="count", max_threshold=None):
    """Two-view verification of a pair list (the matches of a LightGlue / root_sift / dense pair list, in pixels) without OpenCV:
    `find_fundamental_mat_batch` over `batch` pairs per launch sequence -> [(F [3,3] | None, mask [P_b] bool)] in the list's order.
    sampler, refine, score, max_threshold: those of find_fundamental_mat_batch."""
    check_sampler(sampler, device)
    _check_score(score, sampler, threshold, max_threshold)
    refine = _check_refine(refine)
    pairs_of_points = list(pairs_of_points)
    out = []
    for i in range(0, len(pairs_of_points), int(batch)):
        out += find_fundamental_mat_batch(pairs_of_points[i:i + int(batch)], threshold, prob, max_iters, seed, device, sampler=sampler,
                                          refine=refine, score=score, max_threshold=max_threshold)
    return out


def find_homography(src, dst, threshold=1.0, prob=0.999999, max_iters=10000, seed=0, device=None, sampler="host", refit="host",
                    score="count", max_threshold=None):
    """cv2.findHomography(src, dst, RANSAC, threshold, maxIters=max_iters, confidence=prob) restated: dst ~ H src
    -> (H [3, 3] with h33 = 1 | None, mask [P] bool).  Plain RANSAC over four-point samples with the forward transfer error in
    pixels; sampling and the shrinking iteration bound are `_ransac_steps`'.  Host path: `homography_4pt` and `transfer_error`.
    device: the same indices are drawn on the host and uploaded; models, flags and counts come from one gim_homography_step per
    step (`DeviceHomography`; the device rounds differently, so its trajectory need not be the host's).  Then, as
    RANSACPointSetRegistrator::run + findHomography do, the model is re-fitted on the inliers of the best sample (`homography_dlt`)
    and the mask taken once more with the re-fitted model; the re-fit is kept only if it does not lose inliers.  OpenCV's final
    Levenberg-Marquardt polish of the re-fit (HomographyRefineCallback) is NOT built.  score="magsac" ranks the hypotheses by the
    MAGSAC++ loss the reference's demo asks for with USAC_MAGSAC (the published closed form, not cv2's bytes; below).
    sampler: "host", "philox" or "device", as in find_essential_mat ("device" needs `device`; the solve is the device's whenever
    a device is given).
    refit: "host" re-fits with `homography_dlt` (LAPACK's SVD of the 2n x 9 system) and takes the second mask where the first was
    taken (the default; every seeded result so far).  "device" (needs `device`) replaces both with ONE gim_model_refit launch of one
    round on the points the step object holds, and one copy of H, the mask and the counts; with sampler="device" that launch also
    replaces the gim_homography_mask call that ends the RANSAC.  "ge" (device=None) is the same on the host through `refit_ge`,
    the CPU oracle of "device".
    score, max_threshold: as in find_fundamental_mat, over the forward transfer error and with 4 inliers to be eligible; "magsac"
    needs sampler="philox" or "device"; the re-fit that follows starts from the returned model, unchanged."""
    check_sampler(sampler, device)
    max_thr2 = _check_score(score, sampler, threshold, max_threshold)
    check_refit(refit, device)
    src, dst = _points64(src, dst)
    thr2 = float(threshold) ** 2
    H, mask, dev = _run_pair(_H, src, dst, threshold, prob, max_iters, seed, device, "host" if device is None else "device", sampler,
                             max_thr2=max_thr2, finish=_refit_finish(1) if refit == "device" else None)
    mask = np.asarray(mask, dtype=bool)
    if H is None or (sampler == "device" and refit == "device"):        # the latter: `finish` has re-fitted it already
        return H, mask
    if refit == "device":
        models, mask, _, _ = dev.refit(H, 1)
        return models[0], mask
    if refit == "ge":
        return refit_ge(0, src, dst, H, thr2, rounds=1)[:2]
    H2 = homography_dlt(src[mask], dst[mask])
    if H2 is not None:
        mask2 = (transfer_error(H2, src, dst) <= thr2) if dev is None else \
            np.asarray(dev.mask(H2 if dev.offsets is None else H2[None]), dtype=bool)
        if mask2.sum() >= mask.sum():
            H, mask = H2, mask2
    return H, mask


def recover_pose(E, x0, x1, distance_thresh=1e9, mask=None, device=None):
    """cv2.recoverPose(E, x0, x1, eye(3), distanceThresh, mask=mask) on normalised points -> (n_good, R, t, mask_out).
    device: None runs here (LAPACK's SVDs); a device uploads E, the points and the mask and runs gim_recover_pose there
    (ops.recover_pose: `recover_pose_ge`'s arithmetic, so R1 / R2 and the sign of t may be LAPACK's exchanged -- the same candidate
    set); an invalid E gives (0, zero R, zero t, all-False)."""
    if device is not None:
        import torch
        from . import ops
        with torch.cuda.device(torch.device(device)):
            up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(device)   # noqa: E731  (a copy: `a` may be read-only)
            x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 2)
            m = None if mask is None else up(np.asarray(mask).ravel() > 0, np.uint8)
            n, best, R, t, good = ops.recover_pose(up(E, np.float64), up(x0, np.float64), up(np.asarray(x1, dtype=np.float64).reshape(-1, 2), np.float64),
                                                   mask=m, distance_thresh=distance_thresh)
            k = int(best)
            return (int(n[k]) if k >= 0 else 0), R.cpu().numpy(), t.cpu().numpy(), good.cpu().numpy()
    return recover_pose_host(E, x0, x1, distance_thresh, mask)


def _refit_finish(rounds):
    """a `finish` hook of `_batch_results`: the refit's models and masks in place of the RANSAC's"""
    return lambda dev, M: dev.refit(M, rounds)[:2]


def backend():
    """'cv2' when OpenCV imports (and GIM_POSE_BACKEND does not say 'numpy'), else 'numpy'"""
    want = os.environ.get("GIM_POSE_BACKEND", "auto")
    if want not in ("auto", "cv2", "numpy"):
        raise ValueError(f"GIM_POSE_BACKEND={want!r}: auto, cv2 or numpy")
    if want == "numpy":
        return "numpy"
    try:
        import cv2  # noqa: F401
        return "cv2"
    except ImportError:
        if want == "cv2":
            raise
        return "numpy"
