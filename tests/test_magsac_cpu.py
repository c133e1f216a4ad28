"""MAGSAC++ scoring without a GPU: pose.magsac_gain against scipy's incomplete gamma functions and mpmath, its shape and constants,
pose.magsac_quality against a per-point loop, pose.step_records64 and the quality record walk against sequential loops,
score="magsac" with sampler="philox" on the repository's F and H scenes, the decidability of those scenes, every refusal, the
unchanged defaults byte for byte, the new exports against the header, the kernels' resources, and the stand-alone host program
over csrc/magsac_loss.h (tools/magsac_host_check.cpp).  Inputs: tests/magsac_cases.py, tests/ransac_sampler_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import fundamental_cases as FC
import homography_cases as HC
import host_check
import label_link_cases as LC
import magsac_cases as MC
import ransac_sampler_cases as C
from gim_amd import demo, pose, video_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}
UK = pose.MAGSAC_UK


# ---- the gain ------------------------------------------------------------------------------------------------------------------------
def _grid():
    return np.concatenate([np.linspace(0.0, 1.1 * UK, 200001), np.logspace(-30, -3, 1000)])


def test_gain_against_the_incomplete_gamma_functions():
    sp = pytest.importorskip("scipy.special")
    u = _grid()
    n = sp.gammainc(2.5, u) * sp.gamma(2.5) + u * (sp.gammaincc(1.5, u) * sp.gamma(1.5) - pose.MAGSAC_GK)
    ref = np.where(u < UK, 1.0 - n / pose.MAGSAC_LK, 0.0)
    err = np.abs(pose.magsac_gain(u) - ref).max()
    print(f"largest |gain - gammainc form| over {len(u)} values: {err:.3e} = {err * 2 ** 32:.1e} quantisation units")
    assert err <= 1e-13
    # the two constants
    assert abs(sp.gammaincc(1.5, UK) * sp.gamma(1.5) - pose.MAGSAC_GK) <= 1e-15
    assert abs(sp.gammainc(2.5, UK) * sp.gamma(2.5) - pose.MAGSAC_LK) <= 1e-15


def test_gain_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    Gk, gk = mp.gammainc(1.5, UK), mp.gammainc(2.5, 0, UK)
    assert abs(float(Gk) - pose.MAGSAC_GK) <= 1e-15 and abs(float(gk) - pose.MAGSAC_LK) <= 1e-15
    for u in (1e-30, 1e-9, 1e-3, 0.1, 0.5, 1.0, 2.0, 3.3124, 5.0, 6.5, 6.6247):
        ref = 1 - (mp.gammainc(2.5, 0, u) + u * (mp.gammainc(1.5, u) - Gk)) / gk
        assert abs(float(pose.magsac_gain(u)) - float(ref)) <= 1e-13, u


def test_gain_shape():
    u = _grid()[:200001]
    g = pose.magsac_gain(u)
    assert UK == 3.64 * 3.64 / 2.0 and pose.MAGSAC_K == 3.64
    assert pose.magsac_gain(0.0) == 1.0 and (g[u >= UK] == 0.0).all() and pose.magsac_gain(UK) == 0.0
    assert ((g >= 0.0) & (g <= 1.0)).all()
    assert np.diff(g).max() <= 2e-15                    # non-increasing up to the rounding of the four terms
    assert g[np.searchsorted(u, UK) - 1] < 1e-5         # continuous at u_k
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert pose.magsac_gain(bad) == 0.0
    assert pose.magsac_units(0.0, 1.0) == 2 ** 32 and pose.magsac_units(np.nan, 1.0) == 0 and pose.magsac_units(np.inf, 1.0) == 0
    assert pose.magsac_units(1.0, 1.0) == 0 and pose.magsac_units(4.0, 4.0 * (1 + 1e-9)) <= 1


def test_derivative_of_the_closed_form():
    """N'(u) = Gamma(3/2, u) - G_k: the central difference of the closed form against scipy's incomplete gamma function"""
    sp = pytest.importorskip("scipy.special")
    um = np.linspace(0.05, UK, 400)
    h = 1e-5
    num = (pose.magsac_n(um + h) - pose.magsac_n(um - h)) / (2 * h)
    assert np.abs(num - (sp.gammaincc(1.5, um) * sp.gamma(1.5) - pose.MAGSAC_GK)).max() <= 1e-9     # h^2 |N'''| / 6 + 1e-16 / h


# ---- quality and records ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("P,K", [(0, 6), (1, 1), (65, 23)])
def test_quality_against_a_per_point_loop(kind, P, K):
    models, valid, a, b = MC.score_case(kind, P, K)
    for max_thr2 in (MC.THR2, MC.MAX_THR2):
        q, c = pose.magsac_quality(kind, models, valid, a, b, MC.THR2, max_thr2)
        lq, lc = MC.loop_quality(kind, models, valid, a, b, MC.THR2, max_thr2)
        assert q.dtype == np.int64 and c.dtype == np.int64 and q.shape == (K,)
        assert np.array_equal(c, lc)
        assert np.abs(q - lq).max() <= P                 # numpy's matrix products against the loop's operation order: a unit per point
        assert (q[~valid] == 0).all() and (c[~valid] == 0).all()
        if K > 4:
            assert q[2] == 0 and c[2] == 0 and q[3] == 0 and c[3] == 0
            n = P - (1 if P > 3 else 0)                                               # every point but the NaN one
            assert (q[4], c[4]) == ((n * 2 ** 32, n) if kind == 1 else (0, 0))         # all zero: 0 / 1e-300 (kind 1); w == 0 (kind 0)
        if P == 65:
            assert q[1] >= 2 ** 32 and c[1] >= 2                                      # point 0: r2 == 0; point 2: inside k sigma
            q1 = pose.magsac_quality(kind, models[1:2], None, a[:3], b[:3], MC.THR2, MC.THR2)
            assert q1[0][0] // 2 ** 32 == 1 and q1[0][0] - 2 ** 32 < 100 and q1[1][0] == 2   # ... and nearly without gain; point 1: beyond
    with pytest.raises(ValueError):
        pose.magsac_quality(2, models, valid, a, b, 1.0, 1.0)
    with pytest.raises(ValueError):
        pose.magsac_quality(1, models, valid, a, b, 1.0, 0.0)


@pytest.mark.parametrize("k", [1, 3, 10])
def test_step_records64_against_a_plain_loop(k):
    q, counts, nb, floor_q, mc = MC.records_case(k)
    rec = pose.step_records64(q, counts, nb, floor_q, mc)
    assert rec.shape == (6, 1 + 4 * MC.K_REC) and rec.dtype == np.int64
    for b in range(6):
        best, want = int(floor_q[b]), []
        for s in range(int(nb[b])):
            key = [int(q[b, s, j]) if counts[b, s, j] >= mc else 0 for j in range(k)]
            Q = max(key)
            if Q > best:
                best = Q
                j = key.index(Q)
                want.append((s, j, int(counts[b, s, j]), Q))
        assert rec[b, 0] == len(want) and rec[b, 1:1 + 4 * len(want)].reshape(-1, 4).tolist() == [list(t) for t in want], b
    assert rec[1, 0] >= 40 and rec[2, 0] == 9 and rec[3, 0] == 0 and rec[4, 0] > 0 and rec[5, 0] == 0
    if k > 1:
        run = rec[1, 1:1 + 4 * rec[1, 0]].reshape(-1, 4)
        assert (run[run[:, 0] % 2 == 0][:, 1] == 0).any() and (run[:, 1] == k - 1).any()          # ties: the lowest slot


def _sequential(kind, a, b, thr, conf, max_iters, seed, max_thr=None):
    """a plain RANSAC loop with the quality rule, one sample at a time over pose.device_samples -> (model | None, best quality,
    the smallest |difference| of two eligible qualities the loop compared -- but for ties of two models whose every unit was
    looked at and is 0 or 2^32 --, the number of such ties, the bound)"""
    m, solver, k = (7, pose.seven_point_ge, 1) if kind == "F" else (4, pose.homography_4pt, 0)
    P = len(a)
    if P < m:
        return None, 0, np.inf, 0, 0
    thr2, mt2 = thr * thr, (thr if max_thr is None else max_thr) ** 2
    lconf = np.log(max(1.0 - conf, 1e-300))
    best_q, best, niters, n, gap, ties = 0, None, int(max_iters), 0, np.inf, 0
    best_sat = True                                      # the start, quality 0: no unit at all
    error = pose.sampson_error if k == 1 else pose.transfer_error

    def near(x, x_sat, y, y_sat):
        nonlocal gap, ties
        if x == y and x_sat and y_sat:                   # every unit of both models is 0 or 2^32: see the test below
            ties += 1
        else:
            gap = min(gap, abs(x - y))

    while n < niters:
        nb = min(250, niters - n)                        # solved in blocks, walked one by one
        idx = pose.device_samples(seed, n, nb, P, m)
        Ms, valid = solver(a[idx], b[idx])
        kk = Ms.shape[1]
        q, c = pose.magsac_quality(k, Ms.reshape(-1, 3, 3), valid.reshape(-1), a, b, thr2, mt2)
        q, c = q.reshape(nb, kk), c.reshape(nb, kk)
        with np.errstate(all="ignore"):                  # the units themselves, point by point: is every one of a model 0 or 2^32?
            units = pose.magsac_units(error(Ms.reshape(-1, 3, 3), a, b), mt2)
        sat = ((units == 0) | (units == 2 ** 32)).all(1).reshape(nb, kk)
        assert np.array_equal(np.where(valid.reshape(-1), units.sum(1), 0), q.reshape(-1))
        for s in range(nb):
            if n + s >= niters:
                break
            key = [int(q[s, j]) if c[s, j] >= m else 0 for j in range(kk)]
            Q = max(key)
            j = key.index(Q)
            for jj in range(kk):
                if jj != j and c[s, jj] >= m:
                    near(Q, sat[s, j], key[jj], sat[s, jj])
            if c[s, j] >= m:
                near(Q, sat[s, j], best_q, best_sat)
            if Q > best_q:
                best_q, best, best_sat = Q, Ms[s, j], bool(sat[s, j])
                den = 1.0 - (int(c[s, j]) / P) ** m
                niters = min(niters, n + s + 1) if den < 1e-12 else min(niters, max(n + s + 1, int(np.ceil(lconf / np.log(den)))))
        n += nb
    return best, best_q, gap, ties, niters


def _philox(kind, a, b, **kw):
    if kind == "F":
        return pose.find_fundamental_mat(a, b, 1.0, 0.999999, 10000, seed=5, solve="ge", sampler="philox", **kw)
    return pose.find_homography(a, b, 1.0, 0.999999, 10000, seed=5, sampler="philox", refit="ge", **kw)


@pytest.mark.parametrize("kind", ["F", "H"])
def test_quality_walk_equals_a_sequential_loop_and_the_scenes_are_decidable(kind):
    """The walk of `_ransac_steps` (blocks of 250, records) is the sequential loop over the same samples, and on every scene the GPU
    tests reuse no two qualities that the loop compares (a sample's against the best so far, and against its other eligible slots)
    lie within 2 P units -- the device may differ from this oracle by a unit per point on each side.  One exception, checked
    unit by unit and not inferred from the sums: a TIE of two models of which every single point's unit is 0 or 2^32 (a sample
    that fits its own m points exactly and has no other point inside the band).  A unit is 2^32 for every u < 1.7e-10 and 0 for
    every u >= u_k, margins far above the 1e-15 by which two roundings of a residual differ, so such a tie is a tie on both sides
    and the strict comparison rejects it on both.  The all-outlier scenes and the homography scenes hold such ties; their number
    is printed.  Any other pair of compared qualities, equal ones included, counts towards the gap."""
    for name, (a, b) in C.scenes(kind).items():
        for max_thr in (None, 1.5):
            best, best_q, gap, ties, niters = _sequential(kind, a, b, 1.0, 0.999999, 10000, 5, max_thr)
            print(f"{kind} {name} max_threshold {max_thr}: best quality {best_q} = {best_q / 2 ** 32:.2f} points, smallest gap {gap} units "
                  f"(2 P = {2 * len(a)}), {ties} ties of saturated models, bound {niters}")
            assert gap > 2 * len(a), (name, gap)
            if kind == "F":
                M, mask = pose.find_fundamental_mat(a, b, 1.0, 0.999999, 10000, seed=5, solve="ge", sampler="philox", score="magsac",
                                                    max_threshold=max_thr)
                assert (M is None) == (best is None) and (M is None or M.tobytes() == best.tobytes())
            else:                                         # find_homography re-fits: drive the loop underneath it
                M, mask = pose._ransac(a, b, pose.homography_4pt, 4, 1.0, 0.999999, 10000, None, error=pose.transfer_error,
                                       draw=pose._draw("philox", 5, len(a), 4), max_thr2=(1.0 if max_thr is None else max_thr) ** 2, kind=0)
                assert (M is None) == (best is None) and (M is None or M.tobytes() == best.tobytes())
            assert mask.dtype == bool and mask.shape == (len(a),)


def test_record_walk_with_qualities_equals_the_steps_walk():
    """`_Walk(quality=True)` fed with step_records64 accepts what the quality walk of `_ransac_steps` accepts"""
    rng = np.random.default_rng(9)
    P, m, k, N = 2000, 7, 3, 1500
    c = rng.integers(0, 40, (N, k))
    q = rng.integers(1, 1 << 40, (N, k)).astype(np.int64)
    c[30, 1], q[30, 1] = 900, 1 << 41
    c[31, 0], q[31, 0] = 3, 1 << 50                       # ineligible: never accepted
    c[300, 2], q[300, 2] = 1500, 1 << 42                  # shrinks the bound into the second step
    tags = []

    def hook(idx):
        Ms = np.zeros((len(idx), k, 3, 3))
        Ms[:, :, 0, 0], Ms[:, :, 0, 1] = idx[:, None], np.arange(k)[None]
        hook.idx = idx
        return Ms, np.ones((len(idx), k), dtype=bool)

    steps = pose._ransac_steps(P, None, m, 0.999999, N, None, None, None, solve_idx=hook, draw=lambda first, nb: np.arange(first, first + nb),
                               quality=True)
    nbs = []
    try:
        next(steps)
        while True:
            nbs.append(len(hook.idx))
            steps.send((q[hook.idx].reshape(-1), c[hook.idx].reshape(-1)))
    except StopIteration as stop:
        best = stop.value
    want = (int(best[0, 0]), int(best[0, 1]))
    w = pose._Walk(P, m, 0.999999, N, quality=True)
    got, steps2 = None, []
    while True:
        nb, floor = w.plan()
        if nb == 0:
            break
        first = w.done
        rec = pose.step_records64(q[None, first:first + nb], c[None, first:first + nb], [nb], [floor], m)[0]
        hit = w.replay(rec[1:1 + 4 * rec[0]].reshape(-1, 4))
        if hit is not None:
            got = (first + hit[0], hit[1])
        steps2.append(nb)
    assert got == want == (300, 2) and steps2 == nbs and w.done == sum(nbs) and w.niters < N


def _sequential_quality(P, m, conf, max_iters, c, q):
    """the quality rule one sample at a time, written here: the test's own statement -> (best (sample, slot) | None, niters)"""
    lconf = np.log(max(1.0 - conf, 1e-300))
    best_q, best, niters, n = 0, None, int(max_iters), 0
    while n < niters:
        key = np.where(c[n] >= m, q[n], 0)
        j = int(key.argmax())
        if int(key[j]) > best_q:
            best_q, best = int(key[j]), (n, j)
            den = 1.0 - (int(c[n, j]) / P) ** m
            niters = min(niters, n + 1) if den < 1e-12 else min(niters, max(n + 1, int(np.ceil(lconf / np.log(den)))))
        n += 1
    return best, niters


@pytest.mark.parametrize("name", sorted(C.quality_run_cases()))
def test_quality_run_cases_three_drivers_agree(name):
    """tests/ransac_sampler_cases.quality_run_cases: the records driver (`_Walk` fed by step_records64), the generator driver
    (`_ransac_steps(quality=True)`) and the sequential loop above agree on the best (sample, slot), the step sizes and the final
    bound; the plant of each case is really there (the best and the bound it implies)."""
    P, m, conf, N, c, q, plant_best, plant_niters = C.quality_run_cases()[name]
    k = c.shape[1]
    seq_best, seq_niters = _sequential_quality(P, m, conf, N, c, q)
    assert (seq_best, seq_niters) == (plant_best, plant_niters), name
    if name == "the highest quality is ineligible":
        assert q[30].argmax() == 0 and c[30, 0] < m <= c[30, 2]
    if name == "the accepted slot has fewer inliers than another":
        assert c[40].argmax() == 1 != plant_best[1]
    if name == "two samples of equal quality":
        assert q[20, 1] == q[60, 2] and c[60, 2] >= m

    def hook(idx):
        Ms = np.zeros((len(idx), k, 3, 3))
        Ms[:, :, 0, 0], Ms[:, :, 0, 1] = idx[:, None], np.arange(k)[None]
        hook.idx = idx
        return Ms, np.ones((len(idx), k), dtype=bool)

    steps = pose._ransac_steps(P, None, m, conf, N, None, None, None, solve_idx=hook, draw=lambda first, nb: np.arange(first, first + nb), quality=True)
    gen_nbs = []
    try:
        next(steps)
        while True:
            gen_nbs.append(len(hook.idx))
            steps.send((q[hook.idx].reshape(-1), c[hook.idx].reshape(-1)))
    except StopIteration as stop:
        gen_best = None if stop.value is None else (int(stop.value[0, 0]), int(stop.value[0, 1]))
    w = pose._Walk(P, m, conf, N, quality=True)
    rec_best, rec_nbs = None, []
    while True:
        nb, floor = w.plan()
        if nb == 0:
            break
        first = w.done
        rec = pose.step_records64(q[None, first:first + nb], c[None, first:first + nb], [nb], [floor], m)[0]
        hit = w.replay(rec[1:1 + 4 * rec[0]].reshape(-1, 4))
        if hit is not None:
            rec_best = (first + hit[0], hit[1])
        rec_nbs.append(nb)
    print(f"{name}: best {seq_best}, bound {seq_niters}, steps {rec_nbs}")
    assert gen_best == rec_best == seq_best and gen_nbs == rec_nbs
    assert w.niters == seq_niters and w.done == sum(rec_nbs) and w.done - rec_nbs[-1] < seq_niters <= w.done


# ---- score="magsac" on the scenes -------------------------------------------------------------------------------------------------------
def test_philox_magsac_on_the_noisy_and_exact_scenes():
    """score="magsac" finds a model whose inlier set holds the TRUE inliers that the score="count" run finds, minus a margin.
    The truth is the planted inlier set of the scenes (magsac_cases.scene_truth replays their seeded draws).  The margin is
    measured on this oracle and written down, as the issue asks: the two runs may end on different minimal-sample models, each
    fitted to 0.3 px of noise, so each keeps some true matches near 1 px that the other drops.  Measured, true inliers found by
    both / by the count run: F half outliers 1008 / 1008 (of 1008 planted), F mostly inliers 328 / 352 (of 381; the bound ends both
    runs within a few samples; 6.8 % leave, the largest share), H half outliers 985 / 985 (of 988), H mostly inliers 384 / 384 (of
    385).  The assertion allows a tenth.  On the exact scenes nothing may leave.  The mean error over ALL true inliers is printed
    for both scores (F mostly inliers: 0.505 px count, 0.450 px magsac; the other three scenes end on the same sample: 0.200,
    0.371 and 0.390 px)."""
    for kind, err in (("F", pose.sampson_error), ("H", pose.transfer_error)):
        for name in ("half outliers", "mostly inliers"):
            a, b = C.scenes(kind)[name]
            truth = MC.scene_truth(kind)[name]
            Mc, mc = _philox(kind, a, b)
            Mm, mm = _philox(kind, a, b, score="magsac")
            found, kept = int((truth & mc).sum()), int((truth & mc & mm).sum())
            ec, em = float(np.sqrt(err(Mc, a, b)[truth]).mean()), float(np.sqrt(err(Mm, a, b)[truth]).mean())
            print(f"{kind} {name}: {truth.sum()} true inliers; the count run finds {found} of them (mask {mc.sum()}), the magsac run keeps "
                  f"{kept} of those (mask {mm.sum()}); mean error over the true inliers {ec:.4f} px (count) {em:.4f} px (magsac)")
            assert kept >= 0.9 * found
    Ft, p0, p1, truth = FC.ransac_scene()
    F, mask = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=2, solve="ge", sampler="philox", score="magsac")
    assert (mask & truth).sum() == truth.sum() and float(FC.sin_dist(F, Ft)) < 1e-6
    sc = HC.ransac_scene()
    H, mask = pose.find_homography(sc[1], sc[2], 1.0, 0.999999, 10000, seed=2, sampler="philox", score="magsac")
    assert H is not None and (mask & sc[3]).sum() == sc[3].sum()


def test_refusals():
    a, b = C.scenes("F")["mostly inliers"]
    for call in (lambda: pose.find_fundamental_mat(a, b, score="magsac"),                                   # sampler="host"
                 lambda: pose.find_fundamental_mat(a, b, solve="ge", sampler="host", score="magsac"),
                 lambda: pose.find_homography(a, b, score="magsac"),
                 lambda: pose.find_fundamental_mat(a, b, sampler="philox", score="usac"),
                 lambda: pose.find_homography(a, b, sampler="philox", score=None),
                 lambda: pose.find_fundamental_mat(a, b, sampler="philox", score="magsac", max_threshold=0.0),
                 lambda: pose.find_homography(a, b, sampler="philox", score="magsac", max_threshold=-1.0),
                 lambda: pose.find_fundamental_mat(a, b, sampler="philox", score="magsac", max_threshold=float("nan")),
                 lambda: pose.find_fundamental_mat(a, b, max_threshold=2.0),                                 # belongs to magsac
                 lambda: pose.verify_pairs([(a, b)], device="cuda:0", score="magsac"),
                 lambda: pose.find_fundamental_mat_batch([(a, b)], device="cuda:0", sampler="philox", score="magsac", max_threshold=0.0),
                 lambda: demo.compute_geom({"mkpts0_f": a, "mkpts1_f": b}, ransac_score="magsac"),
                 lambda: video_labels.label_pair_host((a, b), score="usac")):
        with pytest.raises(ValueError):
            call()
    for fn in (pose.find_essential_mat, pose.find_essential_mat_batch, pose.find_essential_pose):            # no MAGSAC for E
        with pytest.raises(TypeError):
            fn(a, b, 1e-3, score="magsac")
    with pytest.raises(SystemExit):
        demo.main(["--ransac-score", "magsac"])
    with pytest.raises(SystemExit):
        demo.main(["--ransac-score", "usac", "--ransac-sampler", "philox"])


def _same(x, y):
    (Ma, ma), (Mb, mb) = x, y
    assert (Ma is None) == (Mb is None) and (Ma is None or Ma.tobytes() == Mb.tobytes()) and ma.tobytes() == mb.tobytes()


def test_defaults_are_bit_equal():
    """every touched entry point with and without score="count": the same bytes.  Here the host paths (label_pair_list: the next
    test); the device paths, the batch calls, label_pair and the demo on a device are compared in tests/test_gpu_magsac.py"""
    a, b = C.scenes("F")["mostly inliers"]
    for kw in (dict(), dict(solve="ge"), dict(sampler="philox"), dict(solve="ge", sampler="philox", refine=2)):
        _same(pose.find_fundamental_mat(a, b, seed=3, **kw), pose.find_fundamental_mat(a, b, seed=3, score="count", max_threshold=None, **kw))
    s, t = C.scenes("H")["mostly inliers"]
    for kw in (dict(), dict(sampler="philox"), dict(refit="ge")):
        _same(pose.find_homography(s, t, seed=3, **kw), pose.find_homography(s, t, seed=3, score="count", **kw))
    k0, k1, _ = LC.pair_scene()
    kw = dict(threshold=0.5, max_iters=10000, seed=0)
    assert video_labels.label_pair_host((k0, k1), **kw).tobytes() == video_labels.label_pair_host((k0, k1), score="count", **kw).tobytes()
    out = {"mkpts0_f": a, "mkpts1_f": b}
    g0, g1 = demo.compute_geom(out), demo.compute_geom(out, ransac_score="count")
    assert all(g0[key].tobytes() == g1[key].tobytes() for key in ("Fundamental", "Homography"))
    # the label of the magsac score on the host: the planted matches, as the count's
    rows = video_labels.label_pair_host((k0, k1), score="magsac", **kw)
    assert rows.dtype == np.float32 and 200 <= len(rows) <= 230


def test_label_pair_list_default_is_bit_equal_on_a_host_bank(tmp_path):
    frames, segs = MC.video()
    bank = video_labels.FrameBank(len(frames))
    for i in range(len(frames)):
        bank.put(i, frames[i], seg=segs[i])
    ids = [(0, 2), (1, 3), (2, 5)]
    dirs = {}
    for tag, kw in (("plain", {}), ("count", dict(score="count")), ("magsac", dict(score="magsac"))):
        dirs[tag] = str(tmp_path / tag)
        r = video_labels.label_pair_list(MC.stub_match, bank, ids, "GIM_DKM", dirs[tag], vratio=1.0, exclude=[3], max_iters=500, seed=2, **kw)
        assert r["written"] == ids, (tag, r)
    for name in sorted(os.listdir(dirs["plain"])):
        assert open(os.path.join(dirs["plain"], name), "rb").read() == open(os.path.join(dirs["count"], name), "rb").read(), name
    for i0, i1 in ids:
        assert 70 <= len(np.load(os.path.join(dirs["magsac"], str(np.array([i0, i1])) + ".npy"))) <= 90      # 80 planted of 100


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in (x.strip() for x in m.group(2).split(","))]
    return _CTYPE[m.group(1)], args


def test_exports_follow_the_header_within_revision_115():
    from gim_amd import _lib
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    assert re.findall(r"^ \* (\d{3})\b", open(HEADER).read(), re.M)[-1] == "115"
    for name, nargs in (("gim_magsac_score", 13), ("gim_ransac_records64", 10)):
        res, args = _header_prototype(name)
        assert (res, args) == _lib.PROTOTYPES[name] and len(args) == nargs
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    score, rec = _lib.lib.gim_magsac_score, _lib.lib.gim_ransac_records64
    err = _lib.lib.gim_last_error
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = lambda n: ctypes.c_void_p(p.value + n)   # noqa: E731
    # empty problems return before anything is touched; malformed ones are refused before a launch
    assert score(1, None, None, None, None, None, 0, 7, 1.0, 1.0, None, None, None) == 0
    assert score(0, None, None, None, None, None, 3, 0, 1.0, 1.0, None, None, None) == 0
    for kind in (-1, 2):
        assert score(kind, p, None, p, p, p, 1, 4, 1.0, 1.0, p, p, None) != 0 and b"kind" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert score(1, p, None, p, p, p, 1, 4, 1.0, bad, p, p, None) != 0 and b"max_thr2" in err()
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert score(1, ptrs[0], None, ptrs[1], ptrs[2], ptrs[3], 1, 4, 1.0, 1.0, ptrs[4], ptrs[5], None) != 0 and b"NULL" in err()
    assert score(1, p, None, off(8), p, p, 1, 4, 1.0, 1.0, p, p, None) != 0 and b"16-byte" in err()
    assert score(1, p, None, p, p, p, 1, 4, 1.0, 1.0, off(4), p, None) != 0 and b"misaligned" in err()
    assert score(1, p, None, p, p, p, 1, 4, 1.0, 1.0, p, off(2), None) != 0 and b"misaligned" in err()
    assert score(1, p, None, p, p, p, 65536, 4, 1.0, 1.0, p, p, None) != 0 and b"65535" in err()
    assert score(1, p, None, p, p, p, -1, 4, 1.0, 1.0, p, p, None) != 0
    assert rec(None, None, None, None, 7, 0, 7, 3, None, None) == 0
    for k in (-1, 0, 2, 4, 9, 11):
        assert rec(p, p, p, p, 7, 1, 4, k, p, None) != 0 and b"1, 3 or 10" in err()
    for i in range(5):
        ptrs = [p] * 5
        ptrs[i] = None
        assert rec(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 7, 1, 4, 3, ptrs[4], None) != 0 and b"NULL" in err()
    for i, n in enumerate((4, 2, 2, 4, 4)):
        ptrs = [p] * 5
        ptrs[i] = off(n)
        assert rec(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 7, 1, 4, 3, ptrs[4], None) != 0 and b"misaligned" in err()
    assert rec(p, p, p, p, 7, 65536, 4, 3, p, None) != 0 and b"65535" in err()
    assert rec(p, p, p, p, 7, 40000, 20000, 1, p, None) != 0 and b"samples" in err()             # B (1 + 4 K) > INT32_MAX


def test_kernels_target_gfx950_without_scratch_or_spills():
    """magsac_score_kernel<0 | 1> with the fp64 erf, erfc and exp inlined: 145 VGPRs each when this was written, three waves per
    SIMD (at most 168 registers), no scratch, no spilled vector register; ransac_records64_kernel<1 | 3 | 10> beside the three
    unchanged ransac_records_kernel instances"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr._kernels()
    for name, n, max_regs in (("magsac_score_kernel<", 2, 168), ("ransac_records64_kernel<", 3, 64), ("ransac_records_kernel<", 3, 64)):
        hit = [(k, v) for k, v in ks.items() if name in k]
        assert len(hit) == n, (name, [k for k, _ in hit])
        for k, (regs, scratch, spills) in hit:
            print(f"{k[:70]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
            assert scratch == 0 and spills == 0 and regs <= max_regs, (k, regs, scratch, spills)


def test_host_check_agrees_with_numpy(tmp_path):
    """tools/magsac_host_check.cpp is plain C++ over csrc/magsac_loss.h: built with the host compiler (no sanitizer here; that run
    is a development step recorded in profiles/magsac.txt) it passes its own checks, and its gains and units are numpy's: the
    gain within 1e-14 (two C libraries' erf, erfc and exp), the units within one"""
    r = host_check.run("magsac_host_check", tmp_path)
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    rows = re.findall(r"u (\S+) gain ([0-9a-f]{16}) (\S+) units (-?\d+)", r.stdout)
    assert len(rows) == 30
    for u, bits, _, units in rows:
        u = float(u)
        g = np.array([int(bits, 16)], dtype=np.uint64).view(np.float64)[0]
        assert abs(g - float(pose.magsac_gain(u))) <= 1e-14, u
        assert abs(int(units) - int(pose.magsac_units(u * (1.0 / UK), 1.0))) <= 1, u
