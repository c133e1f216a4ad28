"""Seeded inputs shared by tests/test_magsac_cpu.py and tests/test_gpu_magsac.py: models and points for the MAGSAC++ score
(pose.magsac_quality / gim_magsac_score), quality arrays for the record reduction keyed on them (pose.step_records64 /
gim_ransac_records64), and the thresholds of the end-to-end runs.  Nothing here touches a device; every case is built once and
frozen."""
import functools

import numpy as np

import fundamental_cases as FC
import homography_oracle as HO
import ransac_sampler_cases as C

THR2, MAX_THR2 = 1.0, 2.25       # (1 px)^2, and a band of 1.5 px for the calls that marginalise wider than they count
K_REC = C.K


@functools.lru_cache(maxsize=None)
def score_case(kind, P, K):
    """kind 1 (fundamental matrices, pixels) or 0 (homographies) -> (models [K,3,3], valid bool [K], a [P,2], b [P,2]).  The points
    are a noisy two-view scene (0.3 px) with every third match an outlier; model 0 is the truth, the others are perturbed so that
    their residuals spread from zero to far beyond the band.  Planted where the sizes allow: point 0 has r2 == 0 exactly under
    model 1 (a pure x-translation for kind 1, the identity for kind 0), point 1 lies 1e-6 (relative) beyond k sigma of it and
    point 2 as much inside, point 3 has a NaN coordinate; model 2 has a NaN entry, model 3 an infinite one, model 4 is all zero,
    and every seventh model from 5 on is invalid."""
    rng = np.random.default_rng(1000 * kind + 10 * P + K)
    if kind == 1:
        a, b, M = FC.two_views(rng, max(P, 8))
    else:
        M = HO.general_h(rng)
        a = rng.uniform([0, 0], [HO.W, HO.H_IMG], (max(P, 8), 2))
        b = HO.proj(M, a)
    a, b = a[:P].copy(), b[:P] + rng.normal(size=(P, 2)) * 0.3
    out = np.arange(P) % 3 == 2
    b[out] = rng.uniform([0.0, 0.0], [640.0, 480.0], (int(out.sum()), 2))
    models = M[None] * (1.0 + rng.normal(size=(K, 3, 3)) * np.logspace(-7, -2, K)[:, None, None])
    models[0] = M
    valid = np.ones(K, dtype=bool)
    if K > 1:
        models[1] = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) if kind == 1 else np.eye(3)
        if P > 0:
            b[0] = a[0]                                              # r2 == 0: e = y1 - y0 (kind 1), dst - src (kind 0)
        # kind 1 under the x-translation: err = (y1 - y0)^2 / 2; kind 0 under the identity: err = |dst - src|^2
        off = np.sqrt(THR2 * (2.0 if kind == 1 else 1.0))
        if P > 1:
            b[1] = a[1] + [0.0, off * (1.0 + 1e-6)]
        if P > 2:
            b[2] = a[2] + [0.0, off * (1.0 - 1e-6)]
    if P > 3:
        b[3, 0] = np.nan
    if K > 2:
        models[2, 1, 1] = np.nan
    if K > 3:
        models[3, 0, 2] = np.inf
    if K > 4:
        models[4] = 0.0
    valid[5::7] = False
    for x in (models, valid, a, b):
        x.setflags(write=False)
    return models, valid, a, b


def loop_quality(kind, models, valid, a, b, thr2, max_thr2):
    """pose.magsac_quality one point at a time with Python floats for the residual (the order of the device's expressions) and
    pose.magsac_units for the gain -> (quality [K], counts [K]) as Python-int arrays"""
    import math

    from gim_amd import pose
    K, P = len(models), len(a)
    q, c = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for k in range(K):
        m = [float(v) for v in np.asarray(models[k]).reshape(9)]
        if not valid[k] or not all(math.isfinite(v) for v in m):
            continue
        for p in range(P):
            ax, ay, bx, by = float(a[p, 0]), float(a[p, 1]), float(b[p, 0]), float(b[p, 1])
            try:
                if kind == 1:
                    r0, r1, r2 = m[0] * ax + m[1] * ay + m[2], m[3] * ax + m[4] * ay + m[5], m[6] * ax + m[7] * ay + m[8]
                    c0, c1 = m[0] * bx + m[3] * by + m[6], m[1] * bx + m[4] * by + m[7]
                    e = r0 * bx + r1 * by + r2
                    den = r0 * r0 + r1 * r1 + c0 * c0 + c1 * c1
                    err = (e * e) / (1e-300 if den < 1e-300 else den)
                else:
                    w = m[6] * ax + m[7] * ay + m[8]
                    if w == 0.0:
                        continue
                    ex, ey = bx - (m[0] * ax + m[1] * ay + m[2]) / w, by - (m[3] * ax + m[4] * ay + m[5]) / w
                    err = ex * ex + ey * ey
            except OverflowError:
                continue
            if not math.isfinite(err):
                continue
            c[k] += err <= thr2
            q[k] += int(pose.magsac_units(err, max_thr2))
    return q, c


@functools.lru_cache(maxsize=None)
def records_case(k):
    """quality int64 [6, K, k], counts int32 [6, K, k], nb [6], floor_q int64 [6], min_count: the count arrays of
    ransac_sampler_cases.count_case(k) as eligibility, with qualities far above 2^32 that do not follow the counts.  Pair 0: many
    ineligible slots and slot ties (the lowest wins), a later sample that equals an earlier one; pair 1: a strictly increasing run
    of 40 records; pair 2: records on both sides of every wave and chunk edge; pair 3: a floor above every quality; pair 4:
    nb = 100 with larger qualities beyond it; pair 5: nb = 0."""
    counts, nb, _ = C.count_case(k)
    rng = np.random.default_rng(70 + k)
    q = rng.integers(0, 1 << 36, counts.shape).astype(np.int64)
    q[0] = rng.integers(0, 12, counts[0].shape) << 33                       # few distinct values: ties across slots and samples
    q[0, 5] = q[0, 5].max()
    q[0, 9] = q[0, 5]
    q[1] = rng.integers(0, 1 << 30, counts[1].shape)
    q[1, 10:50, k - 1] = (1 << 40) + (np.arange(40) << 20)                  # eligible there: count_case plants counts >= 50
    q[1, 10:50:2, 0] = q[1, 10:50:2, k - 1]
    q[1, 60:] = np.minimum(q[1, 60:], 1 << 39)
    q[2] = 0
    for i, s in enumerate((0, 63, 64, 127, 128, 191, 192, 255, 256)):
        q[2, s, i % k] = (1 << 34) + i                                      # count_case: counts 20 + i there, 0 elsewhere
    q[4, 100:] += 1 << 50
    floor_q = np.array([5 << 33, 1 << 31, 0, 1 << 62, 1 << 35, 0], dtype=np.int64)
    for x in (q, floor_q):
        x.setflags(write=False)
    return q, counts, nb, floor_q, 6


def check_records64(rec, ref):
    """the specified part of two record buffers [B, 1 + 4 K] agrees: n_rec and the first n_rec quadruples of every pair"""
    rec, ref = np.asarray(rec), np.asarray(ref)
    assert rec.shape == ref.shape and rec.dtype == np.int64
    assert np.array_equal(rec[:, 0], ref[:, 0]), (rec[:, 0], ref[:, 0])
    for b in range(len(ref)):
        n = 1 + 4 * int(ref[b, 0])
        assert np.array_equal(rec[b, :n], ref[b, :n]), (b, rec[b, :n], ref[b, :n])


@functools.lru_cache(maxsize=None)
def scene_truth(kind):
    """the planted inliers of ransac_sampler_cases.scenes(kind), which returns no truth: its seeded draws are replayed here in its
    order, and the replay must reproduce its points bit for bit -> {name: bool [P]} for the scenes with outliers"""
    rng = np.random.default_rng({"F": 61, "H": 63}[kind])
    scenes, out = C.scenes(kind), {}
    for name, n, share in (("half outliers", 2000, 0.5), ("mostly inliers", 400, 0.05), ("all outliers", 120, 1.0)):
        if kind == "F":
            a, b, _ = FC.two_views(rng, n)
        else:
            H = HO.general_h(rng)
            a = rng.uniform([0, 0], [HO.W, HO.H_IMG], (n, 2))
            b = HO.proj(H, a)
        b = b + rng.normal(size=(n, 2)) * 0.3
        gone = rng.random(n) < share
        b[gone] = rng.uniform([0.0, 0.0], [640.0, 480.0] if kind == "F" else [HO.W, HO.H_IMG], (int(gone.sum()), 2))
        assert a.tobytes() == scenes[name][0].tobytes() and b.tobytes() == scenes[name][1].tobytes(), (kind, name)
        out[name] = ~gone
        out[name].setflags(write=False)
    return out


def video(n=6, H=48, W=64):
    """frames uint8 [n,H,W,3] and class maps uint8 [n,24,32] (class 3 is the excluded one, nowhere dominant) for label_pair_list"""
    rng = np.random.default_rng(78)
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), rng.integers(0, 3, (n, 24, 32), dtype=np.uint8)


def stub_match(inputs):
    """a matcher that sees the sizes of its inputs only: 80 exact matches of a two-view scene and 20 uniform outliers, scaled to
    the two images, seeded by the sizes -> a matcher's result dict of numpy arrays"""
    h0, w0 = inputs["image0"].shape[-2:]
    h1, w1 = inputs["image1"].shape[-2:]
    rng = np.random.default_rng(1000 * h0 + w1)
    X = np.stack([rng.uniform(-1, 1, 100), rng.uniform(-0.7, 0.7, 100), rng.uniform(2.5, 6, 100)], 1)
    c, s_ = np.cos(0.08), np.sin(0.08)
    R, t = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]]), np.array([0.4, 0.05, 0.02])
    Y = X @ R.T + t
    u0, u1 = X[:, :2] / X[:, 2:] * 0.6 + 0.5, Y[:, :2] / Y[:, 2:] * 0.6 + 0.5
    u1[80:] = rng.uniform(0.0, 1.0, (20, 2))
    return {"mkpts0_f": (u0 * [w0, h0]).astype(np.float32), "mkpts1_f": (u1 * [w1, h1]).astype(np.float32)}
