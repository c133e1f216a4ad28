"""Seeded inputs shared by tests/test_label_link_cpu.py and tests/test_gpu_label_link.py: labels for `link`, keypoints for
`label_pack`, and a synthetic video for `propagate`.  Nothing here touches a device; every case is built once and frozen."""
import collections
import functools

import numpy as np

SMALL = (96, 54)                 # a key range where collisions are common
FULL = (1920, 1080)              # the labeller's frames
SIZES = (0, 1, 255, 256, 257, 1000, 4097)   # workgroup edges, and one past the 4096-row chunk of the compacting kernels

Case = collections.namedtuple("Case", "name lab0 lab1 width height")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _labels(rng, n, m, width, height, shared=0.3):
    """n and m rows with mid points inside the frame: about `shared` of lab1's mid points are copies of lab0's (shared keys), every
    seventh / fifth mid x sits on a half pixel, the outer points are anywhere"""
    lab0 = rng.uniform(0.0, [width - 1, height - 1, width - 1, height - 1], (n, 4)).astype(np.float32)
    lab1 = rng.uniform(0.0, [width - 1, height - 1, width - 1, height - 1], (m, 4)).astype(np.float32)
    lab0[::7, 2] = np.floor(lab0[::7, 2]) + np.float32(0.5)
    lab1[::5, 0] = np.floor(lab1[::5, 0]) + np.float32(0.5)
    if n and m:
        k = int(round(shared * m))
        lab1[rng.permutation(m)[:k], :2] = lab0[rng.integers(0, n, k), 2:]
    return lab0, lab1


@functools.lru_cache(maxsize=None)
def random_case(n, m, size=SMALL, seed=0):
    lab0, lab1 = _labels(np.random.default_rng([seed, n, m, size[0]]), n, m, *size)
    _freeze(lab0, lab1)
    return Case(f"random-{n}x{m}-{size[0]}", lab0, lab1, *size)


@functools.lru_cache(maxsize=None)
def half_integer_case():
    """mid x in 0.5, 1.5, 2.5, ...: round half to even sends 0.5 -> 0, 1.5 -> 2, 2.5 -> 2"""
    w, h = SMALL
    xs = (np.arange(40, dtype=np.float32) % 20) + np.float32(0.5)
    ys = (np.arange(40, dtype=np.float32) // 20) + np.float32(2.5)
    lab0 = np.stack([np.arange(40), np.arange(40) + 100, xs, ys], 1).astype(np.float32)
    lab1 = np.stack([np.arange(20, dtype=np.float32), np.full(20, 2.0), np.arange(20) + 200, np.arange(20) + 300], 1).astype(np.float32)
    _freeze(lab0, lab1)
    return Case("half-integer", lab0, lab1, w, h)


@functools.lru_cache(maxsize=None)
def one_key_case(rows=300):
    """`rows` rows of either side on one key (sub-pixel offsets that round to the same pixel) among 200 others: the last wins"""
    w, h = SMALL
    rng = np.random.default_rng(5)
    lab0, lab1 = _labels(rng, rows + 200, rows + 150, w, h)
    at0, at1 = rng.permutation(rows + 200)[:rows], rng.permutation(rows + 150)[:rows]
    lab0[at0, 2:] = np.array([17.0, 9.0], dtype=np.float32) + rng.uniform(-0.4, 0.4, (rows, 2)).astype(np.float32)
    lab1[at1, :2] = np.array([17.0, 9.0], dtype=np.float32) + rng.uniform(-0.4, 0.4, (rows, 2)).astype(np.float32)
    _freeze(lab0, lab1)
    return Case("one-key", lab0, lab1, w, h)


@functools.lru_cache(maxsize=None)
def alias_case():
    """mid x that rounds to the width: (w, y) shares the key of (0, y + 1), in the last row too (the top of the key range)"""
    w, h = SMALL
    lab0 = np.array([[1, 1, w - 0.3, 4.0], [2, 2, 5.0, 6.0], [3, 3, w - 0.5, h - 1.0], [4, 4, w + 0.2, h]], dtype=np.float32)
    lab1 = np.array([[0.2, 5.0, 10, 10], [5.0, 6.0, 20, 20], [0.0, h, 30, 30], [w, 5.0, 40, 40]], dtype=np.float32)
    _freeze(lab0, lab1)
    return Case("alias", lab0, lab1, w, h)


@functools.lru_cache(maxsize=None)
def no_shared_case():
    w, h = SMALL
    lab0, lab1 = _labels(np.random.default_rng(6), 300, 280, w, h, shared=0.0)
    lab0[:, 2] = np.floor(lab0[:, 2] / 2) * 2            # even pixels on one side, odd ones on the other
    lab1[:, 0] = np.floor(lab1[:, 0] / 2) * 2 + 1
    _freeze(lab0, lab1)
    return Case("no-shared", lab0, lab1, w, h)


@functools.lru_cache(maxsize=None)
def dropped_case():
    """the one case with unusable keys: NaN, +-inf, a negative key, keys past w * (h + 1), a huge coordinate -> (case, usable rows of
    lab0 [bool], usable rows of lab1 [bool])"""
    w, h = SMALL
    lab0, lab1 = _labels(np.random.default_rng(8), 400, 380, w, h)
    bad0 = {3: (np.nan, 4.0), 17: (5.0, np.nan), 64: (np.inf, 1.0), 65: (-np.inf, 1.0), 128: (-1.0, 0.0), 255: (1.0, h + 1.0),
            256: (w + 1.0, h), 300: (3e38, 3e38), 399: (2.0, -1.0)}
    bad1 = {0: (np.nan, np.nan), 63: (0.0, h + 2.0), 64: (-0.6, 0.0), 379: (1e30, 0.0)}
    for rows, lab, c in ((bad0, lab0, 2), (bad1, lab1, 0)):
        for r, xy in rows.items():
            lab[r, c:c + 2] = xy
    ok0, ok1 = np.ones(400, dtype=bool), np.ones(380, dtype=bool)
    ok0[list(bad0)], ok1[list(bad1)] = False, False
    _freeze(lab0, lab1, ok0, ok1)
    return Case("dropped", lab0, lab1, w, h), ok0, ok1


def link_cases():
    """every case whose keys are all usable"""
    out = [random_case(n, m) for n, m in ((1000, 900), (257, 255), (0, 10), (10, 0), (0, 0), (1, 1), (1, 300), (300, 1))]
    return out + [random_case(3000, 2500, FULL), half_integer_case(), one_key_case(), alias_case(), no_shared_case()]


# ---- label_pack ---------------------------------------------------------------------------------------------------------------------
AFFINE = (1920 / 1333, 1080 / 750, 12.0, 7.5, 1920 / 1301, 1080 / 731, -3.25, 0.1)   # scales that are not exact in binary
VRATIO = 720 / 1080


@functools.lru_cache(maxsize=None)
def pack_case(n, seed=1):
    """n matches of a 1333 x 750 frame pair: a third static within a pixel (watermarks), some exactly one pixel apart in one
    coordinate (the edge of `< 1`), one NaN row -> (k0, k1 fp32 [n,2], keep uint8 [n])"""
    rng = np.random.default_rng([seed, n])
    k0 = rng.uniform(0.0, [1332.0, 749.0], (n, 2)).astype(np.float32)
    k1 = rng.uniform(0.0, [1332.0, 749.0], (n, 2)).astype(np.float32)
    still = rng.random(n) < 1 / 3
    k1[still] = k0[still] + rng.uniform(-0.99, 0.99, (int(still.sum()), 2)).astype(np.float32)
    k0[::11] = np.floor(k0[::11])
    k1[::11] = k0[::11] + np.array([1.0, 0.25], dtype=np.float32)
    if n > 2:
        k0[n // 2] = np.nan
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    _freeze(k0, k1, keep)
    return k0, k1, keep


# ---- a synthetic video for propagate ---------------------------------------------------------------------------------------------------
VIDEO_SKIPS = [1, 2, 4]          # standing in for 10 / 20 / 40
VIDEO_FRAMES = 13
VIDEO_MIN_FINAL = 8
VIDEO_MISSING = (5, 6)           # the skip-1 pair no source labelled


@functools.lru_cache(maxsize=None)
def video():
    """Integer-pixel tracks in a 96 x 54 video of 13 frames, every track moving one pixel per frame in x.  60 tracks live in frames
    0-9, 60 in frames 7-12 and only 3 in all frames: a label that reaches frame 8 from frame 0 shares 3 < VIDEO_MIN_FINAL rows with
    any label that leaves frame 8 for frame 10 or later, so that hop fails and the fall-back shortens it.  Every frame pair of every
    skip is labelled by one source (skip 1: two sources) with 85 % of the tracks it could see, in shuffled order, except
    VIDEO_MISSING.  -> {skip: {(idx0, idx1): [fp32 [n,4], ...]}}"""
    rng = np.random.default_rng(11)
    w, h = SMALL
    cells = rng.permutation((w - VIDEO_FRAMES - 12) * h)[:123]
    base = np.stack([cells % (w - VIDEO_FRAMES - 12), cells // (w - VIDEO_FRAMES - 12)], 1).astype(np.float32)
    first = np.array([0] * 60 + [7] * 60 + [0] * 3)
    last = np.array([9] * 60 + [12] * 60 + [12] * 3)
    labels = {}
    for skip in VIDEO_SKIPS:
        labels[skip] = {}
        for f in range(VIDEO_FRAMES - skip):
            g = f + skip
            if skip == 1 and (f, g) == VIDEO_MISSING:
                continue
            alive = np.flatnonzero((first <= f) & (last >= g))
            sources = []
            for _ in range(2 if skip == 1 else 1):
                seen = rng.permutation(alive[rng.random(len(alive)) < 0.85])
                row = np.concatenate([base[seen] + np.float32([f, 0]), base[seen] + np.float32([g, 0])], 1).astype(np.float32)
                row.setflags(write=False)
                sources.append(row)
            labels[skip][(f, g)] = sources
    return labels


def video_store():
    """the video's labels in a fresh gim_amd.video_labels.LabelStore"""
    from gim_amd.video_labels import LabelStore
    store = LabelStore()
    for skip, pairs in video().items():
        for pair, sources in pairs.items():
            for a in sources:
                store.put(skip, pair, a)
    return store


# (idx0, idx1, skips) of the propagate tests, host and device: the whole video, its parts around the missing pair and the failing hop,
# shorter skip lists, an end that no skip reaches exactly, an empty span
PROPAGATE_REQUESTS = [(0, 12, VIDEO_SKIPS), (0, 8, VIDEO_SKIPS), (4, 12, VIDEO_SKIPS), (8, 12, VIDEO_SKIPS), (0, 11, VIDEO_SKIPS),
                      (1, 7, VIDEO_SKIPS[:2]), (4, 8, VIDEO_SKIPS[:2]), (5, 6, VIDEO_SKIPS[:1]), (3, 9, VIDEO_SKIPS[:1]), (2, 2, VIDEO_SKIPS)]


# ---- label_pair -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_scene(seed=3, inliers=210, outliers=90, watermarks=50):
    """a two-view scene of tests/fundamental_cases.py as a matcher would report it: exact matches, 30 % uniform outliers and 50 static
    "watermark" matches within a pixel of each other, shuffled, fp32 -> (k0, k1 [350,2], static [350] bool)"""
    import fundamental_cases as F
    rng = np.random.default_rng(seed)
    n = inliers + outliers
    p0, p1, _ = F.two_views(rng, n)
    p1[inliers:] = rng.uniform([0.0, 0.0], [F.W, F.H_IMG], (outliers, 2))
    w0 = rng.uniform([0.0, 0.0], [F.W, F.H_IMG], (watermarks, 2))
    w1 = w0 + rng.uniform(-0.9, 0.9, (watermarks, 2))
    order = rng.permutation(n + watermarks)
    k0 = np.concatenate([p0, w0])[order].astype(np.float32)
    k1 = np.concatenate([p1, w1])[order].astype(np.float32)
    static = (np.arange(n + watermarks) >= n)[order]
    _freeze(k0, k1, static)
    return k0, k1, static
