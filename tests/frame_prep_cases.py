"""The seeded cases of the frame-preparation tests (tests/test_frame_prep_cpu.py, tests/test_gpu_frame_prep.py): the smallest shapes at
which gim_frame_prep can go wrong.  T = (64, 16) is the kernel's largest tile (frame_prep.TILE_W / TILE_H).

A case is a dict: frame uint8 [H, W, 3], seg uint8 [Hs, Ws], exclude (class ids), box, size (wn, hn), flags.  Frames are uniform random
bytes, except that the integer-factor cases nudge one byte of every source block whose sum would make the mean an exact half (with
an even block size a quarter of all means would otherwise be ties, where the band of the fp64 comparison could not be capped)."""
import numpy as np

from gim_amd import frame_prep as fp

ALL = fp.ALL_FLAGS
NO8 = ALL & ~fp.OUT_MASK8                  # sizes that are no multiple of 8 cannot have the 1/8 mask
CLASSES = 7
EXCLUDE = [2, 5]


def _frame(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _seg(seed, Hs, Ws):
    return np.random.default_rng(seed + 7919).integers(0, CLASSES, (Hs, Ws), dtype=np.uint8)


def _no_ties(frame, box, fx, fy):
    """nudge one byte of every fx x fy block of the box whose sum is an odd multiple of fx * fy / 2"""
    x0, y0, x1, y1 = box
    n = fx * fy
    if n % 2:
        return frame
    frame = frame.copy()
    for y in range(y0, y1, fy):
        for x in range(x0, x1, fx):
            for c in range(3):
                if int(frame[y:y + fy, x:x + fx, c].sum()) % n == n // 2:
                    frame[y, x, c] = frame[y, x, c] + 1 if frame[y, x, c] < 255 else 254
    return frame


def _case(name, seed, hw, seg_hw, box, size, flags=None, exclude=EXCLUDE, integer=None):
    H, W = hw
    frame = _frame(seed, H, W)
    box = (0, 0, W, H) if box is None else box
    if integer:
        frame = _no_ties(frame, box, *integer)
    if flags is None:
        flags = ALL if size[0] % 8 == 0 and size[1] % 8 == 0 else NO8
    return {"name": name, "frame": frame, "seg": _seg(seed, *seg_hw), "exclude": exclude, "box": box, "size": size, "flags": flags,
            "integer": integer}


def cases():
    T = (fp.TILE_W, fp.TILE_H)
    out = [
        _case("fractional", 1, (40, 50), (40, 50), (3, 4, 40, 33), (16, 8)),                       # 37 x 29 -> 16 x 8
        _case("integer", 2, (40, 50), (40, 50), (6, 8, 38, 24), (16, 8), integer=(2, 2)),          # 32 x 16 -> 16 x 8
        _case("identity", 3, (24, 32), (24, 32), None, (32, 24), integer=(1, 1)),
        _case("up", 4, (40, 50), (40, 50), (20, 11, 31, 18), (16, 8)),                             # 11 x 7 -> 16 x 8
        _case("down-x-up-y", 5, (40, 50), (40, 50), (5, 20, 45, 27), (16, 8)),                     # 40 x 7 -> 16 x 8
        _case("border-left-top", 6, (40, 50), (40, 50), (0, 0, 23, 19), (16, 8)),
        _case("border-right-bottom", 7, (40, 50), (40, 50), (27, 21, 50, 40), (16, 8)),
        _case("border-all", 8, (40, 50), (40, 50), (0, 0, 50, 40), (24, 16)),
        _case("one-pixel", 9, (40, 50), (40, 50), (49, 39, 50, 40), (8, 8)),
        _case("one-wide", 10, (40, 50), (40, 50), (17, 3, 18, 36), (5, 11)),
        _case("one-high", 11, (40, 50), (40, 50), (3, 17, 44, 18), (13, 3)),
        _case("factor-16", 12, (64, 128), (64, 128), (0, 0, 128, 64), (8, 4), integer=(16, 16)),
        _case("factor-16-x", 13, (40, 160), (40, 160), (0, 3, 160, 36), (10, 24)),                 # 16 in x, 1.375 in y
        _case("seg-smaller", 14, (40, 50), (13, 17), (3, 4, 40, 33), (16, 8)),
        _case("seg-larger", 15, (40, 50), (97, 121), (3, 4, 40, 33), (16, 8)),
        _case("all-excluded", 16, (40, 50), (40, 50), (3, 4, 40, 33), (16, 8), exclude=list(range(256))),
        _case("none-excluded", 17, (40, 50), (40, 50), (3, 4, 40, 33), (16, 8), exclude=[]),
        _case("unmasked", 18, (40, 50), (40, 50), (3, 4, 40, 33), (16, 8), flags=ALL & ~fp.MASKED),
    ]
    for k, (dw, dh) in enumerate([(-1, -1), (0, 0), (1, 1), (1, -1), (-1, 1)]):                    # T - 1, T, T + 1 on both axes
        out.append(_case(f"tile{dw:+d}{dh:+d}", 20 + k, (60, 190), (31, 95), (2, 1, 187, 58), (T[0] + dw, T[1] + dh)))
    out.append(_case("tiles-2x3", 30, (60, 190), (60, 190), (0, 0, 190, 60), (2 * T[0] + 8, 3 * T[1] - 8)))   # more than one tile per axis
    return out


REFUSED = [((0, 0, 129, 8), (8, 8)), ((0, 0, 8, 33), (8, 2))]     # above factor 16 in x, in y: refused before a launch (frame 40 x 160)


def ragged_batch():
    """six jobs over three slots, one slot used twice over (slot 1 three times), every output subset once -> (frames [3, H, W, 3],
    seg [3, Hs, Ws], exclude, jobs)"""
    H, W, Hs, Ws = 40, 50, 20, 30
    frames = np.stack([_frame(40 + s, H, W) for s in range(3)])
    seg = np.stack([_seg(40 + s, Hs, Ws) for s in range(3)])
    jobs = [
        (0, (3, 4, 40, 33), (16, 8), fp.OUT_U8),
        (1, None, (24, 16), fp.OUT_MASK | fp.OUT_MASK8),
        (2, (20, 11, 31, 18), (16, 8), fp.OUT_RGB | fp.MASKED),
        (1, (5, 20, 45, 27), (13, 9), fp.OUT_GRAY | fp.OUT_NORM),
        (0, (0, 0, 50, 40), (66, 17), NO8),
        (1, (27, 21, 50, 40), (16, 8), ALL & ~fp.MASKED),
    ]
    return frames, seg, EXCLUDE, jobs
