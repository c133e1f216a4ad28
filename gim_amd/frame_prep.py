"""Frame preparation of the video labeller: the stretch between a decoded frame and a matcher's input (the reference's
video_preprocessor.py:292-366, the per-method inputs at :406-493 and read_segmentation_image at :603-621) -- crop to a box, area
resize, the class-exclusion mask through the reference's two nearest-neighbour resizes, LoFTR's 1/8 mask, and the fp32 tensors the
matchers and the segmenter take.  On the host in numpy (`frame_prep_np`, product code and the CPU oracle of the kernel, as pose.*_ge
are) or on a device through csrc/frame_prep.hip (`plan` + ops.frame_prep).  csrc/frame_prep_math.h is the arithmetic restated here.

The resize is a written contract, not cv2.resize's bytes: per axis destination index d of m over a source extent n covers
[d s, min((d + 1) s, n)) with s = n / m in double, every source index under it weighs its covered share (a double expression rounded
once to fp32), rows are summed in fp32 left to right, then the rows top to bottom, no fused multiply-add, rintf, clamp.  For an integer
factor that is the mean, below 1 the coverage rule INTER_AREA applies when it zooms.  OpenCV rounds 1 / (dst / src) in double before the
floor of its nearest-neighbour index and has a separate integer-factor path for bytes; neither is restated.

`get_resized_wh` here is video_preprocessor.py:586-591 (fit into a [h, w] box); zeb_data.get_resized_wh is datasets/utils.py's (a long
side) and `get_divisible_wh` is shared with it.
"""
import numpy as np

from .zeb_data import get_divisible_wh  # noqa: F401  (video_preprocessor.py:594-600 is datasets/utils.py:43-54)

MAX_FACTOR = 16                  # csrc/frame_prep_math.h GIM_FP_MAX_FACTOR
TAPS = MAX_FACTOR + 2            # GIM_FP_TAPS
TILE_W, TILE_H = 64, 16          # GIM_FP_TILE_W / _H
LDS_BYTES = 40960                # GIM_FP_LDS_BYTES
JOB_WORDS = 16                   # GIM_FP_JOB_WORDS
OUT_U8, OUT_MASK, OUT_MASK8, OUT_RGB, OUT_GRAY, OUT_NORM, MASKED = 1, 2, 4, 8, 16, 32, 64
OUTPUTS = ("u8", "mask", "mask8", "rgb", "gray", "norm")       # in the order of the flag bits
ALL_FLAGS = 127
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def get_resized_wh(w, h, resize):
    """video_preprocessor.py:586-591: the size that fits (w, h) into resize = [nh, nw], aspect kept"""
    nh, nw = resize
    scale = min(nh / h, nw / w)
    return int(round(w * scale)), int(round(h * scale))


def exclude_table(exclude):
    """a 256-byte table, non-zero: the class is excluded.  `exclude`: such a table (uint8 [256]) or class ids"""
    a = np.asarray(exclude)
    if a.dtype == np.uint8 and a.shape == (256,):
        return np.ascontiguousarray(a)
    t = np.zeros(256, dtype=np.uint8)
    ids = a.astype(np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() > 255):
        raise ValueError(f"exclude: class ids in [0, 255], got {ids.tolist()}")
    t[ids] = 1
    return t


# ---- the contract's arithmetic (csrc/frame_prep_math.h) ------------------------------------------------------------------------------
def area_weights(n, m):
    """the coverage table of one axis, source extent n -> destination extent m: (k0 int64 [m], count int64 [m], w fp32 [m, K]) with
    K = count.max(); w[d, i] is the weight of source index k0[d] + i, 0 beyond count[d] (gim_fp_span / gim_fp_weight)"""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"area_weights: extents {n} -> {m} (both >= 1)")
    if n > MAX_FACTOR * m:
        raise ValueError(f"area_weights: {n} -> {m} shrinks the axis by more than {MAX_FACTOR}")
    s = np.float64(n) / np.float64(m)
    d = np.arange(m, dtype=np.float64)
    a = d * s
    b = np.minimum((d + 1.0) * s, np.float64(n))
    k0 = np.floor(a).astype(np.int64)
    count = np.ceil(b).astype(np.int64) - k0
    assert count.min() >= 1 and count.max() <= TAPS - 1, (n, m, int(count.min()), int(count.max()))
    k = k0[:, None] + np.arange(int(count.max()), dtype=np.int64)[None]
    kf = k.astype(np.float64)
    w = ((np.minimum(b[:, None], kf + 1.0) - np.maximum(a[:, None], kf)) / (b - a)[:, None]).astype(np.float32)
    w[np.arange(w.shape[1])[None] >= count[:, None]] = 0.0
    return k0, count, w


def area_resize(src, wn, hn):
    """src uint8 [hc, wc, C] -> uint8 [hn, wn, C] by the contract: t_y = sum_k wx_k * float(src[y, k]) in fp32 with k ascending, then
    v = sum_y wy_y * t_y with y ascending, each product and each sum rounded to fp32, then rint and the clamp to a byte"""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3:
        raise ValueError(f"area_resize: uint8 [h, w, c], got {src.dtype} {src.shape}")
    hc, wc = src.shape[:2]
    kx, cx, wx = area_weights(wc, wn)
    ky, cy, wy = area_weights(hc, hn)
    f = src.astype(np.float32)
    t = np.zeros((hc, wn, src.shape[2]), dtype=np.float32)
    for i in range(wx.shape[1]):                       # a term beyond a pixel's count adds +0 to a sum that is never -0: no change
        p = wx[:, i][None, :, None] * f[:, np.minimum(kx + i, wc - 1), :]
        t = t + p
    v = np.zeros((hn, wn, src.shape[2]), dtype=np.float32)
    for i in range(wy.shape[1]):
        p = wy[:, i][:, None, None] * t[np.minimum(ky + i, hc - 1)]
        v = v + p
    return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)


def mask_index(nn, lo, nc, nf, ns):
    """the class-map index under every output index of one axis (gim_fp_mask_index): resize to the frame, crop, resize to the output,
    each nearest-neighbour with an integer floor.  nn: output extent, [lo, lo + nc): the crop, nf: frame extent, ns: class-map extent"""
    j = np.arange(int(nn), dtype=np.int64)
    c = int(lo) + np.minimum(j * int(nc) // int(nn), int(nc) - 1)
    return np.minimum(c * int(ns) // int(nf), int(ns) - 1)


def gray_u8(u8):
    """cv2.cvtColor(RGB2GRAY) on bytes: (4899 r + 9617 g + 1868 b + 8192) >> 14"""
    c = u8.astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def _check_job(frame_hw, box, size, flags):
    H, W = frame_hw
    x0, y0, x1, y1 = (int(v) for v in box)
    wn, hn = (int(v) for v in size)
    flags = int(flags)
    if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f"frame_prep: box {(x0, y0, x1, y1)} in a {W} x {H} frame")
    if wn < 1 or hn < 1:
        raise ValueError(f"frame_prep: output size {wn} x {hn}")
    if x1 - x0 > MAX_FACTOR * wn or y1 - y0 > MAX_FACTOR * hn:
        raise ValueError(f"frame_prep: {x1 - x0} x {y1 - y0} -> {wn} x {hn} shrinks an axis by more than {MAX_FACTOR}")
    if flags < 0 or flags & ~ALL_FLAGS:
        raise ValueError(f"frame_prep: flags {flags}")
    if flags & OUT_MASK8 and (wn % 8 or hn % 8):
        raise ValueError(f"frame_prep: mask8 needs an output of multiples of 8, got {wn} x {hn}")
    return (x0, y0, x1, y1), (wn, hn), flags


def frame_prep_np(frame, seg, exclude, box, size, flags):
    """One job of gim_frame_prep in numpy, the same fp32 order -> {name: array} of the outputs `flags` asks for, and `kept`.
    frame uint8 [H, W, 3] RGB; seg uint8 [Hs, Ws] class map or None (then every mask is 1); exclude: `exclude_table`'s argument;
    box (x0, y0, x1, y1) or None: the whole frame; size (wn, hn); flags: OUT_* or-ed, MASKED to multiply rgb and gray by the mask.
      u8 uint8 [hn, wn, 3], mask uint8 [hn, wn], mask8 uint8 [hn / 8, wn / 8] = mask[::8, ::8], rgb fp32 [3, hn, wn] = (u8 * m) / 255,
      gray fp32 [1, hn, wn] = (grey * m) / 255, norm fp32 [3, hn, wn] = (u8 / 255 - mean) / std, kept = mask.sum()"""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"frame_prep: frame must be uint8 [H, W, 3], got {frame.dtype} {frame.shape}")
    H, W = frame.shape[:2]
    (x0, y0, x1, y1), (wn, hn), flags = _check_job((H, W), box if box is not None else (0, 0, W, H), size, flags)
    u8 = area_resize(frame[y0:y1, x0:x1], wn, hn)
    if seg is None:
        mask = np.ones((hn, wn), dtype=np.uint8)
    else:
        seg = np.asarray(seg)
        if seg.dtype != np.uint8 or seg.ndim != 2:
            raise ValueError(f"frame_prep: seg must be uint8 [Hs, Ws], got {seg.dtype} {seg.shape}")
        sy = mask_index(hn, y0, y1 - y0, H, seg.shape[0])
        sx = mask_index(wn, x0, x1 - x0, W, seg.shape[1])
        mask = (exclude_table(exclude)[seg[sy[:, None], sx[None]]] == 0).astype(np.uint8)
    m = mask if flags & MASKED else np.ones_like(mask)
    out = {"kept": int(mask.sum(dtype=np.int64))}
    if flags & OUT_U8:
        out["u8"] = u8
    if flags & OUT_MASK:
        out["mask"] = mask
    if flags & OUT_MASK8:
        out["mask8"] = np.ascontiguousarray(mask[::8, ::8])
    if flags & OUT_RGB:
        out["rgb"] = np.ascontiguousarray(((u8 * m[..., None]).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
    if flags & OUT_GRAY:
        out["gray"] = ((gray_u8(u8) * m).astype(np.float32) / np.float32(255.0))[None]
    if flags & OUT_NORM:
        out["norm"] = np.ascontiguousarray(((u8.astype(np.float32) / np.float32(255.0) - MEAN) / STD).transpose(2, 0, 1))
    return out


# ---- the job and work tables of ops.frame_prep -----------------------------------------------------------------------------------------
def tile_bytes(tw, th, wc, wn, hc, hn):
    """gim_fp_tile_bytes: the LDS bound of a tile's source footprint"""
    sx, sy = np.float64(wc) / np.float64(wn), np.float64(hc) / np.float64(hn)
    cols, rows = int(np.ceil(np.float64(tw) * sx)) + 2, int(np.ceil(np.float64(th) * sy)) + 2
    return rows * (((cols * 3 + 15 + 15) // 16) * 16)


def choose_tile(wc, hc, wn, hn):
    """gim_frame_prep_tile: the largest tile, halving th and then tw from 64 x 16, whose footprint fits the kernel's LDS"""
    tw, th = TILE_W, TILE_H
    while tile_bytes(tw, th, wc, wn, hc, hn) > LDS_BYTES and (tw > 1 or th > 1):
        if th > 1:
            th >>= 1
        else:
            tw >>= 1
    if tile_bytes(tw, th, wc, wn, hc, hn) > LDS_BYTES:
        raise ValueError(f"frame_prep: no tile fits {wc} x {hc} -> {wn} x {hn}")
    return tw, th


class Plan:
    """jobs int64 [J, 16] and work int32 [n_work, 4] as gim_frame_prep reads them, the elements of the six ragged output buffers, and
    per job the (offset, shape) of every output it asked for"""

    def __init__(self, jobs, work, elems, views):
        self.jobs, self.work, self.elems, self.views = jobs, work, elems, views


def plan(frame_hw, jobs, align=4, guard=0):
    """The job and work tables of a batch, built on the host.  frame_hw: (H, W) of the frame slab; jobs: a sequence of
    (slot, box | None, (wn, hn), flags).  Every refusal of the kernel's entry point is raised here first.  A job's outputs start at
    multiples of `align` elements of their buffer, with `guard` (a multiple of align) elements nobody writes in front and behind."""
    H, W = int(frame_hw[0]), int(frame_hw[1])
    table = np.zeros((len(jobs), JOB_WORDS), dtype=np.int64)
    elems = [0] * 6
    work, views = [], []
    for j, (slot, box, size, flags) in enumerate(jobs):
        (x0, y0, x1, y1), (wn, hn), flags = _check_job((H, W), box if box is not None else (0, 0, W, H), size, flags)
        tw, th = choose_tile(x1 - x0, y1 - y0, wn, hn)
        shapes = ((hn, wn, 3), (hn, wn), (hn // 8, wn // 8), (3, hn, wn), (1, hn, wn), (3, hn, wn))
        offs, view = [0] * 6, {}
        for o, shape in enumerate(shapes):
            if flags & (1 << o):
                offs[o] = elems[o] + guard
                view[OUTPUTS[o]] = (offs[o], shape)
                elems[o] += 2 * guard + -(-int(np.prod(shape)) // align) * align
        table[j] = [int(slot), x0, y0, x1, y1, wn, hn, flags, *offs, tw, th]
        views.append(view)
        work += [(j, ox, oy, 0) for oy in range(0, hn, th) for ox in range(0, wn, tw)]
    return Plan(table, np.asarray(work, dtype=np.int32).reshape(-1, 4), elems, views)
