"""Video pseudo-labels: the labeller's tail, `link` and `propagate` (the reference's video_preprocessor.py:513-566 and
datasets/walk/walk.py:29,170-266), on the host in numpy or on a device through csrc/label_link.hip.

A label is an fp32 [n,4] array of matches (x0, y0, x1, y1) of a frame pair in the pixels of the frames the labels were written in.
`link` joins the labels of a->b and b->c into a->c through the rounded pixels they share in b; `propagate` is the reference's
recursion of such hops over the label sets of several frame skips; `label_pair` turns one matcher output into a label.

`link` restates the reference's dicts and sets as two tables over the key range (`link_tables`; ops.label_link on the device), with
one documented difference: rows whose key is not finite or lies outside [0, width * (height + 1)] are ignored and counted where the
reference would still join them.  Everything else -- which rows join, their partners, their order, the copied bits -- is the
reference's (tests/label_link_oracle.py holds the dict / set formulation the tests compare against).

`FrameBank`, `prepare_pair` and `label_pair_list` are the loop in front of that tail (video_preprocessor.py:255-566 without decoding):
frames uploaded and segmented once, both sides of a pair prepared in one launch (gim_amd/frame_prep.py, csrc/frame_prep.hip), the
matcher behind a `match(inputs)` callable, the reference's files.

Not here: video decoding and frame selection, the pair-id selection of walk.py:115-128, the debug figure, MAGSAC scoring
(`label_pair` runs plain RANSAC), the SIFT detector (OpenCV's, where it imports), and a lockstep `propagate` over many pairs
(ops.label_link takes B links per call for it).
"""
import collections
import os

import numpy as np

from ._lib import GimHipError  # noqa: F401
from .bank import SlotBank

LABEL_MAX_KEY = 1 << 24


# ---- numpy restatement of csrc/label_key.h -----------------------------------------------------------------------------------------
def label_keys(x, y, width):
    """np.round(x) + np.round(y) * width in fp32 (walk.py:29): round half to even, one product, one sum"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (np.rint(x) + (np.rint(y) * np.float32(width)).astype(np.float32)).astype(np.float32)


def label_slots(keys, width, height):
    """the table slot of every key, -1 where the key is not usable (not finite, or outside [0, width * (height + 1)])"""
    with np.errstate(all="ignore"):
        ok = (keys >= np.float32(0.0)) & (keys <= np.float32(width * (height + 1)))
    return np.where(ok, np.where(ok, keys, 0).astype(np.int64), -1)


def _check_frame(width, height):
    width, height = int(width), int(height)
    if width < 1 or height < 1 or width * (height + 1) > LABEL_MAX_KEY:
        raise ValueError(f"width={width}, height={height}: both >= 1 and width * (height + 1) <= 2^24")
    return width, height


def link_tables(label0, label1, width, height):
    """The join of `link` as two tables over the key range, the CPU oracle of ops.label_link -> (out fp32 [n,4], ij int64 [n,2],
    dropped (rows of label0, rows of label1) without a usable key).  A table holds the largest row of each key (dict(zip(..)) keeps
    the last); row i of label0 survives iff it is that row of its key and label1 has the key; survivors in ascending i."""
    width, height = _check_frame(width, height)
    label0 = np.ascontiguousarray(label0, dtype=np.float32).reshape(-1, 4)
    label1 = np.ascontiguousarray(label1, dtype=np.float32).reshape(-1, 4)
    s0 = label_slots(label_keys(label0[:, 2], label0[:, 3], width), width, height)
    s1 = label_slots(label_keys(label1[:, 0], label1[:, 1], width), width, height)
    size = width * (height + 1) + 1
    t0, t1 = np.zeros(size, dtype=np.int64), np.zeros(size, dtype=np.int64)
    i0, i1 = np.flatnonzero(s0 >= 0), np.flatnonzero(s1 >= 0)
    t0[s0[i0]] = i0 + 1                                           # ascending rows: the last assignment of a slot is its largest row
    t1[s1[i1]] = i1 + 1
    i = i0[(t0[s0[i0]] == i0 + 1) & (t1[s0[i0]] > 0)]
    j = t1[s0[i]] - 1
    out = np.concatenate([label0[i, :2], label1[j, 2:]], 1)
    return out, np.stack([i, j], 1), (int((s0 < 0).sum()), int((s1 < 0).sum()))


def label_pack_np(k0, k1, keep=None, moved_thr=0.0, affine=None, vratio=1.0):
    """numpy restatement of ops.label_pack (gim_label_pack) -> the kept rows fp32 [n,4] in input order"""
    k0 = np.ascontiguousarray(k0, dtype=np.float32).reshape(-1, 2)
    k1 = np.ascontiguousarray(k1, dtype=np.float32).reshape(-1, 2)
    kept = np.ones(len(k0), dtype=bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    thr = np.float32(moved_thr)
    if thr > 0:
        with np.errstate(all="ignore"):
            d = np.abs(k0 - k1)
            kept = kept & ~((d[:, 0] < thr) & (d[:, 1] < thr))
    a, b = k0[kept], k1[kept]
    with np.errstate(all="ignore"):
        if affine is not None:
            f = np.asarray(affine, dtype=np.float64).reshape(8)
            a = (a.astype(np.float64) * f[0:2] + f[2:4]) * np.float64(vratio)
            b = (b.astype(np.float64) * f[4:6] + f[6:8]) * np.float64(vratio)
        else:
            a, b = a * np.float32(vratio), b * np.float32(vratio)
        return np.concatenate([a, b], 1).astype(np.float32)


# ---- link ---------------------------------------------------------------------------------------------------------------------------
_WORKSPACES = {}


def _workspace(device, max_keys):
    """one zeroed workspace per (device, table length): every ops.label_link call leaves it zeroed"""
    from . import ops
    key = (str(device), int(max_keys))
    if key not in _WORKSPACES:
        _WORKSPACES[key] = ops.label_link_workspace(1, max_keys, device)
    return _WORKSPACES[key]


def _writable(a):
    """contiguous fp32, copied only when torch.from_numpy could not take it (a read-only array)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if a.flags.writeable else a.copy()


def _to_device(label, device):
    import torch
    if isinstance(label, torch.Tensor):
        return label.to(device=device, dtype=torch.float32).reshape(-1, 4).contiguous()
    return torch.from_numpy(_writable(label).reshape(-1, 4)).to(device)


def link(label0, label1, width, height, min_final_matches, device=None):
    """walk.py:217-247: the label of a->c from the labels of a->b and b->c, or None when fewer than min_final_matches rows join.
    device=None: numpy (`link_tables`), arrays in and out.  With a device: ops.label_link; labels may be arrays or tensors, the
    result is a tensor on the device and the only host read is the 4-byte count."""
    if device is None:
        out = link_tables(label0, label1, width, height)[0]
        return None if len(out) < min_final_matches else out
    import torch
    from . import ops
    width, height = _check_frame(width, height)
    device = torch.device(device)
    with torch.cuda.device(device):
        a, b = _to_device(label0, device), _to_device(label1, device)
        out, _, count, _ = ops.label_link(a, b, width, height, workspace=_workspace(device, width * (height + 1) + 1))
        n = int(count.item())
    return None if n < min_final_matches else out[:n]


# ---- the label files of a video ----------------------------------------------------------------------------------------------------
class LabelStore:
    """The labels of a video by (skip, (idx0, idx1)), from any number of sources per skip (the reference: one directory per matcher
    and resize, walk.py:99-113).  `dump` is walk.py:249-266: the sources that hold the pair, concatenated as fp32.  With a device the
    concatenated label goes there on first use and stays."""

    def __init__(self):
        self._labels = {}        # (skip, (idx0, idx1)) -> [array, ...] in source order
        self._on_device = {}     # (skip, pair, device) -> tensor

    @staticmethod
    def _pair(pair):
        return int(pair[0]), int(pair[1])

    def put(self, skip, pair, array):
        """one source's label of a pair (callers that label in-process)"""
        key = (int(skip), self._pair(pair))
        self._labels.setdefault(key, []).append(np.asarray(array).reshape(-1, 4))
        for k in [k for k in self._on_device if k[:2] == key]:
            del self._on_device[k]

    @classmethod
    def from_dirs(cls, dirs):
        """{skip: [dir, ...]}: directories in the reference's layout -- nums.npy, idxs.npy [n,2] and one
        str(np.array(pair)) + '.npy' per labelled pair (video_preprocessor.py:555-566)"""
        store = cls()
        for skip, paths in dirs.items():
            for path in paths:
                for name in ("nums.npy", "idxs.npy"):
                    if not os.path.exists(os.path.join(path, name)):
                        raise FileNotFoundError(os.path.join(path, name))
                for pair in np.load(os.path.join(path, "idxs.npy")).reshape(-1, 2):
                    p = os.path.join(path, "{}.npy".format(str(np.array(pair))))
                    if os.path.exists(p):
                        store.put(skip, pair, np.load(p))
        return store

    def pairs(self, skip):
        return sorted(p for s, p in self._labels if s == int(skip))

    def dump(self, skip, pair, device=None):
        """the pair's label over all sources, fp32 [n,4] (an empty list when no source has it, as the reference returns)"""
        key = (int(skip), self._pair(pair))
        if key not in self._labels:
            return []
        if device is None:
            return np.concatenate(self._labels[key], axis=0).astype(np.float32)
        dkey = key + (str(device),)
        if dkey not in self._on_device:
            self._on_device[dkey] = _to_device(np.concatenate(self._labels[key], axis=0).astype(np.float32), device)
        return self._on_device[dkey]


def propagate(store, idx0, idx1, skips, *, width, height, min_final_matches, device=None):
    """walk.py:170-215: the label of (idx0, idx1) chained from the labels of the frame skips `skips` (ascending; the last one is walked,
    the shorter ones fill in recursively) -> (label | None, id0, id1); the ids are the frames the label actually spans.  Same control
    flow as the reference, every hop through `link`.  On a device the growing label stays there: the host reads only the hops' 4-byte
    counts."""
    skips = list(skips)
    skip, rest = skips[-1], skips[:-1]
    # the hops: idx0, idx0 + skip, ... and a shorter last one when idx1 is not reached exactly
    stops = list(range(idx0, idx1 + 1, skip)) if idx1 >= idx0 else [idx0]
    if stops[-1] != idx1:
        stops.append(idx1)
    hops = collections.deque(zip(stops[:-1], stops[1:]))
    if device is None:
        cat = lambda parts: np.concatenate(parts, axis=0)   # noqa: E731
    else:
        import torch
        cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, 0)   # noqa: E731

    chain, end = None, None                       # the label carried so far; it counts as spanning idx0 .. end
    while hops:
        a, b = hops.popleft()
        if a == b:
            break
        parts = []
        if b - a == skip:                         # a labelled pair of this skip ...
            direct = store.dump(skip, (a, b), device)
            if len(direct) > 0:
                parts.append(direct)
        if rest:                                  # ... and what the shorter skips chain across the same hop
            sub, s0, s1 = propagate(store, a, b, rest, width=width, height=height, min_final_matches=min_final_matches, device=device)
            if (s0, s1) == (a, b):
                parts.append(sub)
        if not parts:
            continue                              # a hop without a label is passed over: the carried label keeps its start
        hop = cat(parts)
        if chain is None:
            chain, end = hop, b
            continue
        joined = link(chain, hop, width, height, min_final_matches, device)
        if joined is not None:
            chain, end = joined, b
        else:                                     # the reference's fall-back: drop the hop, try once more ending skips[0] earlier
            hops = collections.deque([(a, b - skips[0])])
    if chain is None:
        return None, None, None
    return chain, idx0, end


# ---- one labelling step --------------------------------------------------------------------------------------------------------------
def _keypoints(matcher_out):
    if isinstance(matcher_out, dict):
        if "mkpts0_f" not in matcher_out or "mkpts1_f" not in matcher_out:
            raise ValueError(f"label_pair: no mkpts0_f / mkpts1_f among {sorted(matcher_out)}")
        return matcher_out["mkpts0_f"], matcher_out["mkpts1_f"]
    k0, k1 = matcher_out
    return k0, k1


def label_pair(matcher_out, *, device, affine=None, vratio=1.0, threshold=0.5, confidence=0.999999, max_iters=100000, seed=0,
               refine=0, score="count"):
    """The tail of a labelling step (video_preprocessor.py:513-555) for one frame pair -> label fp32 [n,4] on the device.
    matcher_out: a matcher's result dict (`mkpts0_f` / `mkpts1_f`, matched keypoints [n,2] in pixels) or a (k0, k1) pair.
      1. ops.label_pack with moved_thr = 1 drops static matches (watermarks, line 516);
      2. pose.find_fundamental_mat(solve="device", sampler="device") on the survivors, where the reference calls
         cv2.findFundamentalMat(USAC_MAGSAC, 0.5, 0.999999, 100000): score="count" (the default) is plain RANSAC with the Sampson
         distance; score="magsac" ranks the hypotheses by the MAGSAC++ loss on the device (gim_magsac_score: the published closed
         form, not cv2's bytes) -- at 0.5 px an inlier count picks among near-ties arbitrarily, the marginalised score prefers the
         model whose inliers are tight;
         refine = R in 1 .. 8 adds the step USAC ends with, up to R rounds of eight-point refit on the inliers in the launch that
         takes the mask (pose.find_fundamental_mat's `refine`; 0, the default, keeps the minimal-sample model's mask);
      3. ops.label_pack with the inlier mask and the rescale: `affine` (sx0, sy0, ox0, oy0, sx1, sy1, ox1, oy1) and `vratio` of
         line 549, or `vratio` alone (line 552).
    Fewer than 7 survivors, or no model: an empty label, without the second launch."""
    import torch
    from . import ops, pose
    points = _keypoints(matcher_out)
    device = torch.device(device)
    with torch.cuda.device(device):
        k0, k1 = (t.to(device=device, dtype=torch.float32).reshape(-1, 2).contiguous() if isinstance(t, torch.Tensor)
                  else torch.from_numpy(_writable(t).reshape(-1, 2)).to(device) for t in points)
        moved, count = ops.label_pack(k0, k1, moved_thr=1.0)
        n = int(count.item())
        empty = torch.empty(0, 4, dtype=torch.float32, device=device)
        if n < 7:
            return empty
        moved = moved[:n]
        pts = moved.cpu().numpy().astype(np.float64)
        F, mask = pose.find_fundamental_mat(pts[:, :2], pts[:, 2:], threshold=threshold, prob=confidence, max_iters=max_iters, seed=seed,
                                            device=device, solve="device", sampler="device", refine=refine, score=score)
        if F is None or not mask.any():
            return empty
        m0, m1 = moved[:, :2].contiguous(), moved[:, 2:].contiguous()
        keep = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(device)
        out, count = ops.label_pack(m0, m1, keep=keep, affine=affine, vratio=vratio)
        return out[:int(count.item())]


# ---- frames on the device, the inputs of a pair, the labelling loop ---------------------------------------------------------------------
METHODS = ("GIM_DKM", "GIM_LOFTR", "GIM_GLUE", "SIFT")


class FrameBank(SlotBank):
    """The frames of a video by frame index: uint8 [S, H, W, 3] RGB and their class maps uint8 [S, Hs, Ws], uploaded and segmented
    ONCE per frame however many pairs name it (the reference segments on first use and caches on disk, video_preprocessor.py:309-340).
    LRU eviction over `capacity_frames` slots (gim_amd/bank.py); a pair that names an evicted frame raises before any launch.
    device=None keeps numpy arrays: the host path of `prepare_pair` / `label_pair_list` (frame_prep_np), which needs no device.
    module: a gim_amd.semseg SegmentationModule; `put` then segments the frame on the device at the long-side-`seg_size` resolution
    (semseg.segment_device).  Without one, `put` takes the class map (`seg=`), at any resolution, one resolution per bank."""

    def __init__(self, capacity_frames, device=None, module=None, seg_size=720):
        super().__init__(capacity_frames, "frame bank")
        if module is not None and device is None:
            raise ValueError("frame bank: segmenting needs a device")
        self.device = self.resolve_device(device) if device is not None else None
        self.module, self.seg_size = module, int(seg_size)
        self.frames = self.seg = None

    def _slab(self, shape):
        if self.device is None:
            return np.zeros(shape, dtype=np.uint8)
        import torch
        return torch.zeros(shape, dtype=torch.uint8, device=self.device)

    def put(self, idx, frame_u8, seg=None):
        """frame idx: uint8 [H, W, 3] RGB (array or tensor), uploaded once; seg: its uint8 [Hs, Ws] class map, or None: segmented here
        when the bank has a module, else every pixel counts as class 0.  Returns the slot."""
        frame = frame_u8 if not isinstance(frame_u8, np.ndarray) else np.ascontiguousarray(frame_u8)
        if tuple(frame.shape[2:]) != (3,) or len(frame.shape) != 3 or str(frame.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"frame bank: a frame is uint8 [H, W, 3], got {frame.dtype} {tuple(frame.shape)}")
        H, W = int(frame.shape[0]), int(frame.shape[1])
        if self.frames is None:
            self.frames = self._slab((self.capacity, H, W, 3))
        elif tuple(self.frames.shape[1:3]) != (H, W):
            raise ValueError(f"frame bank: holds {tuple(self.frames.shape[1:3])} frames, got {(H, W)}")
        if self.device is None:
            frame_d = np.asarray(frame)
            seg_d = None if seg is None else np.ascontiguousarray(seg, dtype=np.uint8)
        else:
            import torch
            frame_d = (frame if isinstance(frame, torch.Tensor) else torch.from_numpy(frame)).to(self.device)
            if seg is not None:
                seg_d = (seg if isinstance(seg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(seg, dtype=np.uint8))).to(self.device)
            elif self.module is not None:
                from . import semseg
                with torch.cuda.device(self.device):
                    seg_d = semseg.segment_device(frame_d, self.seg_size, self.module)[0]
            else:
                seg_d = None
        if seg_d is None:
            seg_d = self._slab((1, 1))
        if len(seg_d.shape) != 2 or str(seg_d.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"frame bank: a class map is uint8 [Hs, Ws], got {seg_d.dtype} {tuple(seg_d.shape)}")
        if self.seg is None:
            self.seg = self._slab((self.capacity,) + tuple(seg_d.shape))
        elif tuple(self.seg.shape[1:]) != tuple(seg_d.shape):
            raise ValueError(f"frame bank: holds {tuple(self.seg.shape[1:])} class maps, got {tuple(seg_d.shape)}")
        slot = self.reserve([int(idx)])[0]
        self.frames[slot] = frame_d
        self.seg[slot] = seg_d
        return slot


def pair_boxes(pts, frame_hw, resize_hw, df=8):
    """video_preprocessor.py:296-303 / :321-328 for both sides of a cached label pts [n, 4]: per side the crop box (floor / ceil of
    the label's extent), its size (w, h) and the target (w_new, h_new) = get_divisible_wh(get_resized_wh(w, h, resize_hw), df)
    -> [(box (x0, y0, x1, y1), (w, h), (w_new, h_new))] * 2.  A box that is empty or leaves the frame raises ValueError."""
    import math
    from .frame_prep import get_divisible_wh, get_resized_wh
    pts = np.asarray(pts).reshape(-1, 4)
    if len(pts) == 0:
        raise ValueError("pair_boxes: an empty label has no extent")
    out = []
    for c in (0, 2):
        x0, x1 = math.floor(pts[:, c].min()), math.ceil(pts[:, c].max())
        y0, y1 = math.floor(pts[:, c + 1].min()), math.ceil(pts[:, c + 1].max())
        if not (0 <= x0 < x1 <= frame_hw[1] and 0 <= y0 < y1 <= frame_hw[0]):
            raise ValueError(f"pair_boxes: the label's extent {(x0, y0, x1, y1)} is empty or leaves the {frame_hw[1]} x {frame_hw[0]} frame")
        w, h = x1 - x0, y1 - y0
        w_new, h_new = get_divisible_wh(*get_resized_wh(w, h, list(resize_hw)), df)
        out.append(((x0, y0, x1, y1), (w, h), (w_new, h_new)))
    return out


def _method_flags(method):
    from . import frame_prep as fp
    if method not in METHODS:
        raise ValueError(f"method={method!r}: one of {METHODS}")
    return {"GIM_DKM": fp.OUT_RGB | fp.MASKED, "GIM_LOFTR": fp.OUT_RGB | fp.OUT_GRAY | fp.OUT_MASK8,
            "GIM_GLUE": fp.OUT_GRAY | fp.MASKED, "SIFT": fp.OUT_U8 | fp.OUT_MASK}[method]


def method_inputs(method, side0, side1, as_tensor):
    """the dict the reference builds for `method` (video_preprocessor.py:406-493) from the two sides' frame_prep outputs
    ({name: array or tensor}); as_tensor: array -> the caller's tensor type (identity on the device path)"""
    t = as_tensor
    if method == "GIM_DKM":
        return {"image0": t(side0["rgb"])[None], "image1": t(side1["rgb"])[None]}
    if method == "GIM_LOFTR":
        return {"image0": t(side0["gray"])[None], "image1": t(side1["gray"])[None], "color0": t(side0["rgb"])[None],
                "color1": t(side1["rgb"])[None], "mask0": t(side0["mask8"])[None], "mask1": t(side1["mask8"])[None]}
    if method == "GIM_GLUE":
        import torch
        g0, g1 = t(side0["gray"])[None], t(side1["gray"])[None]
        return {"gray0": g0, "gray1": g1, "size0": torch.tensor([[g0.shape[-1], g0.shape[-2]]]), "size1": torch.tensor([[g1.shape[-1], g1.shape[-2]]])}
    return {"rgb0": side0["u8"], "rgb1": side1["u8"], "mask0": side0["mask"], "mask1": side1["mask"]}


def prepare_pair(bank, idx0, idx1, method, exclude, resize=None):
    """The matcher's inputs of the frame pair (idx0, idx1) of `bank` -> (inputs, affine, kept).
    method: "GIM_DKM" (image0 / image1 fp32 [1,3,h,w], masked), "GIM_LOFTR" (image0 / image1 grey [1,1,h,w], color0 / color1
    [1,3,h,w], both unmasked, mask0 / mask1 uint8 [1,h/8,w/8]), "GIM_GLUE" (gray0 / gray1 [1,1,h,w] masked, size0 / size1 [1,2] (w, h))
    or "SIFT" (rgb0 / rgb1 uint8 [h,w,3], mask0 / mask1 uint8 [h,w], for a host detector).  exclude: the excluded class ids or a
    256-byte table.  resize=None: the first pass, whole frames at their own size, affine None.  resize=(pts, (h, w)): the second pass
    -- pts [n,4] the pair's cached label, both frames cropped to its extent and resized into the (h, w) box (`pair_boxes`), affine =
    (wA / wA_new, hA / hA_new, xA0, yA0, wB / wB_new, hB / hB_new, xB0, yB0) as label_pair(affine=) takes it (line 549).
    kept: the mask sums of both sides -- int32 [2] on the bank's device (one launch serves both sides), a numpy array on the host path.
    A frame that is not resident raises GimHipError before any launch."""
    from . import frame_prep as fp
    flags = _method_flags(method)
    s0, s1 = bank.slots([int(idx0), int(idx1)])
    H, W = (int(v) for v in bank.frames.shape[1:3])
    if resize is None:
        jobs, affine = [(s0, None, (W, H), flags), (s1, None, (W, H), flags)], None
    else:
        pts, box_hw = resize
        (b0, (w0, h0), n0), (b1, (w1, h1), n1) = pair_boxes(pts, (H, W), box_hw)
        jobs = [(s0, b0, n0, flags), (s1, b1, n1, flags)]
        affine = (w0 / n0[0], h0 / n0[1], b0[0], b0[1], w1 / n1[0], h1 / n1[1], b1[0], b1[1])
    if bank.device is None:
        import torch
        sides = [fp.frame_prep_np(bank.frames[s], bank.seg[s], exclude, box, size, fl) for s, box, size, fl in jobs]
        kept = np.array([sides[0]["kept"], sides[1]["kept"]], dtype=np.int32)
        return method_inputs(method, sides[0], sides[1], torch.from_numpy), affine, kept
    import torch
    from . import ops
    with torch.cuda.device(bank.device):
        r = ops.frame_prep(bank.frames, bank.seg, exclude, jobs)
    sides = [{name: r.get(j, name) for name in r.plan.views[j]} for j in (0, 1)]
    return method_inputs(method, sides[0], sides[1], lambda a: a), affine, r.kept


def label_pair_host(matcher_out, *, affine=None, vratio=1.0, threshold=0.5, confidence=0.999999, max_iters=100000, seed=0, refine=0,
                    score="count"):
    """`label_pair` on the host, the CPU oracle of its control flow: label_pack_np for both packs, pose.find_fundamental_mat with the
    host solver and sampler -> label fp32 [n,4] as a numpy array.  score="magsac" has no default_rng walk: it runs
    solve="ge", sampler="philox", the all-CPU restatement of label_pair's device run."""
    from . import pose
    k0, k1 = (np.asarray(t.detach().cpu() if hasattr(t, "detach") else t, dtype=np.float32).reshape(-1, 2) for t in _keypoints(matcher_out))
    moved = label_pack_np(k0, k1, moved_thr=1.0)
    empty = np.zeros((0, 4), dtype=np.float32)
    if len(moved) < 7:
        return empty
    pts = moved.astype(np.float64)
    how = dict(solve="ge", sampler="philox", score=score) if score != "count" else {}
    F, mask = pose.find_fundamental_mat(pts[:, :2], pts[:, 2:], threshold=threshold, prob=confidence, max_iters=max_iters, seed=seed, refine=refine,
                                        **how)
    if F is None or not mask.any():
        return empty
    return label_pack_np(moved[:, :2], moved[:, 2:], keep=mask, affine=affine, vratio=vratio)


def label_pair_list(match, bank, ids, method, out_dir, *, vratio, exclude, resize_cache=None, resize_hw=(900, 1600), refine=0, seed=0,
                    score="count", **ransac):
    """The labelling loop of video_preprocessor.py:255-566 without decoding: for every (idx0, idx1) of `ids`, in order,
        prepare_pair -> match(inputs) -> label_pair -> out_dir/str(np.array([idx0, idx1])) + '.npy', nums.npy, idxs.npy
    in the reference's layout (`LabelStore.from_dirs` reads it back).  match(inputs) returns a matcher's result dict (mkpts0_f /
    mkpts1_f) or a (k0, k1) pair, or None for a pair it cannot match (fewer than 8 descriptors on a side, :371 / :378; no matches,
    :501).  resize_cache=None is the first pass; a directory is the second (opt.resize): every pair is cropped to the extent of its
    label in that directory and resized into the resize_hw = (h, w) box.  Skipped, as the reference skips them: a pair whose file
    exists, a second-pass pair without a cached label (:287), kept == 0 on either side (:367), a match of None, no inliers (:522).
    Host reads per pair: `kept` (8 bytes) and what label_pair reads.  With a host bank (FrameBank(device=None)) everything runs in
    numpy (`label_pair_host`).  score: that of label_pair.  ransac: threshold / confidence / max_iters of label_pair.
    -> {"written": [(idx0, idx1)], "skipped": {(idx0, idx1): reason}}"""
    os.makedirs(out_dir, exist_ok=True)
    nums_path, idxs_path = os.path.join(out_dir, "nums.npy"), os.path.join(out_dir, "idxs.npy")
    nums = np.load(nums_path) if os.path.exists(nums_path) else np.array([])
    idxs = np.load(idxs_path) if os.path.exists(idxs_path) else np.array([])
    written, skipped = [], {}
    for idx0, idx1 in ids:
        idx0, idx1 = int(idx0), int(idx1)
        current = np.array([idx0, idx1])
        name = "{}.npy".format(str(current))
        path = os.path.join(out_dir, name)
        if os.path.exists(path):
            skipped[(idx0, idx1)] = "exists"
            continue
        resize = None
        if resize_cache is not None:
            cache = os.path.join(resize_cache, name)
            if not os.path.exists(cache):
                skipped[(idx0, idx1)] = "no cached label"
                continue
            resize = (np.load(cache), resize_hw)
        inputs, affine, kept = prepare_pair(bank, idx0, idx1, method, exclude, resize)
        k = kept.tolist()                                          # the pair's one host read before the matcher
        if k[0] == 0 or k[1] == 0:
            skipped[(idx0, idx1)] = "kept == 0"
            continue
        out = match(inputs)
        if out is None:
            skipped[(idx0, idx1)] = "no match"
            continue
        if bank.device is None:
            pts = label_pair_host(out, affine=affine, vratio=vratio, seed=seed, refine=refine, score=score, **ransac)
        else:
            pts = label_pair(out, device=bank.device, affine=affine, vratio=vratio, seed=seed, refine=refine, score=score, **ransac).cpu().numpy()
        if len(pts) == 0:
            skipped[(idx0, idx1)] = "no inliers"
            continue
        pts = pts.astype(np.float32)
        nums = np.concatenate([nums, np.array([len(pts)])], axis=0) if len(nums) else np.array([len(pts)])
        idxs = np.concatenate([idxs, current[None]], axis=0) if len(idxs) else current[None]
        np.save(path, pts)
        np.save(nums_path, nums)
        np.save(idxs_path, idxs)
        written.append((idx0, idx1))
    return {"written": written, "skipped": skipped}


# ---- thin adapters: match(inputs) over the existing modules ------------------------------------------------------------------------------
def loftr_match(model):
    """match(inputs) for "GIM_LOFTR" over a gim_amd.loftr.LoFTR module (video_preprocessor.py:460-472)"""
    def match(inputs):
        data = dict(inputs)
        model(data)
        return {"mkpts0_f": data["mkpts0_f"], "mkpts1_f": data["mkpts1_f"]}
    return match


def dense_match(model, num=5000):
    """match(inputs) for "GIM_DKM" over a gim_amd.dkm.DKMv3 / gim_amd.roma.RoMa module: match, sample `num`, pixels (:424-436)"""
    def match(inputs):
        from . import ops
        img0, img1 = inputs["image0"], inputs["image1"]
        dense, certainty = model.match(img0, img1)
        sparse, _ = model.sample(dense, certainty, num)
        k0, k1 = ops.dense_to_pixels(sparse, img0.shape[-2:], img1.shape[-2:])
        return {"mkpts0_f": k0, "mkpts1_f": k1}
    return match


def glue_match(detector, model):
    """match(inputs) for "GIM_GLUE" over gim_amd.lightglue's SuperPoint and LightGlue modules (:486-511); None without a match"""
    def match(inputs):
        import torch
        from .lightglue.pipeline import gim_lightglue_inference
        one = torch.ones(1, 2)
        data = {"image0": inputs["gray0"], "image1": inputs["gray1"], "scale0": one, "scale1": one,
                "image_size0": inputs["size0"], "image_size1": inputs["size1"]}
        gim_lightglue_inference(detector, model, data)
        if data["mkpts0_f"].shape[0] == 0:
            return None
        return {"mkpts0_f": data["mkpts0_f"], "mkpts1_f": data["mkpts1_f"]}
    return match


def sift_match(device="cuda", ratio=0.8):
    """match(inputs) for "SIFT": OpenCV's detector under the masks on the host (:370-381), nn_match.RootSiftMatcher on the device.
    Raises GimHipError where cv2 does not import (the detector is not restated); None with fewer than 8 descriptors on a side."""
    from .nn_match import RootSiftMatcher, _cv2
    cv2 = _cv2()
    matcher = RootSiftMatcher(ratio=ratio, device=device)

    def match(inputs):
        import torch
        sides = []
        for s in ("0", "1"):
            rgb, mask = (np.ascontiguousarray(inputs[k + s].cpu().numpy() if hasattr(inputs[k + s], "cpu") else inputs[k + s]) for k in ("rgb", "mask"))
            sift = cv2.SIFT_create(nfeatures=rgb.shape[0] * rgb.shape[1] // 64, contrastThreshold=1e-5)
            kpts, desc = sift.detectAndCompute(cv2.cvtColor(rgb, cv2.COLOR_RGB2BGR), mask)
            if desc is None or desc.shape[0] < 8:
                return None
            kpts = np.array([[kp.pt[0], kp.pt[1]] for kp in kpts], dtype=np.float32).reshape(-1, 2)
            sides += [torch.from_numpy(kpts).to(device), torch.from_numpy(np.ascontiguousarray(desc, dtype=np.float32)).to(device)]
        return matcher.match_descriptors(*sides)
    return match
