"""Video pseudo-labels: the labeller's tail, `link` and `propagate` (the reference's video_preprocessor.py:513-566 and
datasets/walk/walk.py:29,170-266), on the host in numpy or on a device through csrc/label_link.hip.

A label is an fp32 [n,4] array of matches (x0, y0, x1, y1) of a frame pair in the pixels of the frames the labels were written in.
`link` joins the labels of a->b and b->c into a->c through the rounded pixels they share in b; `propagate` is the reference's
recursion of such hops over the label sets of several frame skips; `label_pair` turns one matcher output into a label.

`link` restates the reference's dicts and sets as two tables over the key range (`link_tables`; ops.label_link on the device), with
one documented difference: rows whose key is not finite or lies outside [0, width * (height + 1)] are ignored and counted where the
reference would still join them.  Everything else -- which rows join, their partners, their order, the copied bits -- is the
reference's (tests/label_link_oracle.py holds the dict / set formulation the tests compare against).

Not here: video decoding and frame selection, the pair-id selection of walk.py:115-128, the debug figure, MAGSAC scoring
(`label_pair` runs plain RANSAC), and a lockstep `propagate` over many pairs (ops.label_link takes B links per call for it).
"""
import collections
import os

import numpy as np

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
               refine=0):
    """The tail of a labelling step (video_preprocessor.py:513-555) for one frame pair -> label fp32 [n,4] on the device.
    matcher_out: a matcher's result dict (`mkpts0_f` / `mkpts1_f`, matched keypoints [n,2] in pixels) or a (k0, k1) pair.
      1. ops.label_pack with moved_thr = 1 drops static matches (watermarks, line 516);
      2. pose.find_fundamental_mat(solve="device", sampler="device") on the survivors: PLAIN RANSAC with the Sampson distance where
         the reference calls cv2.findFundamentalMat(USAC_MAGSAC, 0.5, 0.999999, 100000) -- MAGSAC's scoring is not restated;
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
                                            device=device, solve="device", sampler="device", refine=refine)
        if F is None or not mask.any():
            return empty
        m0, m1 = moved[:, :2].contiguous(), moved[:, 2:].contiguous()
        keep = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(device)
        out, count = ops.label_pack(m0, m1, keep=keep, affine=affine, vratio=vratio)
        return out[:int(count.item())]
