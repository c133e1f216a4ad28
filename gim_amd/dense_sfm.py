"""Dense SfM over a pair list: the dense matches of every pair stay on the device and are aggregated there into one keypoint set per
image and keypoint-indexed one-to-one matches -- hloc's `keypoints` / `matches0` / `matching_scores0` datasets with one read-back per
scene for the keypoints and one per batch of pairs for the matches.

What the reference does on the host, one match at a time (hloc/match_dense.py: `match_and_assign`, :422-):
    match_dense          :204-258   per pair: model, rescale to the original image, write keypoints0/1 + scores
    aggregate_matches    :298-390   per pair: read back, bin through dictionaries (`assign_keypoints(update=True)`), per image the
                                    best bin per cell and the max_kps best cells
    assign_matches       :393-419   per pair: KDTree of the final keypoints, nearest within max_error, one-to-one
is here `DenseMatchAggregator` on csrc/dense_agg.hip (gim_agg_vote / gim_agg_finalize / gim_agg_keypoints / gim_agg_assign);
`gim_amd.hloc_formats` keeps the host restatement, which the tests use as the oracle.

Differences from the reference, none of which a COLMAP import sees:
  * keypoint ids are a permutation of the reference's (first-appearance order there).  Here: without max_kps the raster order of the
    voted cells; with max_kps the first max_kps cells in (score descending, raster cell index) order.  `cells(name)` maps ids to cells.
  * score sums are exact 64-bit fixed point (2^-32) instead of fp32 in arrival order, so they do not depend on the order of the pairs.
  * ties: the lowest bin index of a cell, the lowest keypoint id at equal distance, the lowest match index at equal score.
Out of scope: the localisation branch (query keypoints not binned), pre-existing reference features, the
`existing_refs` flip and the RAM-saving pair reordering.
"""
import numpy as np
import torch

from . import hloc_formats, ops
from ._lib import GimHipError
from .bank import pair_batches


class DenseMatchAggregator:
    """One scene: `add_image` every image, `add_pair` the matches of every pair (device tensors; they are stored and vote at once),
    `finalize` the keypoints, `assign` / `write` the keypoint-indexed matches."""

    def __init__(self, max_error=2, cell_size=8, device="cuda", capacity_matches=1 << 16):
        self.max_error, self.cell_size = max_error, cell_size
        self.patch = ops.agg_patch(max_error, cell_size)          # refuses patch / vote outside 1..8 and max_error > patch / 2
        self.bins = ops.agg_bins(max_error, self.patch)
        self.device = torch.device(device)
        self.slots = {}                                           # image name -> slot, in order of arrival; nothing is ever evicted
        self.sizes = []                                           # per slot (W, H)
        self.cell_off = [0]                                       # per slot its first cell in the flat cell arrays
        self.pairs = []                                           # (name0, name1) in order of arrival
        self.pair_slots = []
        self.offsets = [0]                                        # pool rows of the pairs
        self._capacity = max(int(capacity_matches), 1)
        self._pool = None                                         # (kpts0 [cap,2], kpts1 [cap,2], scores [cap]) on the device
        self._grid = None                                         # (geom [S,4], votes [cells*bins], cell_n [cells]) for the first _grid_slots slots
        self._grid_slots = 0
        self._dropped = []
        self._kp = None
        self._final = None

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.slots)

    def __contains__(self, name):
        return name in self.slots

    def add_image(self, name, width, height):
        """a slot for the image (original size in pixels); naming a resident image again must repeat its size"""
        width, height = int(width), int(height)
        if self._kp is not None:
            raise GimHipError("DenseMatchAggregator: add_image after finalize")
        if width < 1 or height < 1:
            raise GimHipError(f"DenseMatchAggregator: image {name!r} of size {width} x {height}")
        if name in self.slots:
            if self.sizes[self.slots[name]] != (width, height):
                raise GimHipError(f"DenseMatchAggregator: image {name!r} is resident with size {self.sizes[self.slots[name]]}, not {(width, height)}")
            return self.slots[name]
        gw, gh = ops.agg_grid(width, height, self.patch)
        if self.cell_off[-1] + gw * gh > 0x7fffffff:
            raise GimHipError("DenseMatchAggregator: the cells of the scene do not fit int32 indices")
        slot = self.slots[name] = len(self.sizes)
        self.sizes.append((width, height))
        self.cell_off.append(self.cell_off[-1] + gw * gh)
        return slot

    def _reserve(self, n):
        """room for n more pool rows: the arrays double (one copy) when they are full"""
        need = self.offsets[-1] + n
        if need > 0x7fffffff:
            raise GimHipError("DenseMatchAggregator: the stored matches do not fit int32 rows")
        if self._pool is not None and need <= self._pool[2].shape[0]:
            return
        cap = self._capacity if self._pool is None else self._pool[2].shape[0]
        while cap < need:
            cap *= 2
        new = (torch.empty(cap, 2, dtype=torch.float32, device=self.device), torch.empty(cap, 2, dtype=torch.float32, device=self.device),
               torch.empty(cap, dtype=torch.float32, device=self.device))
        if self._pool is not None:
            used = self.offsets[-1]
            for dst, src in zip(new, self._pool):
                dst[:used].copy_(src[:used])
        self._pool = new

    def _state(self):
        """the flat cell arrays over all slots; images that arrived after the first vote get zeroed cells appended"""
        S = len(self.sizes)
        if S == 0:
            raise GimHipError("DenseMatchAggregator: no image")
        if self._grid is None or self._grid_slots != S:
            geom = torch.tensor([[w, h, self.cell_off[s], 0] for s, (w, h) in enumerate(self.sizes)], dtype=torch.int32).to(self.device)
            have = 0 if self._grid is None else self._grid[2].shape[0]
            more = self.cell_off[-1] - have
            votes = torch.zeros(more * self.bins, dtype=torch.int64, device=self.device)
            cell_n = torch.zeros(more, dtype=torch.int32, device=self.device)
            if self._grid is not None:
                votes, cell_n = torch.cat([self._grid[1], votes]), torch.cat([self._grid[2], cell_n])
            self._grid, self._grid_slots = (geom, votes, cell_n), S
        if self._pool is None:
            self._reserve(0)
        return ops.AggState(*self._pool, *self._grid, self.cell_off, self.max_error, self.patch)

    def _slot(self, name):
        if name not in self.slots:
            raise GimHipError(f"DenseMatchAggregator: image {name!r} is unknown: add_image it first")
        return self.slots[name]

    # ---- the three steps ----------------------------------------------------------------------------------------------------
    def add_pair(self, name0, name1, kpts0, kpts1, scores):
        """stores the pair's matches (device tensors: kpts0, kpts1 [n,2] pixel coordinates of the original images, scores [n]) and
        lets them vote; n == 0 is a pair like any other"""
        if self._kp is not None:
            raise GimHipError("DenseMatchAggregator: add_pair after finalize")
        s0, s1 = self._slot(name0), self._slot(name1)
        n = int(scores.shape[0])
        if kpts0.shape != (n, 2) or kpts1.shape != (n, 2) or scores.dim() != 1:
            raise GimHipError(f"DenseMatchAggregator: pair ({name0!r}, {name1!r}): kpts {tuple(kpts0.shape)} / {tuple(kpts1.shape)}, scores {tuple(scores.shape)}")
        self._reserve(n)
        lo = self.offsets[-1]
        for dst, src in zip(self._pool, (kpts0, kpts1, scores)):
            dst[lo:lo + n].copy_(src)                             # casts to fp32 where needed
        self.pairs.append((name0, name1))
        self.pair_slots.append((s0, s1))
        self.offsets.append(lo + n)
        st = self._state()
        batch = ops.agg_batch([lo, lo + n], [s0], [s1], len(self.sizes), st.scores.shape[0], self.device)
        self._dropped.append(ops.agg_vote(st, batch))

    def dropped(self):
        """per pair the matches that did not count (outside their image, or a score that is not finite and in [0, 65536)); a read-back"""
        return torch.cat(self._dropped).tolist() if self._dropped else []

    def finalize(self, max_kps=8192):
        """{name: (keypoints fp32 [K,2], score fp64 [K])} as host arrays, one read-back for the scene; `max_kps` None keeps every cell.
        May be repeated with another max_kps; pairs can no longer be added."""
        kp = ops.agg_finalize(self._state(), max_kps)
        k, sc, ce = kp.keypoints.cpu().numpy(), kp.score.cpu().numpy(), kp.cells.cpu().numpy()
        o = kp.host_kp_off
        self._kp = kp
        self._final = {name: (k[o[s]:o[s + 1]], sc[o[s]:o[s + 1]], ce[o[s]:o[s + 1]]) for name, s in self.slots.items()}
        return {name: v[:2] for name, v in self._final.items()}

    def cells(self, name):
        """int32 [K,2]: the cell (cx, cy) of every final keypoint of the image, in id order"""
        self._need_final()
        return self._final[name][2]

    def keypoints_device(self):
        """the ops.AggKeypoints of the last finalize (flat device arrays over all images)"""
        self._need_final()
        return self._kp

    def _need_final(self):
        if self._kp is None:
            raise GimHipError("DenseMatchAggregator: finalize first")

    def assign(self, batch_pairs=32):
        """yields (matches0 int32 [max id0 + 1], matching_scores0 fp16) per pair, in the order the pairs were added; `batch_pairs` pairs
        per launch sequence and read-back"""
        self._need_final()
        if batch_pairs < 1:
            raise GimHipError(f"DenseMatchAggregator: batch_pairs={batch_pairs}")
        st = self._state()
        b1 = 0
        for chunk in pair_batches(self.pair_slots, int(batch_pairs)):
            b0, b1 = b1, b1 + len(chunk)
            s0, s1 = zip(*chunk)
            batch = ops.agg_batch(self.offsets[b0:b1 + 1], s0, s1, len(self.sizes), st.scores.shape[0], self.device)
            r = ops.agg_assign(st, self._kp, batch)
            rows0, P = r.matches0.shape[0], b1 - b0
            host = torch.cat([r.matches0.view(torch.uint8), r.row_len.view(torch.uint8), r.scores_f16.view(torch.uint8)]).cpu().numpy()
            m0, ln = host[:4 * rows0].view(np.int32), host[4 * rows0:4 * (rows0 + P)].view(np.int32)
            s16 = host[4 * (rows0 + P):].view(np.float16)
            for p in range(P):
                a = int(r.koff0[p])
                yield m0[a:a + ln[p]].copy(), s16[a:a + ln[p]].copy()

    def write(self, feature_fd, match_fd, write_dense=True, batch_pairs=32):
        """hloc's files through gim_amd.hloc_formats: `keypoints` / `score` per image into feature_fd, per pair `matches0` /
        `matching_scores0` into match_fd[pair], behind `keypoints0` / `keypoints1` / `scores` (the stored dense matches) with write_dense"""
        self._need_final()
        for name, (k, sc, _) in self._final.items():
            hloc_formats.write_keypoints(feature_fd, name, k, sc)
        if write_dense:
            used = self.offsets[-1]
            k0, k1, sc = (t[:used].cpu().numpy() for t in self._state()[:3])
        for p, (m0, s0) in enumerate(self.assign(batch_pairs)):
            name0, name1 = self.pairs[p]
            key = hloc_formats.pair_key(name0, name1)
            if write_dense:
                lo, hi = self.offsets[p], self.offsets[p + 1]
                grp = hloc_formats.write_dense_pair(match_fd, name0, name1, k0[lo:hi], k1[lo:hi], sc[lo:hi])
            else:
                grp = match_fd[key] if key in match_fd else match_fd.create_group(key)
            hloc_formats.write_matches0(grp, m0, s0)


def _scale_of(scales, name):
    if scales is None or scales.get(name) is None:
        return np.array([1.0, 1.0])
    return np.asarray(scales[name], dtype=np.float64).reshape(2)


@torch.no_grad()
def match_dense_pair_list(matcher, images, pairs, aggregator, scales=None, bank=None, batch_pairs=1):
    """The loop of match_dense.py:221-257 with the matches kept on the device.  matcher: an `adapters.HlocDenseMatcher`, an hloc plugin
    or any callable with their dict contract ({'image0', 'image1', 'name0', 'name1'} -> {'keypoints0', 'keypoints1', 'scores'});
    images: {name: [1,C,H,W] device tensor}; pairs: [(name0, name1)]; scales: {name: (sx, sy)} = original size / matched size
    (ImagePairDataset.preprocess), default 1.  Every pair gets the rescale of :242-243, scale_keypoints(k + 0.5, s) - 0.5 in fp32 on
    the device, and goes to `aggregator.add_pair`; images the aggregator does not know are added with their original size.  Returns
    nothing: `aggregator.finalize` / `assign` / `write` follow.
    bank (a gim_amd.dense_bank.DenseFeatureBank of the matcher's net; the matcher then needs `bank_put` / `match_pairs`, as
    HlocDenseMatcher and the dense hloc plugins have them): every image is extracted on first use instead of once per pair, pairs go
    out `batch_pairs` at a time, the tail and the rescale are one launch per batch; `add_pair` gets the same rows in the same order."""
    for name0, name1 in pairs:
        for name in (name0, name1):
            if name not in images:
                raise GimHipError(f"match_dense_pair_list: pair ({name0!r}, {name1!r}) names an image that was not given")
            if name not in aggregator:
                s = _scale_of(scales, name)
                h, w = images[name].shape[-2:]
                aggregator.add_image(name, int(round(w * s[0])), int(round(h * s[1])))
    if bank is not None:
        bp = max(1, int(batch_pairs))
        for chunk in pair_batches(pairs, bp):
            names = list(dict.fromkeys(n for pr in chunk for n in pr))
            if len(names) > bank.capacity:
                raise GimHipError(f"match_dense_pair_list: a batch of {len(chunk)} pairs names {len(names)} images, the bank has {bank.capacity} slots")
            resident = [n for n in names if n in bank]
            if resident:
                bank.slots(resident)                     # most recently used: making room below does not evict them
            for n in names:
                if n not in bank:
                    matcher.bank_put(bank, n, images[n])
            sc = [(tuple(np.float32(_scale_of(scales, n0))), tuple(np.float32(_scale_of(scales, n1)))) for n0, n1 in chunk]
            for (n0, n1), pred in zip(chunk, matcher.match_pairs(bank, chunk, batch_pairs=bp, scales=sc)):
                aggregator.add_pair(n0, n1, pred["keypoints0"], pred["keypoints1"], pred["scores"])
        return
    for name0, name1 in pairs:
        pred = matcher({"image0": images[name0], "image1": images[name1], "name0": name0, "name1": name1})
        out = []
        for side, name in (("0", name0), ("1", name1)):
            k = pred["keypoints" + side] + 0.5
            s = _scale_of(scales, name)
            if np.any(s != 1.0):
                k = k * k.new_tensor(s)
            out.append(k - 0.5)
        aggregator.add_pair(name0, name1, out[0], out[1], pred["scores"])
