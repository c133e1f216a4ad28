"""The fine FPN head of gim_loftr (resnet.py:321-329), from the trunk's (x1, x2, x3_out) to the fine map at 1/2 resolution: dense, or (forward())
with its last `depth` stages left for after coarse matching, on the 8 x 32 patches the matches' fine windows can read:
  0  the dense head;
  1  layer1_outconv2's two 3 x 3 layers (1/2 level) wait for the matches     (`_fine_sparse_ok`);
  2  ... and the 1/2-level lateral conv + upsample-add in front of them       (`_lateral_sparse_ok`);
  3  ... and the three 1/4-level launches in front of that lateral            (`_quarter_sparse_ok`).
`FineHead` is a mixin of `LoFTR`: its methods launch through `self._conv`, read the switches and fork through `self._fork_join`."""
import functools
from typing import NamedTuple, Optional

import torch

from .. import ops
from .._lib import ACT_LEAKY, ACT_NONE
from ..packing import is_half


def _half(v):
    """output extent of a stride-2 convolution with pad = k // 2 (k7 p3, k3 p1) over an extent of v"""
    return (v - 1) // 2 + 1


class HeadInputs(NamedTuple):
    """what the stages left to `_fine_tail_sparse` read, None for the rest: depth 3: x1, x2, x3_out; depth 2: x1, x2_out; depth 1: x1_out"""
    x1: Optional[torch.Tensor] = None
    x2: Optional[torch.Tensor] = None
    x3_out: Optional[torch.Tensor] = None
    x2_out: Optional[torch.Tensor] = None
    x1_out: Optional[torch.Tensor] = None

    @property
    def depth(self):
        return 1 if self.x1_out is not None else 2 if self.x2_out is not None else 3


def _cached_per_key(check):
    """a predicate (self, P, xs) -> bool, computed once per `_head_key`: the answers live in `self._head_ok`, which `_invalidate()` empties"""
    @functools.wraps(check)
    def ok(self, P, xs):
        key = (check.__name__,) + self._head_key(P, xs)
        if key not in self._head_ok:
            self._head_ok[key] = bool(check(self, P, xs))
        return self._head_ok[key]
    return ok


class FineHead:
    def _fpn_fine(self, P, x1, x2, x3_out, head=0):
        """the FPN's top-down path to the 1/2 resolution (resnet.py:321-329): six convolutions that nothing of the coarse level (position
        encoding, transformer, coarse matching) depends on.  Returns the fine map; head = 1..3: stops in front of the last `head` stages and
        returns their `HeadInputs` (forward's sparse head, _fine_tail_sparse)."""
        if head == 3:
            return HeadInputs(x1=x1, x2=x2, x3_out=x3_out)
        # lateral 1x1 conv + F.interpolate(scale_factor=2, bilinear, align_corners=True) of the coarser level + add (resnet.py:
        # 321-327): the upsample-add runs in the conv's epilogue when the launch takes it, else as a second pass over the output
        x2_out = self._conv(x2, P["l2o"], ups=x3_out)
        x2_out = self._conv(self._conv(x2_out, P["l2o2a"], ACT_LEAKY), P["l2o2b"])
        if head == 2:
            return HeadInputs(x1=x1, x2_out=x2_out)
        x1_out = self._conv(x1, P["l1o"], ups=x2_out)
        return HeadInputs(x1_out=x1_out) if head == 1 else self._fpn_fine_tail(P, x1_out)

    def _fine_halo(self, P, h2, w2):
        """do the fine head's last two layers run on the 3x3 halo kernel at this 1/2-resolution size?  With `fine_sparse` on, every path of the
        module (forward, extract, debug) sends them there wherever the map is whole 8 x 32 patches, whether the launch then walks a patch list
        or all patches: one kernel, one K order, so forward() and extract() + match_features() stay bit-identical."""
        return bool(self.fine_sparse and is_half(self._dt()) and self.use_lds_dma and ops.HALO and P["l1o2a"].halo is not None
                    and P["l1o2b"].halo is not None and h2 % 8 == 0 and w2 % 32 == 0)

    def _fpn_fine_tail(self, P, x1_out, tiles=None, n_tiles=None, out=None):
        """layer1_outconv2 (resnet.py:329): the two 3x3 layers at 1/2 resolution whose output is the fine map.  tiles / n_tiles
        (ops.fine_tile_lists): only those 8 x 32 patches are computed (see _fine_tail_sparse); out = (mid, f): the two layers' output maps
        (the pair-range chains of _fine_tail_sparse share them)."""
        B, H, W, _ = x1_out.shape
        if self._fine_halo(P, H, W):
            # (no health word: these launches add no residual -- ops.conv_rows hands the word to residual / split launches only)
            mid, f = out if out is not None else self._fine_head_maps(P, HeadInputs(x1_out=x1_out))
            ops.conv3x3_halo(x1_out, P["l1o2a"], mid, ACT_LEAKY, tiles=tiles, n_tiles=n_tiles)
            ops.conv3x3_halo(mid, P["l1o2b"], f, ACT_NONE, tiles=tiles, n_tiles=n_tiles)
            return f
        assert tiles is None and out is None
        return self._conv(self._conv(x1_out, P["l1o2a"], ACT_LEAKY), P["l1o2b"])

    def _fine_head_maps(self, P, head):
        """the (uncleared) maps the sparse head writes between `head` and the fused fine kernel, in launch order.  depth 3, six: layer2_outconv +
        upsample-add, layer2_outconv2's two layers, the lateral sum x1_out, layer1_outconv2's two layers; depth 2: the last three; 1: two."""
        new = lambda t, name: torch.empty(*t.shape[:3], P[name].n_store, dtype=t.dtype, device=t.device)   # noqa: E731
        front = ((head.x2, "l2o"), (head.x2, "l2o2a"), (head.x2, "l2o2b"), (head.x1, "l1o"))[(4, 3, 0)[head.depth - 1]:]
        maps = tuple(new(t, name) for t, name in front)
        x1_out = maps[-1] if maps else head.x1_out
        return maps + (new(x1_out, "l1o2a"), new(x1_out, "l1o2b"))

    # ---- how deep may this forward's sparse head go? ---------------------------------------------------------------------------------
    def _head_key(self, P, xs):
        """everything the three predicates below read (the key of their cache): the inputs' count and shape, the switches of the module and of gim_amd.ops, and each head
        pack's type, widths and halo packing (kernel size, stride and padding are the architecture's; new weights go through `_invalidate()`)"""
        packs = tuple((pk.dtype, pk.cin_pad, pk.n_store, pk.halo is not None)
                      for pk in (P[n] for n in ("l2o", "l2o2a", "l2o2b", "l1o", "l1o2a", "l1o2b")))
        return (len(xs), tuple(xs[0].shape[:3]), self.debug is None, self._dt(), bool(self.use_lds_dma), bool(self.fine_sparse),
                bool(self.lateral_sparse), bool(self.quarter_sparse), ops.HALO, ops.HALO_MIN_TILES, ops.FORCE_BIG_TILE, ops.UPS_FUSED, packs)

    def _head_depth(self, P, xs):
        """the number of head stages this forward leaves for after coarse matching (module docstring): each level only on top of the one before"""
        checks = (self._fine_sparse_ok, self._lateral_sparse_ok, self._quarter_sparse_ok)
        return next((d for d, ok in enumerate(checks) if not ok(P, xs)), 3)

    @_cached_per_key
    def _fine_sparse_ok(self, P, xs):
        """may this forward compute the fine map under the matched windows only?  (the conditions of _fine_tail_sparse)"""
        if self.debug is not None or len(xs) != 1:   # debug dumps and the extract() handles hold complete maps
            return False
        B, H, W = xs[0].shape[:3]
        h2, w2 = _half(H), _half(W)
        h8, w8 = _half(_half(h2)), _half(_half(w2))
        # the window stride the gather uses (4 h8 = h2), and no more patches than the one-workgroup list kernel flags
        return self._fine_halo(P, h2, w2) and h2 == 4 * h8 and w2 == 4 * w8 and B * (h2 // 8) * (w2 // 32) <= ops.FINE_TILE_MAX_FLAGS

    @_cached_per_key
    def _lateral_sparse_ok(self, P, xs):
        """may this forward (one that `_fine_sparse_ok` accepts) also compute the lateral sum x1_out under the matched windows only?  The
        launch must be one the patch-list entry takes, and one whose dense form fuses the upsample-add as well -- extract() runs that one,
        and forward() must stay bit-identical to extract() + match_features() (ops.conv_ups_tiles_supported); x1 is [B,h2,w2,.], x2_out
        [B,h2/2,w2/2,.]."""
        if not self.lateral_sparse:
            return False
        B, H, W = xs[0].shape[:3]
        pk = P["l1o"]
        h2, w2 = _half(H), _half(W)
        return ops.conv_ups_tiles_supported((B, h2, w2, pk.cin_pad), pk, (B, h2 // 2, w2 // 2, pk.n_store), dense_too=True)

    @_cached_per_key
    def _quarter_sparse_ok(self, P, xs):
        """may this forward (one that `_lateral_sparse_ok` accepts) also compute the 1/4-level part of the head -- layer2_outconv + upsample-add
        of x3_out, then the two 3 x 3 layers of layer2_outconv2 -- on patch lists behind coarse matching?  Each of the three launches must be one
        its list entry takes AND one whose dense form runs on the same 256 x 256 tile in the same K order: extract() and every fall-back run
        the dense launches, and forward() must stay bit-identical to extract() + match_features().  x2 is [B,h4,w4,.], x3_out [B,h8,w8,.]."""
        if not (self.quarter_sparse and self._lateral_sparse_ok(P, xs)):
            return False
        B, H, W = xs[0].shape[:3]
        h2, w2 = _half(H), _half(W)
        h4, w4 = _half(h2), _half(w2)
        pk, pa, pb = P["l2o"], P["l2o2a"], P["l2o2b"]
        return (h2 == 2 * h4 and w2 == 2 * w4 and h4 % 2 == 0 and w4 % 2 == 0 and ops.fine_tile_lists4_fits(B // 2, h2, w2)
                and pa.cin_pad == pk.n_store and pb.cin_pad == pa.n_store
                and ops.conv_ups_tiles_supported((B, h4, w4, pk.cin_pad), pk, (B, h4 // 2, w4 // 2, pk.n_store), dense_too=True)
                and ops.conv_tiles_supported((B, h4, w4, pa.cin_pad), pa, dense_too=True)
                and ops.conv_tiles_supported((B, h4, w4, pb.cin_pad), pb, dense_too=True))

    # ---- the stages left for after coarse matching -------------------------------------------------------------------------------------
    def _fine_tail_sparse(self, P, head, cr, bs):
        """The last `head.depth` stages of the head on the 8 x 32 patches that the fine level can read, behind coarse matching and in the same
        captured graph.  The fine map has ONE consumer: the gather of a 5 x 5 window per match and side at rows 4 cy - 2 .. 4 cy + 2
        (fine_fused.hip / gim_fine_gather; zeros outside the image).  One one-workgroup launch (ops.fine_tile_lists) builds the patch lists of
        the depth from the device-side match count (no host sync); the launches then walk them.  Pixels of other patches are never written and never read:
        the maps are NOT cleared (a replayed graph leaves the previous forward's values there).

        depth 1 (gim_fine_tile_list).  A window pixel of layer1_outconv2's second layer reads the first layer at +-1 more, so both launches
        walk one list: the patches that hold a pixel of [4 cy - 3, 4 cy + 3] x [4 cx - 3, 4 cx + 3] for some match.  Every input of a listed
        first-layer pixel lies in x1_out, which is dense.

        depth 2 (gim_fine_tile_lists).  Two lists from one launch: the +-3 list for the two 3 x 3 layers, and the patches of the reach one
        pixel wider, +-4, for the lateral -- every x1_out pixel a CONSUMED first-layer output (+-3) reads lies within +-4, hence in a patch
        of the second list.  A listed first-layer patch also reads a one-pixel ring that may lie in patches the lateral never wrote (stale
        or uninitialised values): those reach only first-layer outputs outside every +-3 box, which the second layer's consumed outputs
        (+-2) never read -- convolution outputs do not mix across pixels.  The alternative, ONE +-4 list for all three launches, rests on
        the same argument but grew the two 3 x 3 launches (the expensive ones: a patch row is added below every match on an odd coarse
        row, 4 cy + 4 = 8 k) and shrank nothing, and measured slower.

        depth 3 (gim_fine_tile_lists4).  x2_out has ONE consumer, the list-walking lateral, which reads it where Epilogue::ups_accumulate
        stages upsample sources for the +-4 patches: S, weight-0 sources included (0 x NaN = NaN, and an unlisted pixel may hold anything).
        x2_out is valid on S if layer2_outconv2's first layer is valid on S dilated by 1, and that if the 1/4-level lateral is valid on S
        dilated by 2: lists C, B, A (C <= B <= A), from the same launch.  The ring a listed patch reads outside its list reaches only
        outputs outside S and its dilations, which nothing consumed reads.

        `fine_chains` > 1 (depth 3): K pair-range chains on parallel streams.  Chain g owns the pairs [bs g / K, bs (g + 1) / K), i.e. the
        images b and bs + b of those pairs: its list launch marks the patches of its own matches only (b_range), then its six launches
        walk those lists.  No launch reads across images, so the chains write disjoint patches of the same six maps, with the bits the
        one-chain launches write.  The launches are persistent: alone on the chip each pays a whole last round, two chains fill each
        other's.  Fork behind coarse matching, join in front of the fused fine kernel; same kernels, same arithmetic."""
        depth = head.depth
        H, W = (head.x1_out if depth == 1 else head.x1).shape[1:3]
        K = min(int(self.fine_chains), bs) if (depth == 3 and self.debug is None and self.fine_chains > 1 and self._fine_halo(P, H, W)) else 1
        # allocated on the main stream in front of the fork, read by the main stream behind the join
        maps = self._fine_head_maps(P, head)

        def chain(g):
            pairs = {"b_range": (bs * g // K, bs * (g + 1) // K)} if K > 1 else {}
            lists = ops.fine_tile_lists(cr.b_ids, cr.i_ids, cr.j_ids, cr.count, bs, cr.args.w0c, cr.args.w1c, 4, H, W, depth=depth, **pairs)
            # (first depth that runs it, launch): t is what the launch in front returned, y the map to write
            table = ((3, lambda t, y: ops.conv2d_ups_tiles(head.x2, P["l2o"], head.x3_out, lists.tilesq[0], lists.n_tilesq[0:1], y=y)),
                     (3, lambda t, y: ops.conv2d_tiles(t, P["l2o2a"], lists.tilesq[1], lists.n_tilesq[1:2], ACT_LEAKY, out=y)),
                     (3, lambda t, y: ops.conv2d_tiles(t, P["l2o2b"], lists.tilesq[2], lists.n_tilesq[2:3], out=y)),
                     (2, lambda t, y: ops.conv2d_ups_tiles(head.x1, P["l1o"], t, lists.tiles4, lists.n_tiles4, y=y)))
            t = head.x2_out if depth == 2 else head.x1_out
            for (_, launch), y in zip([row for row in table if depth >= row[0]], maps):
                t = launch(t, y)
                if K > 1 and t is not y:   # a dense fall-back allocates its own map: _quarter_sparse_ok admitted all four
                    raise RuntimeError("fine_chains: a list launch of the sparse fine head fell back to its dense form")
            self._fpn_fine_tail(P, t, lists.tiles, lists.n_tiles, out=maps[-2:])
            return lists

        # the chains' patch lists and counts stay referenced until the join (the caching allocator re-uses a freed block per stream)
        keep = self._fork_join(cr.b_ids.device, K, chain)   # noqa: F841
        return maps[-1]   # (`keep` dies past the join: see the lifetime note at T.init_state, _transformer_emit)
