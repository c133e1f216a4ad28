"""Thin torch-tensor wrappers over the libgimhip C ABI (device pointers + current stream; torch is only
the allocator / stream owner).  Every function launches HIP kernels from `gim_amd/csrc`; none of them
has a torch or CPU fallback."""
import collections
import ctypes
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ACT_ELU1, ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_RELU, GIM_BF16, GIM_F16, GIM_F32, check, lib  # noqa: F401
from .packing import elem_size, torch_dtype
from .switches import flag

_DT = {torch.float32: GIM_F32, torch.bfloat16: GIM_BF16, torch.float16: GIM_F16}
HALF = (torch.bfloat16, torch.float16)   # the two 16-bit operand kinds: same kernels in two flavours (csrc/gim_common.h)


# bench.py's live roofline measurement.  When set to a list, every launch of that group is bracketed by HIP events recorded on the launch
# stream and (start, end, algorithmic_flops, label) is appended (_Timed): PROFILE -- the gim_conv2d_bn_act / gim_conv3x3_halo_tiles
# launches, label = the layer's shape; PROFILE_FUSED -- the fused kernels, label = the kernel family.
PROFILE = None
PROFILE_FUSED = None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Timed:
    """bench.py's live measurement: HIP events on the launch stream around one C-ABI call, appended as (start, end, algorithmic_flops,
    label) to PROFILE_FUSED -- or, `conv=True`, to PROFILE -- when that list is set.  `label` / `flops` may be callables: evaluated behind
    the launch, in measuring runs only (a label nobody else builds, a count that lives on the device)."""

    def __init__(self, label, flops, conv=False):
        self.label, self.flops, self.conv = label, flops, conv

    def __enter__(self):
        self.sink = PROFILE if self.conv else PROFILE_FUSED
        if self.sink is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.e1.record()
            flops, label = (v() if callable(v) else v for v in (self.flops, self.label))
            self.sink.append((self.e0, self.e1, flops, label))
        return False


def patch_last_fused_flops(family, flops):
    """bench.py's live measurement: a launch that did not know its work when it was enqueued (fine_fused with a device-side count)"""
    if PROFILE_FUSED:
        for i in range(len(PROFILE_FUSED) - 1, -1, -1):
            if PROFILE_FUSED[i][3] == family:
                e0, e1, _, nm = PROFILE_FUSED[i]
                PROFILE_FUSED[i] = (e0, e1, flops, nm)
                return


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.GimHipError("gim_amd ops need device (cuda/HIP) tensors: the product path has no CPU fallback")


def gim_dtype(t):
    return _DT[t.dtype]


def _rows(t):
    """[..., C] tensor with a uniform row stride -> (rows, ld)"""
    assert t.stride(-1) == 1
    if t.dim() == 2:
        return t.shape[0], t.stride(0)
    assert t.is_contiguous()
    return t.numel() // t.shape[-1], t.shape[-1]


# ---- layout ------------------------------------------------------------------------------------
def nchw_to_nhwc(src, dst, b_off=0):
    """src [B,C,H,W] fp32 -> dst [Btot,H,W,cpad] (fp32/bf16), images b_off.."""
    _req_cuda(src, dst)
    assert src.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous()
    B, C, H, W = src.shape
    check(lib.gim_nchw_to_nhwc(_p(src), _p(dst), B, C, H, W, dst.shape[-1], dst.shape[-1], b_off,
                               gim_dtype(dst), _stream()), "gim_nchw_to_nhwc")


def _health(word):
    """the `health` argument of the kernels that store an un-normalised residual stream (include/gim_hip.h, "fp16 range guard"): an
    int32 device tensor (one element) they OR 4 into when an fp16 value they store left the IEEE range, or None"""
    if word is not None:
        _req_cuda(word)
        assert word.dtype == torch.int32 and word.numel() >= 1
    return _p(word)


def nchw_to_nhwc_split(src, dst, b_off=0):
    """src [B,C,H,W] fp32 -> dst [Btot,H,W,ld] 16-bit with channels [hi(C) | lo(C) | hi(C) | 0...] when ld >= 3 C, [hi(C) | lo(C) |
    0...] when 2 C <= ld < 3 C (gim_nchw_to_nhwc_split)"""
    _req_cuda(src, dst)
    assert src.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and dst.dtype in HALF
    B, C, H, W = src.shape
    check(lib.gim_nchw_to_nhwc_split(_p(src), _p(dst), B, C, H, W, dst.shape[-1], b_off, gim_dtype(dst), _stream()),
          "gim_nchw_to_nhwc_split")


def stem7x7(x, ps, out_dtype=None):
    """x [B,H,W,8] 16-bit pixels ([r g b 0...] or, ps.split, [hi(3) lo(3) 0 0]) -> relu(bn1(conv1(x))) [B,Ho,Wo,64] (gim_stem7x7;
    ps = packing.pack_stem7x7)"""
    _req_cuda(x, ps.w, ps.bias)
    assert x.dtype in HALF and x.dtype == ps.w.dtype and x.is_contiguous() and x.shape[-1] == 8
    assert ps.w.numel() * 2 == lib.gim_stem7x7_weight_bytes(int(ps.split))
    B, H, W, _ = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, 64, dtype=out_dtype or x.dtype, device=x.device)
    with _Timed("stem7x7", 2.0 * B * Ho * Wo * 64 * 49 * ps.cin):   # the layer's algorithmic flops
        check(lib.gim_stem7x7(_p(x), _p(ps.w), _p(ps.bias), _p(y), B, H, W, int(ps.split), gim_dtype(x), gim_dtype(y), _stream()),
              "gim_stem7x7")
    return y


def copy_segments(pairs):
    """[(src or None, dst), ...] contiguous device tensors of equal byte size per pair (src None: dst is zero filled) -> all of
    them in ONE launch (gim_copy_segments); more than 12 pairs go out in batches."""
    pairs = [(s, d) for s, d in pairs if d.numel() > 0]
    for i in range(0, len(pairs), _lib.CopySegs.MAX):
        seg = _lib.CopySegs()
        chunk = pairs[i:i + _lib.CopySegs.MAX]
        for k, (s, d) in enumerate(chunk):
            _req_cuda(s, d)
            assert d.is_contiguous() and (s is None or (s.is_contiguous() and s.numel() * s.element_size() == d.numel() * d.element_size()))
            seg.src[k] = s.data_ptr() if s is not None else None
            seg.dst[k] = d.data_ptr()
            seg.bytes[k] = d.numel() * d.element_size()
        seg.n = len(chunk)
        check(lib.gim_copy_segments(ctypes.byref(seg), _stream()), "gim_copy_segments")


def slot_index(idx, slots, device):
    """slot indices for `slot_copy`: a host sequence / CPU tensor is range-checked against `slots` HERE and uploaded as int32; a device tensor
    is handed through as int32 (the kernel skips what is out of range, nothing waits for it).  None stays None (identity).
    The banks check the slot lists of their callers with gim_amd.bank.SlotBank.check_slots."""
    if idx is None:
        return None
    if torch.is_tensor(idx) and idx.is_cuda:
        assert idx.dim() == 1 and not idx.dtype.is_floating_point
        return idx if (idx.dtype == torch.int32 and idx.is_contiguous()) else idx.to(torch.int32).contiguous()
    host = [int(v) for v in (idx.tolist() if torch.is_tensor(idx) else idx)]
    bad = [v for v in host if not 0 <= v < slots]
    if bad:
        raise IndexError(f"slot index {bad[0]} outside [0, {slots})")
    return torch.tensor(host, dtype=torch.int32).to(device, non_blocking=True)


def slot_copy(src, dst, src_idx=None, dst_idx=None, n=None):
    """Blocks of src [S, ...] -> blocks of dst [D, ...] in ONE launch (gim_slot_copy): block src_idx[i] of src goes to block dst_idx[i] of
    dst for i < n.  Both tensors are contiguous with the same bytes per block (a multiple of 16); an index is a host sequence (checked
    here, then uploaded), a device integer tensor, or None (identity).  n defaults to the length of an index, else to S.  Destination
    indices must be distinct."""
    _req_cuda(src, dst)
    assert src.is_contiguous() and dst.is_contiguous() and src.dim() >= 1 and dst.dim() >= 1
    S, D = src.shape[0], dst.shape[0]
    bb = src[0].numel() * src.element_size() if S else dst[0].numel() * dst.element_size()
    assert D == 0 or dst[0].numel() * dst.element_size() == bb, "slot_copy: source and destination blocks differ in size"
    if bb % 16:
        raise ValueError(f"slot_copy: {bb} bytes per block is not a multiple of 16")
    si, di = slot_index(src_idx, S, src.device), slot_index(dst_idx, D, dst.device)
    lens = {t.numel() for t in (si, di) if t is not None}
    if n is None:
        n = lens.pop() if len(lens) == 1 else (S if not lens else -1)
    if any(t is not None and t.numel() < n for t in (si, di)) or n < 0:
        raise ValueError("slot_copy: the index arrays and n disagree")
    if dst_idx is not None and not (torch.is_tensor(dst_idx) and dst_idx.is_cuda):
        if len(set(int(v) for v in dst_idx)) != len(dst_idx):
            raise ValueError("slot_copy: destination indices must be distinct")
    if (si is None and n > S) or (di is None and n > D):
        raise IndexError(f"slot_copy: identity over {n} blocks needs that many slots (source {S}, destination {D})")
    check(lib.gim_slot_copy(_p(src), _p(dst), _p(si), _p(di), int(n), int(bb), int(S), int(D), _stream()), "gim_slot_copy")
    return dst


def pack_matches(m_bids, mkpts0, mkpts1, mconf, pair_ids=None, pid_base=0):
    """rows [pair_id, x0, y0, x1, y1, conf] fp32 [M, 6]; pair_id = pair_ids[m_bids] (device int64 tensor) or pid_base + m_bids"""
    _req_cuda(m_bids, mkpts0, mkpts1, mconf, pair_ids)
    M = m_bids.numel()
    assert m_bids.dtype == torch.int64 and mkpts0.dtype == mkpts1.dtype == mconf.dtype == torch.float32
    assert mkpts0.shape == (M, 2) and mkpts1.shape == (M, 2) and mconf.shape == (M,)
    assert pair_ids is None or pair_ids.dtype == torch.int64
    out = torch.empty(M, 6, dtype=torch.float32, device=m_bids.device)
    check(lib.gim_pack_matches(_p(m_bids.contiguous()), _p(mkpts0.contiguous()), _p(mkpts1.contiguous()), _p(mconf.contiguous()),
                               _p(pair_ids), int(pid_base), _p(out), M, _stream()), "gim_pack_matches")
    return out


def nhwc_to_nchw(src, C):
    """src [B,H,W,cstore] -> new fp32 [B,C,H,W] (reference layout, for tests / lazy outputs)"""
    _req_cuda(src)
    B, H, W, ld = src.shape
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=src.device)
    check(lib.gim_nhwc_to_nchw(_p(src), _p(out), B, C, H, W, ld, gim_dtype(src), _stream()), "gim_nhwc_to_nchw")
    return out


# ---- conv / linear --------------------------------------------------------------------------------
FORCE_BIG_TILE = flag("force_big_tile", False)   # tests: the 256 x 256 tile on every eligible launch, whatever its size (gim_conv_args.use_lds_dma = 3)
# fp32 operands multiplied as IEEE-fp16 hi / lo pairs on the 16-bit MFMA (gim_conv_args.split16: three products per 16 K instead of eight fp32 MFMAs, 2^-22 per
# product): the default of the launches that pass no `split16` -- gim_loftr's fp32 mode passes its own per launch (LoFTR.fp32_split)
FP32_SPLIT = flag("fp32_split_all", False)
UPS_FUSED = flag("ups_fused", True)   # FPN: bilinear x2 + add inside the lateral 1x1 conv's epilogue (False: a second pass over the output)
# 3x3 halo kernel (conv_igemm.hip: conv3x3_halo_kernel); module attributes, tests flip them (switches: conv_halo, conv_halo_min_tiles)
HALO = flag("conv_halo", True)
HALO_MIN_TILES = flag("conv_halo_min_tiles", 2000)   # round 3 sweep: below ~2000 tiles (the 1/4-resolution layers) the generic kernel is 5-8 % faster


def _conv_args(pk, geom, ldx, ldy, *, x=None, y=None, act=ACT_NONE, res=None, res_mod=0, act_cols=0, lds_dma=True, ups=None, split16=False,
               health=None, halo=False):
    """The gim_conv_args of every launch and predicate of this file (the one place that fills the struct).  geom = (B, H, W, Ho, Wo) as the
    launch states it, ldx / ldy: the row strides of input and output.  x / y: the tensors, or None -- the predicates need no pointer, the
    output is then of the pack's dtype.  res: row view of the residual; ups: the half-resolution NHWC operand of the fused upsample-add, or its
    shape; health: see `_health`, passed on to residual and split launches only.  halo: the halo kernel's form -- w / ktab / kpad / npad /
    bias of `pk.halo`, res_mod = cin_pad, use_lds_dma = 2."""
    B, H, W, Ho, Wo = geom
    w, ktab, bias, npad, kpad = pk.w, pk.ktab, pk.bias, pk.npad, pk.kpad
    if halo:
        w, ktab, nslab, bias = pk.halo
        npad, kpad, res_mod = w.shape[0], nslab * 64, pk.cin_pad
    a = _lib.ConvArgs()
    if x is not None:
        assert x.dtype == torch_dtype(pk.dtype), (x.dtype, pk.dtype)
        a.x, a.y = x.data_ptr(), y.data_ptr()
    a.w, a.ktab = w.data_ptr(), ktab.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.res = res.data_ptr() if res is not None else None
    a.x_bytes = ((B * H * W - 1) * ldx + pk.cin_pad) * (2 if halo else elem_size(pk.dtype))
    a.B, a.H, a.W, a.Ho, a.Wo = B, H, W, Ho, Wo
    a.stride, a.pad = (1, 1) if halo else (pk.stride, pk.pad)
    a.ldx, a.ldy = ldx, ldy
    a.ldres = res.stride(0) if res is not None else 0
    a.N, a.npad, a.kpad = pk.n_store, npad, kpad
    a.act, a.res_mod, a.act_cols = act, res_mod, act_cols
    a.dtype, a.out_dtype = pk.dtype, gim_dtype(y) if y is not None else pk.dtype
    a.res_dtype = gim_dtype(res) if res is not None else GIM_F32
    a.use_lds_dma = 2 if halo else (3 if FORCE_BIG_TILE else 1) if lds_dma else 0
    a.split16 = 1 if (split16 and pk.dtype == GIM_F32 and lds_dma) else 0
    # residual launches: the fp16 range guard (ORs 4); split launches: an operand beyond the fp16 range of the hi / lo split (ORs 8)
    a.health = _health(health).value if (health is not None and (res is not None or a.split16)) else None
    if ups is not None:
        if torch.is_tensor(ups):
            assert y is None or ups.dtype == y.dtype   # (what the second pass, `upsample2x_add`, asks as well)
            a.ups = ups.data_ptr()
        a.ups_h, a.ups_w, a.ups_ld = tuple(getattr(ups, "shape", ups))[1:4]
    return a


def _halo_pays(pk, B, H, W):
    """whole 8 x 32 patches, enough of them to fill 256 one-per-CU workgroups twice, and no all-padding 32-channel fragment in
    the tile (N = 196 in a 256-wide tile: the generic kernel skips that fragment, this one does not) -- measured +4..5 % on
    the layers that qualify, -2 % on the 196-channel ones"""
    if H % 8 or W % 32:
        return False
    if HALO_MIN_TILES <= 0:   # tests: every layer with a halo packing, the padded ones included
        return True
    npad = pk.halo[0].shape[0]
    bn = 256 if npad % 256 == 0 else 128
    if pk.n_store <= npad - 32:     # incl. the 64-channel layers (SuperPoint / VGG19 / ResNet stems) in the 128-wide tile: half of it would be
        return False                # padding -- the generic 256 x 64 tile is 2x faster there (profiles/r03_lightglue_kernel_stats.txt: 552 vs 280 us)
    return B * (H // 8) * (W // 32) * (npad // bn) >= HALO_MIN_TILES


def _dense_route(pk, a, xs=None, contiguous=True, tile=False):
    """Where does the dense launch of `pk` go?  a: its generic struct (`_conv_args`: operand kinds, residual, lds_dma and, with an upsample
    operand, ups_h / ups_w / ups_ld are read from it); xs: the (B, H, W) of the input map, None for a launch over rows (`conv_rows`,
    `linear`), which never leaves the generic entry; contiguous: is x?
      "halo"   `conv3x3_halo` (`conv2d` only)
      "ups"    the persistent kernel with the upsample-add in its epilogue (gim_conv_ups_supported)
      "big"    the persistent kernel on the 256 x 256 tile (gim_conv2d_big_tile) -- told from "other" only where `tile` asks for it: one more
               question to the library, whose answer no launch needs
      "other"  any other kernel of gim_conv2d_bn_act
    A launch that cannot fuse its upsample operand goes without it: `a.ups` is cleared here, so that `a` is the launch as it runs, and the
    caller adds the operand in a second pass.  `conv2d` / `conv_rows` dispatch on the answer, and the `dense_too` halves of
    `conv_tiles_supported` / `conv_ups_tiles_supported` ask it with a struct built from shapes: they assume a contiguous 16-bit x, an output
    of x's dtype, no residual and lds_dma, which is what gim_loftr's fine head hands its dense launches wherever it asks (`LoFTR._conv`;
    fine_head.py `_fine_halo`, in front of every such question, wants a 16-bit module with lds_dma)."""
    if (xs is not None and HALO and pk.halo is not None and not a.res and a.use_lds_dma in (1, 3) and a.dtype in (GIM_BF16, GIM_F16)
            and a.out_dtype == a.dtype and contiguous and _halo_pays(pk, *xs)):
        return "halo"
    if a.ups_h and UPS_FUSED and lib.gim_conv_ups_supported(ctypes.byref(a)):
        return "ups"
    a.ups = None
    return "big" if tile and lib.gim_conv2d_big_tile(ctypes.byref(a)) else "other"


def _conv_timed(pk, M, tag="", n_tiles=None):
    """`_Timed` of a conv launch (PROFILE): label = the layer's shape + tag; algorithmic flops (real channels, no padding) of M output pixels
    or, over a patch list, of the computed patches x 256 pixels -- the live measurement alone reads that count back"""
    return _Timed(lambda: f"{pk.cin}->{pk.cout} k{pk.kh}s{pk.stride} M={M}{tag}",
                  lambda: 2.0 * (M if n_tiles is None else int(n_tiles[0].item()) * 256) * pk.cout * pk.cin * pk.kh * pk.kw, conv=True)


def _conv_dense(a, pk, route):
    """gim_conv2d_bn_act of the generic struct `a`; returns whether the upsample-add went along (`_dense_route` said "ups")"""
    with _conv_timed(pk, a.B * a.Ho * a.Wo, " +ups" if route == "ups" else ""):
        check(lib.gim_conv2d_bn_act(ctypes.byref(a), _stream()), "gim_conv2d_bn_act")
    return route == "ups"


def conv_rows(x, pk, geom, y, act=ACT_NONE, res=None, res_mod=0, lds_dma=True, act_cols=0, ups=None, health=None, split16=None):
    """Generic launch.  x: 2-D row view [rows_in, ldx]; geom = (B, H, W, Ho, Wo); y: 2-D row view.  ups: half-resolution NHWC tensor whose
    bilinear x2 upsampling is added in the epilogue when the launch can take it; returns whether it was (False: the caller adds it in a
    separate pass).  split16: fp32 operands as split products (None: the module's default, FP32_SPLIT)."""
    _req_cuda(x, y, res)
    B, H, W, Ho, Wo = geom
    assert y.shape[0] >= B * Ho * Wo and y.shape[1] >= pk.n_store
    a = _conv_args(pk, geom, x.stride(0), y.stride(0), x=x, y=y, act=act, res=res, res_mod=res_mod, act_cols=act_cols, lds_dma=lds_dma, ups=ups,
                   split16=FP32_SPLIT if split16 is None else split16, health=health)
    return _conv_dense(a, pk, _dense_route(pk, a))


def conv2d(x, pk, act=ACT_NONE, res=None, out_dtype=None, lds_dma=True, ups=None, health=None, split16=None):
    """x [B,H,W,cin_pad] NHWC -> new [B,Ho,Wo,n_store].  ups: [B,Ho/2,Wo/2,n_store] -> y += bilinear_x2(ups) (align_corners=True):
    in the conv's epilogue when the launch supports it, otherwise as a second pass (gim_upsample2x_add).  `_dense_route` picks the kernel."""
    B, H, W, cs = x.shape
    assert cs == pk.cin_pad, (cs, pk)
    d = getattr(pk, "dil", 1)       # dilated taps (packing.pack_conv(dilation=)): effective extent (k - 1) d + 1
    Ho = (H + 2 * pk.pad - (pk.kh - 1) * d - 1) // pk.stride + 1
    Wo = (W + 2 * pk.pad - (pk.kw - 1) * d - 1) // pk.stride + 1
    y = torch.empty(B, Ho, Wo, pk.n_store, dtype=out_dtype or x.dtype, device=x.device)
    r = res.view(-1, res.shape[-1]) if res is not None else None
    _req_cuda(x, y, res)
    geom = (B, H, W, Ho, Wo)
    if pk.kh == 1 and pk.kw == 1 and pk.stride == 1 and pk.pad == 0:
        geom = (1, 1, B * H * W, 1, B * H * W)  # pixel index == row index: the kernel skips the coordinate decode
    a = _conv_args(pk, geom, x.view(-1, cs).stride(0), pk.n_store, x=x, y=y, act=act, res=r, lds_dma=lds_dma, ups=ups,
                   split16=FP32_SPLIT if split16 is None else split16, health=health)
    route = _dense_route(pk, a, (B, H, W), x.is_contiguous())
    if route == "halo":
        conv3x3_halo(x, pk, y, act)
        return y
    if ups is not None:
        assert ups.shape == (B, Ho // 2, Wo // 2, pk.n_store) and res is None and ups.is_contiguous()
    if not _conv_dense(a, pk, route) and ups is not None:
        upsample2x_add(ups, y)
    return y


def _tile_list(tiles, n_tiles):
    """a patch list as the list-walking launches take it (int32 device tensors; the count stays on the device) -> its three C arguments"""
    assert tiles.dtype == n_tiles.dtype == torch.int32 and tiles.is_contiguous() and n_tiles.numel() >= 1
    return _p(tiles), _p(n_tiles), tiles.numel()


def conv3x3_halo(x, pk, y, act=ACT_NONE, tiles=None, n_tiles=None):
    """x [B,H,W,cin_pad] bf16 -> y [B,H,W,n_store] bf16 through the halo-tile kernel (3x3, stride 1, pad 1, no residual).
    tiles / n_tiles (int32 device tensors, `fine_tile_lists`): only the 8 x 32 patches tiles[:n_tiles[0]] are computed, the count stays on
    the device; every other pixel of y keeps what it held (gim_conv3x3_halo_tiles)."""
    _req_cuda(x, y, tiles, n_tiles)
    assert x.is_contiguous() and y.is_contiguous(), "conv3x3_halo addresses pixels as (b*H + y)*W + x rows of width cin_pad"
    B, H, W, cs = x.shape
    a = _conv_args(pk, (B, H, W, H, W), cs, y.shape[-1], x=x, y=y, act=act, halo=True)
    assert tiles is None or y.shape[:3] == x.shape[:3]
    with _conv_timed(pk, B * H * W, " halo" + ("" if tiles is None else " sparse"), n_tiles):
        if tiles is None:
            check(lib.gim_conv2d_bn_act(ctypes.byref(a), _stream()), "gim_conv2d_bn_act(halo)")
        else:
            check(lib.gim_conv3x3_halo_tiles(ctypes.byref(a), *_tile_list(tiles, n_tiles), _stream()), "gim_conv3x3_halo_tiles")


def conv_ups_tiles_supported(x, pk, ups, act=ACT_NONE, res=None, dense_too=False):
    """does `conv2d_ups_tiles` take this lateral launch?  x [B,H,W,cin_pad] / ups [B,H/2,W/2,n_store]: tensors or shapes
    (gim_conv_ups_tiles_supported: a bare 16-bit 1x1 conv onto a map of whole 8 x 32 patches).  dense_too: ... and would `conv2d` fuse the
    upsample-add into the dense launch of the same shape as well (`_dense_route`, with what it assumes of a launch stated by its shapes)?
    Only then are the two bit-identical: the two-pass path rounds the conv output before the add."""
    xs, us = tuple(getattr(x, "shape", x)), tuple(getattr(ups, "shape", ups))
    if not (UPS_FUSED and pk.kh == 1 and pk.kw == 1 and pk.stride == 1 and pk.pad == 0 and xs[3] == pk.cin_pad):
        return False
    if us != (xs[0], xs[1] // 2, xs[2] // 2, pk.n_store) or xs[1] % 2 or xs[2] % 2:
        return False
    rows = xs[0] * xs[1] * xs[2]
    a = _conv_args(pk, (1, 1, rows, 1, rows), xs[3], pk.n_store, act=act, ups=us)
    a.res = 1 if res is not None else None   # (the predicate looks at whether there is one)
    return bool(lib.gim_conv_ups_tiles_supported(ctypes.byref(a)) and (not dense_too or _dense_route(pk, a, xs[:3]) == "ups"))


def conv2d_ups_tiles(x, pk, ups, tiles, n_tiles, y=None):
    """`conv2d(x, pk, ups=ups)` -- the FPN's lateral 1x1 conv + bilinear x2 of `ups` + add -- on the 8 x 32 patches tiles[:n_tiles[0]] of
    y [B,H,W,n_store] only (int32 device tensors, `fine_tile_lists`; the count stays on the device): listed patches get the bits the dense
    launch writes, every other pixel of y keeps what it held (gim_conv2d_ups_tiles).  A launch the entry does not take
    (`conv_ups_tiles_supported`) runs dense."""
    _req_cuda(x, ups, tiles, n_tiles, y)
    if not (x.is_contiguous() and ups.is_contiguous() and x.dtype in HALF and ups.dtype == x.dtype and conv_ups_tiles_supported(x, pk, ups)):
        return conv2d(x, pk, ups=ups)
    B, H, W, cs = x.shape
    if y is None:
        y = torch.empty(B, H, W, pk.n_store, dtype=x.dtype, device=x.device)
    assert y.shape == (B, H, W, pk.n_store) and y.is_contiguous() and y.dtype == x.dtype
    rows = B * H * W
    a = _conv_args(pk, (1, 1, rows, 1, rows), cs, pk.n_store, x=x, y=y, ups=ups)
    with _conv_timed(pk, rows, " +ups sparse", n_tiles):
        check(lib.gim_conv2d_ups_tiles(ctypes.byref(a), *_tile_list(tiles, n_tiles), _stream()), "gim_conv2d_ups_tiles")
    return y


def conv_tiles_supported(x, pk, dense_too=False):
    """does `conv2d_tiles` take this launch?  x [B,H,W,cin_pad]: a tensor or its shape (gim_conv2d_tiles_supported: a 16-bit 3 x 3 /
    stride 1 / pad 1 conv without residual onto a map of whole 8 x 32 patches, 256-channel tile columns).  dense_too: ... and does `conv2d`
    run the dense launch of the same shape on the same 256 x 256 tile (`_dense_route`, with what it assumes of a launch stated by its shape;
    not the halo kernel, whose K order differs)?  Only then are the two bit-identical."""
    xs = tuple(getattr(x, "shape", x))
    if not (pk.kh == 3 and pk.kw == 3 and pk.stride == 1 and pk.pad == 1 and getattr(pk, "dil", 1) == 1 and xs[3] == pk.cin_pad
            and pk.dtype in (GIM_BF16, GIM_F16)):
        return False
    a = _conv_args(pk, xs[:3] + xs[1:3], xs[3], pk.n_store)
    return bool(lib.gim_conv2d_tiles_supported(ctypes.byref(a)) and (not dense_too or _dense_route(pk, a, xs[:3], tile=True) == "big"))


def conv2d_tiles(x, pk, tiles, n_tiles, act=ACT_NONE, out=None):
    """`conv2d(x, pk, act)` for a 3 x 3 / stride 1 / pad 1 layer on the 8 x 32 patches tiles[:n_tiles[0]] of out [B,H,W,n_store] only
    (int32 device tensors, `fine_tile_lists`; the count stays on the device): listed patches get the bits the dense launch writes on the
    256 x 256 tile, every other pixel of `out` keeps what it held (gim_conv2d_tiles).  A launch the entry does not take
    (`conv_tiles_supported`) runs dense."""
    _req_cuda(x, tiles, n_tiles, out)
    if not (x.is_contiguous() and x.dtype in HALF and conv_tiles_supported(x, pk)):
        return conv2d(x, pk, act)
    B, H, W, cs = x.shape
    if out is None:
        out = torch.empty(B, H, W, pk.n_store, dtype=x.dtype, device=x.device)
    assert out.shape == (B, H, W, pk.n_store) and out.is_contiguous() and out.dtype == x.dtype
    a = _conv_args(pk, (B, H, W, H, W), cs, pk.n_store, x=x, y=out, act=act)
    with _conv_timed(pk, B * H * W, " sparse", n_tiles):
        check(lib.gim_conv2d_tiles(ctypes.byref(a), *_tile_list(tiles, n_tiles), _stream()), "gim_conv2d_tiles")
    return out


FINE_TILE_MAX_FLAGS = lib.gim_fine_tile_list_max_flags()


def _match_list_cap(b_ids, i_ids, j_ids, count, *more):
    """what the patch-list launches ask of the match lists (int64, contiguous, on the device like `count` and `more`); returns their capacity"""
    _req_cuda(b_ids, i_ids, j_ids, count, *more)
    assert b_ids.dtype == i_ids.dtype == j_ids.dtype == torch.int64 and count.dtype == torch.int32
    assert b_ids.is_contiguous() and i_ids.is_contiguous() and j_ids.is_contiguous()
    return min(b_ids.numel(), i_ids.numel(), j_ids.numel())


class TileLists(NamedTuple):
    """what `fine_tile_lists` returns: each list with its device-side count; the fields its depth does not build are None"""
    tiles: torch.Tensor                        # half level, reach +-3: the two 3 x 3 layers of layer1_outconv2
    n_tiles: torch.Tensor
    tiles4: Optional[torch.Tensor] = None      # depth >= 2: half level, reach +-4: the lateral in front of them
    n_tiles4: Optional[torch.Tensor] = None
    tilesq: Optional[torch.Tensor] = None      # depth 3: [3, total / 4] quarter-level lists A, B, C
    n_tilesq: Optional[torch.Tensor] = None


def fine_tile_lists(b_ids, i_ids, j_ids, count, bs, w0c, w1c, stride, H, W, depth=1, b_range=None, tiles=None, n_tiles=None):
    """The patch lists of the sparse fine head's last `depth` stages, from ONE one-workgroup launch that reads the match count on the device:
    ascending lists of 8 x 32 patches that the fine windows of the first min(count[0], capacity) matches reach.
      depth 1  (gim_fine_tile_list)   tiles int32 [2 bs ceil(H/8) ceil(W/32)], n_tiles int32 [1]: the patches of the 1/2-resolution maps
               [2 bs, H, W, .] reached through one 3 x 3 convolution (+-3 around stride * cell).  tiles / n_tiles: the caller's buffers.
      depth 2  (gim_fine_tile_lists)  ... and tiles4 / n_tiles4, the list of the reach grown by one pixel (+-4): the patches whose lateral
               sum the last-but-one 3 x 3 layer reads.
      depth 3  (gim_fine_tile_lists4; H % 16 == 0, W % 64 == 0)  ... and tilesq [3, total/4] / n_tilesq [3], three lists of the
               1/4-resolution maps [2 bs, H/2, W/2] in front of the lateral that walks tiles4: every upsample source that launch stages (S)
               dilated by 2 (list A), by 1 (B), and S itself (C).  b_range = (b_lo, b_hi): only the matches of those pairs mark patches
               (gim_fine_tile_lists4_range; indices and buffer sizes stay those of the whole batch)."""
    if b_range is not None and depth < 3:
        raise ValueError("fine_tile_lists: a pair range needs depth 3 (gim_fine_tile_lists4_range)")
    assert depth in (1, 2, 3) and (depth == 1 or (tiles is None and n_tiles is None)), "caller-supplied buffers are a depth-1 feature"
    cap = _match_list_cap(b_ids, i_ids, j_ids, count, tiles, n_tiles)
    head = (_p(b_ids), _p(i_ids), _p(j_ids), _p(count), cap, bs, w0c, w1c, stride, H, W)
    new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=b_ids.device)   # noqa: E731
    total = 2 * bs * ((H + 7) // 8) * ((W + 31) // 32)
    if depth == 1:
        tiles = new(total) if tiles is None else tiles
        n_tiles = new(1) if n_tiles is None else n_tiles
        check(lib.gim_fine_tile_list(*head, *_tile_list(tiles, n_tiles), _stream()), "gim_fine_tile_list")
        return TileLists(tiles, n_tiles)
    assert depth == 2 or (H % 16 == 0 and W % 64 == 0), (H, W)
    totq = total // 4
    t, n = new(2 * total + (3 * totq if depth == 3 else 0)), new(5 if depth == 3 else 2)
    lists = TileLists(t[:total], n[0:1], t[total:2 * total], n[1:2], *((t[2 * total:].view(3, totq), n[2:5]) if depth == 3 else ()))
    half = (_p(lists.tiles), _p(lists.n_tiles), _p(lists.tiles4), _p(lists.n_tiles4), total)
    if depth == 2:
        check(lib.gim_fine_tile_lists(*head, *half, _stream()), "gim_fine_tile_lists")
    elif b_range is None:
        check(lib.gim_fine_tile_lists4(*head, *half, _p(lists.tilesq), _p(lists.n_tilesq), totq, _stream()), "gim_fine_tile_lists4")
    else:
        check(lib.gim_fine_tile_lists4_range(*head, *half, _p(lists.tilesq), _p(lists.n_tilesq), totq, int(b_range[0]), int(b_range[1]), _stream()),
              "gim_fine_tile_lists4_range")
    return lists


def fine_tile_lists4_fits(bs, H, W):
    """do the half- and quarter-level patch flags of [2 bs, H, W] fit the one-workgroup list kernel, and is the quarter map whole patches?"""
    if H % 16 or W % 64:
        return False
    total = 2 * bs * (H // 8) * (W // 32)
    return ((total + 3) & ~3) + total // 4 <= FINE_TILE_MAX_FLAGS


def linear(x, pk, y, act=ACT_NONE, lds_dma=True, act_cols=0, health=None, split16=None):
    """x: row view [rows, >=K] (row stride may exceed K), y: row view [rows, >=N].  y = act(x @ W^T);
    act_cols > 0 restricts the activation to output columns < act_cols.  health: see conv_rows (split launches only here)."""
    rows = x.shape[0]
    conv_rows(x, pk, (1, 1, rows, 1, rows), y, act, None, 0, lds_dma, act_cols, health=health, split16=split16)


# ---- elementwise ------------------------------------------------------------------------------------
def upsample2x_add(x, y):
    """y [B,2h,2w,C] += bilinear2x(x [B,h,w,C]) (align_corners=True), in place"""
    _req_cuda(x, y)
    B, h, w, C = x.shape
    assert y.shape == (B, 2 * h, 2 * w, C) and x.dtype == y.dtype
    check(lib.gim_upsample2x_add(_p(x), _p(y), B, h, w, C, C, C, gim_dtype(x), _stream()), "gim_upsample2x_add")


def posenc_add(x, pe, out_f32, out_t):
    """x rows [R, C] (dtype T); pe [hw, C] fp32; out_f32 row view and/or out_t row view"""
    _req_cuda(x, pe, out_f32, out_t)
    R, C = x.shape
    check(lib.gim_posenc_add(_p(x), _p(pe), _p(out_f32), _p(out_t), R, pe.shape[0], C, x.stride(0),
                             out_f32.stride(0) if out_f32 is not None else 4,
                             out_t.stride(0) if out_t is not None else 4, gim_dtype(x), _stream()), "gim_posenc_add")


def layernorm_residual(x, gamma, beta, res, out_f32, out_t, eps=1e-5):
    """x fp32 / bf16 row view [R, C]; out_f32 / out_t row views (either may be None)"""
    _req_cuda(x, gamma, beta, res, out_f32, out_t)
    R, C = x.shape
    dt = gim_dtype(out_t) if out_t is not None else GIM_F32
    check(lib.gim_layernorm_residual(_p(x), _p(gamma), _p(beta), _p(res), _p(out_f32), _p(out_t), R, C,
                                     x.stride(0), res.stride(0) if res is not None else 4,
                                     out_f32.stride(0) if out_f32 is not None else 4,
                                     out_t.stride(0) if out_t is not None else 4, gim_dtype(x), dt, eps, _stream()),
          "gim_layernorm_residual")


# ---- linear attention ---------------------------------------------------------------------------------
def linear_attention(q, k, v, out, nb_q, L, nb_kv, S, H, ws=None, q_mask=None, kv_mask=None):
    """q row view [nb_q*L, C]; k,v row views [nb_kv*S, C]; nb_q == nb_kv.  out row view [nb_q*L, C].
    q_mask [nb_q*L] / kv_mask [nb_kv*S]: uint8 padding masks or None."""
    _req_cuda(q, k, v, out, q_mask, kv_mask)
    assert nb_q == nb_kv
    C = H * (q.shape[1] // H)
    D = q.shape[1] // H
    if H == 8 and D in (16, 32) and L <= 64 and S <= 64:  # short sequences: fused single-launch kernel
        check(lib.gim_linear_attention_short(_p(q), _p(k), _p(v), _p(q_mask), _p(kv_mask), _p(out), nb_q, L, S, H, D,
                                             q.stride(0), k.stride(0), v.stride(0), out.stride(0), gim_dtype(q),
                                             gim_dtype(out), _stream()), "gim_linear_attention_short")
        return ws
    need = lib.gim_linear_attention_ws_bytes(nb_kv, S, H, D)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=q.device)
    check(lib.gim_linear_attention_kv(_p(k), _p(v), _p(kv_mask), _p(ws), nb_kv, S, H, D, k.stride(0), v.stride(0),
                                      gim_dtype(k), _stream()), "gim_linear_attention_kv")
    check(lib.gim_linear_attention_apply(_p(q), _p(q_mask), _p(ws), _p(out), nb_q, L, S, H, D, q.stride(0), out.stride(0),
                                         gim_dtype(q), gim_dtype(out), _stream()), "gim_linear_attention_apply")
    return ws


# ---- coarse matching -----------------------------------------------------------------------------------
class CoarseResult:
    __slots__ = ("args", "ws", "count", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "keep")


def coarse_match(feat0, feat1, hw0_c, hw1_c, scale, temperature=0.1, thr=0.2, border_rm=2,
                 scale0=None, scale1=None, mask0=None, mask1=None, count=None, precand_per_row=0):
    """feat0 [N,L,C], feat1 [N,S,C], fp32 or bf16, rows possibly strided (stride(1) = ldf >= C, the same for both; e.g. a
    column range of the transformer's token buffers).  bf16 features run the similarity on the bf16 MFMA (exact products,
    fp32 accumulation).  Returns CoarseResult with cap-sized device buffers; count[0] (device int32) is the number of
    valid leading entries."""
    _req_cuda(feat0, feat1, scale0, scale1)
    assert feat0.dtype == feat1.dtype and feat0.dtype in (torch.float32, torch.bfloat16, torch.float16)
    ldf = feat0.stride(1)
    for f in (feat0, feat1):
        assert f.dim() == 3 and f.stride(2) == 1 and f.stride(1) == ldf and f.stride(0) == f.shape[1] * ldf, (f.shape, f.stride())
    N, L, C = feat0.shape
    S = feat1.shape[1]
    dev = feat0.device
    cap = N * min(L, S)
    r = CoarseResult()
    r.ws = torch.empty(lib.gim_coarse_match_ws_bytes(N, L, S), dtype=torch.uint8, device=dev)
    # [M, health word, per-pair counts].  Bit 1 of the health word is sticky (include/gim_hip.h): a caller that captures this call
    # into a graph passes a `count` buffer it zeroed OUTSIDE the capture, so that replays do not clear the bit
    if count is not None:
        assert count.dtype == torch.int32 and count.numel() >= 2 + N and count.device == dev and count.is_contiguous()
    r.count = torch.zeros(2 + N, dtype=torch.int32, device=dev) if count is None else count
    r.b_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    r.i_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    r.j_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    r.mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    r.mkpts0_c = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    r.mkpts1_c = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    if scale0 is not None:
        scale0 = scale0.to(device=dev, dtype=torch.float32).contiguous()
        scale1 = scale1.to(device=dev, dtype=torch.float32).contiguous()
    if mask0 is not None:
        assert mask0.dtype == torch.uint8 and mask1.dtype == torch.uint8 and mask0.is_contiguous() and mask1.is_contiguous()
        assert mask0.numel() == N * L and mask1.numel() == N * S
    r.keep = (feat0, feat1, scale0, scale1, mask0, mask1)
    a = _lib.CoarseArgs()
    a.feat0, a.feat1 = feat0.data_ptr(), feat1.data_ptr()
    a.scale0 = scale0.data_ptr() if scale0 is not None else None
    a.scale1 = scale1.data_ptr() if scale1 is not None else None
    a.mask0 = mask0.data_ptr() if mask0 is not None else None
    a.mask1 = mask1.data_ptr() if mask1 is not None else None
    a.ws, a.count = r.ws.data_ptr(), r.count.data_ptr()
    a.b_ids, a.i_ids, a.j_ids = r.b_ids.data_ptr(), r.i_ids.data_ptr(), r.j_ids.data_ptr()
    a.mconf, a.mkpts0_c, a.mkpts1_c = r.mconf.data_ptr(), r.mkpts0_c.data_ptr(), r.mkpts1_c.data_ptr()
    a.N, a.L, a.S, a.C = N, L, S, C
    a.h0c, a.w0c, a.h1c, a.w1c = hw0_c[0], hw0_c[1], hw1_c[0], hw1_c[1]
    a.cap, a.temperature, a.thr, a.border_rm, a.scale = cap, temperature, thr, border_rm, scale
    a.feat_dtype, a.ldf = gim_dtype(feat0), ldf
    a.precand_per_row = precand_per_row   # 0: the default capacity; -1: none (tests force the overflow -> recompute fallback)
    r.args = a
    with _Timed("coarse_match", 2.0 * N * L * S * C):   # the similarity GEMM's flops (computed once in the common case)
        check(lib.gim_coarse_match(ctypes.byref(a), _stream()), "gim_coarse_match")
    return r


def coarse_conf_matrix(r):
    """Materialise conf_matrix [N,L,S] from the statistics of a previous coarse_match call."""
    a = r.args
    conf = torch.empty(a.N, a.L, a.S, dtype=torch.float32, device=r.count.device)
    check(lib.gim_coarse_conf_matrix(ctypes.byref(a), _p(conf), _stream()), "gim_coarse_conf_matrix")
    return conf


# ---- fine level ---------------------------------------------------------------------------------------
def fine_gather(feat_f0, feat_f1, b_ids, i_ids, j_ids, M, w0c, w1c, stride, W, out_f32, out_t):
    """feat_f0 [bs,hf0,wf0,C], feat_f1 [bs,hf1,wf1,C] NHWC; out_* row views [2*M*W*W, >=C]"""
    _req_cuda(feat_f0, feat_f1, b_ids, out_f32, out_t)
    _, hf0, wf0, C = feat_f0.shape
    _, hf1, wf1, _ = feat_f1.shape
    assert feat_f0.is_contiguous() and feat_f1.is_contiguous() and feat_f1.shape[3] == C
    check(lib.gim_fine_gather(_p(feat_f0), _p(feat_f1), _p(b_ids), _p(i_ids), _p(j_ids), _p(out_f32), _p(out_t),
                              M, hf0, wf0, hf1, wf1, C, C, w0c, w1c, stride, W,
                              out_f32.stride(0) if out_f32 is not None else 4,
                              out_t.stride(0) if out_t is not None else 4, gim_dtype(feat_f0), _stream()),
          "gim_fine_gather")


def fine_match(f0, f1, mkpts1_c, b_ids, scale1, M, WW, scale, has_scale0):
    """f0/f1 fp32 row views [M*WW, C].  Returns (expec_f [M,3], mkpts1_f [M,2])."""
    _req_cuda(f0, f1, mkpts1_c)
    dev = f0.device
    expec = torch.empty(M, 3, dtype=torch.float32, device=dev)
    mk1 = torch.empty(M, 2, dtype=torch.float32, device=dev)
    if M > 0:
        check(lib.gim_fine_match(_p(f0), _p(f1), _p(mkpts1_c), _p(b_ids), _p(scale1), _p(expec), _p(mk1), M, WW,
                                 f0.shape[1], f0.stride(0), scale, 1 if has_scale0 else 0, _stream()),
              "gim_fine_match")
    return expec, mk1


def _outs(out, shapes, like):
    """output tensors of a fused launch: fresh ones, or the caller's (`out` = a tuple aligned with `shapes`; None entries are
    allocated here) -- contiguous slices of a larger batch when a caller runs image groups separately"""
    res = []
    for i, shp in enumerate(shapes):
        o = out[i] if out is not None else None
        if shp is None:
            res.append(None)
        elif o is None:
            res.append(torch.empty(*shp, dtype=like.dtype, device=like.device))
        else:
            assert tuple(o.shape) == tuple(shp) and o.dtype == like.dtype and o.is_contiguous(), (o.shape, shp)
            res.append(o)
    return res


def bneck64(t1, res, pk, want_next, out=None, health=None):
    """Fused Bottleneck tail (+ the next conv1): t1 [B,H,W,64] bf16, res [B,H,W,256] bf16 -> (x' [B,H,W,256], t1' [B,H,W,N1] or None).
    pk = packing.pack_bneck(...); N1 = 64 (next block of the layer) or 128 (the next layer's first conv1) from the packed weights."""
    _req_cuda(t1, res)
    assert t1.dtype in HALF and res.dtype == t1.dtype and t1.is_contiguous() and res.is_contiguous()
    assert pk[0].dtype == t1.dtype, "bneck64: weights packed for the other 16-bit kind"
    B, H, W, _ = t1.shape
    w2, w3, w1n, b2, b3, b1n = pk
    n1 = w1n.shape[0] if (want_next and w1n is not None) else 0
    assert not want_next or n1 in (64, 128)
    xo, t1n = _outs(out, ((B, H, W, 256), (B, H, W, n1) if n1 else None), t1)
    with _Timed("bneck64_fused", 2.0 * B * H * W * (576 * 64 + 64 * 256 + 256 * n1)):
        check(lib.gim_bneck64_fused(_p(t1), _p(res), _p(xo), _p(t1n), _p(w2), _p(w3), _p(w1n if n1 else None), _p(b2), _p(b3),
                                    _p(b1n if n1 else None), B, H, W, n1, gim_dtype(t1), _health(health), _stream()), "gim_bneck64_fused")
    return xo, t1n


def bneck64_ds(t1, x_in, pk, out=None, health=None):
    """First block of layer 1 with its downsample branch computed in the kernel (gim_bneck64_fused_ds): t1 [B,H,W,64] (conv1 output),
    x_in [B,H,W,64] (the block's input) -> (x' [B,H,W,256], t1' [B,H,W,64]); pk = packing.pack_bneck_ds(...)."""
    _req_cuda(t1, x_in)
    assert t1.dtype in HALF and x_in.dtype == t1.dtype and t1.is_contiguous() and x_in.is_contiguous() and x_in.shape == t1.shape
    w2, w3, wds, w1n, b2, b3ds, b1n = pk
    assert w2.dtype == t1.dtype and w1n.shape[0] == 64
    B, H, W, _ = t1.shape
    xo, t1n = _outs(out, ((B, H, W, 256), (B, H, W, 64)), t1)
    with _Timed("bneck64_fused", 2.0 * B * H * W * (576 * 64 + 64 * 256 + 64 * 256 + 256 * 64)):
        check(lib.gim_bneck64_fused_ds(_p(t1), _p(x_in), _p(xo), _p(t1n), _p(w2), _p(w3), _p(wds), _p(w1n), _p(b2), _p(b3ds), _p(b1n), B, H, W,
                                       gim_dtype(t1), _health(health), _stream()), "gim_bneck64_fused_ds")
    return xo, t1n


def bneck_tail(t2, res, pk, act_next=ACT_RELU, store_x=True, out=None, health=None):
    """Bottleneck tail + the next 1x1 convolution in one launch (planes P = 128: layer 2, P = 256: layer 3): t2 [B,H,W,P], res
    [B,H,W,4P] (same 16-bit dtype) -> (x' [B,H,W,4P] or None when store_x is False, t1' [B,H,W,N1]); pk = packing.pack_bneck_tail(...).
    B*H*W must be a multiple of 256."""
    _req_cuda(t2, res)
    assert t2.dtype in HALF and res.dtype == t2.dtype and t2.is_contiguous() and res.is_contiguous()
    w3, w1n, b3, b1n = pk
    assert w3.dtype == t2.dtype, "bneck_tail: weights packed for the other 16-bit kind"
    B, H, W, pl = t2.shape
    M, n1 = B * H * W, w1n.shape[1]
    assert pl in (128, 256) and w3.shape == (4 * pl, pl) and res.shape == (B, H, W, 4 * pl) and M % 256 == 0
    assert store_x or pl == 256
    xo, t1n = _outs(out, ((B, H, W, 4 * pl) if store_x else None, (B, H, W, n1)), t2)
    fn = lib.gim_bneck_tail128 if pl == 128 else lib.gim_bneck_tail256
    with _Timed("bneck_tail", 2.0 * M * (pl * 4 * pl + 4 * pl * n1)):
        check(fn(_p(t2), _p(res), _p(xo), _p(t1n), _p(w3), _p(w1n), _p(b3), _p(b1n), M, n1, act_next, gim_dtype(t2), _health(health), _stream()),
              "gim_bneck_tail%d" % pl)
    return xo, t1n


def bneck_tail_ds(t2, x_in, pk, act_next=ACT_RELU, out=None, health=None):
    """First block of layer 2 with its downsample branch inside the tail kernel (gim_bneck_tail128_ds): t2 [B,Ho,Wo,128] (conv2 output),
    x_in [B,Hin,Win,256] (the block's input; the stride-2 1x1 downsample convolution reads pixel (2y, 2x)) -> (x' [B,Ho,Wo,512], t1'
    [B,Ho,Wo,128]); pk = packing.pack_bneck_tail(blk, next_conv, next_bn, ..., ds=True)."""
    _req_cuda(t2, x_in)
    assert t2.dtype in HALF and x_in.dtype == t2.dtype and t2.is_contiguous() and x_in.is_contiguous()
    w3, w1n, b3, b1n = pk
    assert w3.dtype == t2.dtype, "bneck_tail_ds: weights packed for the other 16-bit kind"
    B, Ho, Wo, pl = t2.shape
    _, Hin, Win, cd = x_in.shape
    n1 = w1n.shape[1]
    assert pl == 128 and cd == 256 and w3.shape == (512, 384) and w1n.shape == (16, 128, 32) and x_in.shape[0] == B
    assert (Hin - 1) // 2 + 1 == Ho and (Win - 1) // 2 + 1 == Wo and (B * Ho * Wo) % 256 == 0
    xo, t1n = _outs(out, ((B, Ho, Wo, 512), (B, Ho, Wo, n1)), t2)
    with _Timed("bneck_tail", 2.0 * B * Ho * Wo * ((pl + cd) * 4 * pl + 4 * pl * n1)):
        check(lib.gim_bneck_tail128_ds(_p(t2), _p(x_in), _p(xo), _p(t1n), _p(w3), _p(w1n), _p(b3), _p(b1n), B, Ho, Wo, Hin, Win, n1, act_next,
                                       gim_dtype(t2), _health(health), _stream()), "gim_bneck_tail128_ds")
    return xo, t1n


def token_mlp(msg, xb, x32, weights, ln_params, eps, kv=None, L=0, S=0, q_mask=None, emit=None, q_weights=None):
    """x += norm2(mlp.2(relu(mlp.0(cat[x, norm1(merge(msg))])))) on row views: msg [R, >=256] bf16, xb [R, >=256] bf16 (operand copy
    of x, updated in place), x32 [R, >=256] fp32 (updated in place).  With `kv` (the fp32 state of linear_attention_state) the
    attention's apply step is fused in front: `msg` then holds the elu+1 query rows of R / L sequences, S = source length.
    `emit` = (stream from packing.pack_token_emit, [(out [R, >=256] 16-bit row view, act, row_lo, row_hi), ...]): projection blocks
    act(x_new W_b^T) of the new x, written for the rows of the 64-row tiles that start in [row_lo, row_hi).
    A block entry with a fifth element (ws, nb_kv, nchunk, tile0, src_len) is the K block of a fused (k, v) pair -- the next entry is its V block, `out`
    of both may be None: nothing is written but each tile's partial KV state into the partial area of the linear-attention workspace `ws`
    (kv_state_workspace) of the call that consumes these rows as its source; kv_state_finalize(ws, ...) completes it.
    `q_weights` (with `kv`; pack_token_emit([Wq]) of this layer): `msg` may be None -- the query rows are projected inside the kernel from xb."""
    if msg is None:
        assert q_weights is not None and kv is not None, "token_mlp: msg=None needs q_weights and kv"
        msg = xb
    _req_cuda(msg, xb, x32, weights, ln_params, kv, q_mask, q_weights)
    assert msg.dtype in HALF and xb.dtype == msg.dtype and weights.dtype == msg.dtype and x32.dtype == torch.float32
    assert msg.stride(1) == 1 and xb.stride(1) == 1 and x32.stride(1) == 1 and msg.shape[0] == xb.shape[0] == x32.shape[0]
    R = msg.shape[0]
    flops = 2.0 * R * (256 * 256 + 512 * 512 + 512 * 256 + (32 * 256 if kv is not None else 0))
    em = None
    if q_weights is not None:
        assert kv is not None and q_weights.dtype == msg.dtype and q_weights.numel() == 256 * 256 and q_weights.is_contiguous()
        em = _lib.TokenEmit()
        em.q_weights = q_weights.data_ptr()
        flops += 2.0 * R * 256 * 256
    if emit:
        ew, blocks = emit
        assert 0 < len(blocks) <= _lib.TokenEmit.MAX and ew.dtype == msg.dtype and ew.is_cuda and ew.numel() == len(blocks) * 256 * 256
        em = em or _lib.TokenEmit()
        em.nblk, em.weights = len(blocks), ew.data_ptr()
        flops += _fill_emit_blocks(em, blocks, R, msg.dtype)
    with _Timed("token_mlp", flops):
        if em is None:
            check(lib.gim_token_mlp(_p(msg), _p(xb), _p(x32), _p(weights), _p(ln_params), _p(kv), _p(q_mask), R, 256, L, S,
                                    msg.stride(0), xb.stride(0), x32.stride(0), eps, gim_dtype(msg), _stream()), "gim_token_mlp")
        else:
            check(lib.gim_token_mlp_emit(_p(msg), _p(xb), _p(x32), _p(weights), _p(ln_params), _p(kv), _p(q_mask), R, 256, L, S,
                                         msg.stride(0), xb.stride(0), x32.stride(0), eps, gim_dtype(msg), ctypes.byref(em), _stream()),
                  "gim_token_mlp_emit")


def linear_attention_state(k, v, nb_kv, S, H, ws=None, kv_mask=None):
    """First half of linear_attention: KV / Ksum state of nb_kv sequences of S rows.  Returns (ws, need): the fp32 workspace
    (re-used when the one passed in is large enough) and the bytes the call needs of it.  The final state -- per sequence and
    head a D x D KV block followed by the D-vector Ksum, nb_kv*H*(D*D+D) floats -- sits at the START of the workspace, the
    per-chunk partials behind it (gim_linear_attention_kv); `ws` itself is what gim_token_mlp takes as `kv`.  NB the fused apply
    in token_mlp rounds KV to bf16 for the bf16 MFMA, the stand-alone la_apply kernel multiplies it in fp32."""
    _req_cuda(k, v, kv_mask)
    D = k.shape[1] // H
    need = lib.gim_linear_attention_ws_bytes(nb_kv, S, H, D)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=k.device)
    check(lib.gim_linear_attention_kv(_p(k), _p(v), _p(kv_mask), _p(ws), nb_kv, S, H, D, k.stride(0), v.stride(0),
                                      gim_dtype(k), _stream()), "gim_linear_attention_kv")
    return ws, need


def token_project(xb, emit, pos=None):
    """Projection blocks of the 16-bit rows `xb` [R, >= 256] as they are (gim_token_mlp_emit with project_only): `emit` as in token_mlp --
    the first layer's (k, v) pair handed over as partial KV states instead of a projection GEMM, its rows and la_kv launches.
    `pos` = (feat [R, 256] 16-bit rows, pe [hw, 256] fp32, x32 [R, >= 256] fp32 row view): the positional encoding in front (posenc_add's
    arithmetic) -- the kernel computes the rows feat + pe[row % hw] itself and WRITES them to x32 and xb before it projects them."""
    _req_cuda(xb)
    assert xb.dtype in HALF and xb.stride(1) == 1 and xb.shape[1] >= 256
    ew, blocks = emit
    R = xb.shape[0]
    assert 0 < len(blocks) <= _lib.TokenEmit.MAX and ew.dtype == xb.dtype and ew.is_cuda and ew.numel() == len(blocks) * 256 * 256
    em = _lib.TokenEmit()
    em.nblk, em.weights, em.project_only = len(blocks), ew.data_ptr(), 1
    x32 = None
    if pos is not None:
        feat, pe, x32 = pos
        _req_cuda(feat, pe, x32)
        assert feat.dtype == xb.dtype and feat.shape == (R, 256) and feat.stride(1) == 1 and pe.dtype == torch.float32 and pe.shape[1] == 256 and pe.is_contiguous()
        assert x32.dtype == torch.float32 and x32.shape[0] == R and x32.stride(1) == 1 and x32.shape[1] >= 256
        em.pe_feat, em.pe, em.pe_ld, em.pe_hw = feat.data_ptr(), pe.data_ptr(), feat.stride(0), pe.shape[0]
    _fill_emit_blocks(em, blocks, R, xb.dtype)
    with _Timed("token_mlp", 2.0 * sum(max(0, min(b[3], R) - b[2]) for b in blocks) * 256 * 256):
        check(lib.gim_token_mlp_emit(None, _p(xb), _p(x32), None, None, None, None, R, 256, 0, 0, 0, xb.stride(0),
                                     x32.stride(0) if x32 is not None else 0, 0.0, gim_dtype(xb), ctypes.byref(em), _stream()), "gim_token_mlp_emit")


def _fill_emit_blocks(em, blocks, R, dtype):
    """block descriptors of a gim_token_emit (see token_mlp); returns the flops of the blocks"""
    flops = 0.0
    fused_v = False
    for b, blk in enumerate(blocks):
        out, act, lo, hi = blk[:4]
        if len(blk) > 4:      # K of a fused pair
            ws, nb_kv, nchunk, tile0, src_len = blk[4]
            _req_cuda(ws)
            assert ws.dtype == torch.float32 and ws.is_contiguous() and b + 1 < len(blocks) and len(blocks[b + 1]) == 4
            assert hi <= R and lo % 64 == 0 and hi % 64 == 0 and tile0 + (hi - lo) // 64 <= nb_kv * nchunk, "token_mlp: fused KV state: tile range"
            state = nb_kv * 8 * (32 * 32 + 32)
            assert ws.numel() >= state * (nchunk + 1), "token_mlp: KV-state workspace too small (kv_state_workspace)"
            em.kv_part[b], em.kv_nchunk[b], em.kv_tile0[b], em.kv_len[b] = ws.data_ptr() + 4 * state, nchunk, tile0, float(src_len)
            fused_v = True
        elif fused_v:         # V of the pair
            fused_v = False
        else:
            _req_cuda(out)
            assert out.dtype == dtype and out.stride(1) == 1 and out.shape[0] == R and out.shape[1] >= 256
            em.out[b], em.ld[b] = out.data_ptr(), out.stride(0)
        em.act[b], em.row_lo[b], em.row_hi[b] = act, lo, hi
        flops += 2.0 * max(0, min(hi, R) - lo) * 256 * 256
    return flops


def kv_state_workspace(nb_kv, nchunk, device, H=8, D=32):
    """fp32 workspace [state nb_kv x H x (D D + D)][partials nb_kv x H x nchunk x (D D + D)] for partial states written by token_mlp's
    fused (k, v) pairs (gim_linear_attention_ws_bytes_chunks)"""
    return torch.empty(lib.gim_linear_attention_ws_bytes_chunks(nb_kv, H, D, nchunk) // 4, dtype=torch.float32, device=device)


def kv_state_finalize(ws, nb_kv, nchunk, H=8, D=32):
    """state = sum of the partials (gim_linear_attention_finalize); afterwards `ws` is what token_mlp takes as `kv`"""
    _req_cuda(ws)
    assert ws.dtype == torch.float32 and ws.numel() * 4 >= lib.gim_linear_attention_ws_bytes_chunks(nb_kv, H, D, nchunk)
    check(lib.gim_linear_attention_finalize(_p(ws), nb_kv, H, D, nchunk, _stream()), "gim_linear_attention_finalize")
    return ws


def fine_fused(feat_f0, feat_f1, b_ids, i_ids, j_ids, mkpts1_c, scale1, weights, ln_params, M, w0c, w1c, stride, W,
               scale, ln_eps, has_scale0, debug=False, count=None):
    """Whole fine level in one launch (bf16 fine maps).  Returns (expec_f [M,3], mkpts1_f [M,2], fine0, fine1) where
    fine0/fine1 are fp32 [M, W*W, C] dumps of the transformer output when `debug`, else None.
    `count` (device int32 tensor): M is the CAPACITY of the match lists and the kernel processes the first min(M, count[0]) matches --
    the launch does not wait for the host to learn the count (gim_fine_fused_dev); rows beyond it are left unwritten."""
    _req_cuda(feat_f0, feat_f1, b_ids, mkpts1_c, weights, ln_params, count)
    assert feat_f0.dtype in HALF and feat_f1.dtype == feat_f0.dtype and weights.dtype == feat_f0.dtype
    assert feat_f0.is_contiguous() and feat_f1.is_contiguous()
    _, hf0, wf0, C = feat_f0.shape
    _, hf1, wf1, _ = feat_f1.shape
    dev = feat_f0.device
    expec = torch.empty(M, 3, dtype=torch.float32, device=dev)
    mk1 = torch.empty(M, 2, dtype=torch.float32, device=dev)
    geom = (hf0, wf0, hf1, wf1, C, C, w0c, w1c, stride, W, scale, ln_eps, 1 if has_scale0 else 0, gim_dtype(feat_f0), _stream())
    if count is not None:
        assert not debug and count.dtype == torch.int32 and b_ids.numel() >= M
        with _Timed("fine_fused", 0.0):   # the caller fills in the flops once it knows the count (patch_last_fused_flops)
            check(lib.gim_fine_fused_dev(_p(feat_f0), _p(feat_f1), _p(b_ids), _p(i_ids), _p(j_ids), _p(mkpts1_c), _p(scale1), _p(weights),
                                         _p(ln_params), _p(expec), _p(mk1), M, _p(count), *geom), "gim_fine_fused_dev")
        return expec, mk1, None, None
    d0 = torch.empty(M, W * W, C, dtype=torch.float32, device=dev) if debug else None
    d1 = torch.empty(M, W * W, C, dtype=torch.float32, device=dev) if debug else None
    assert weights.numel() * weights.element_size() == lib.gim_fine_fused_weight_bytes()
    with _Timed("fine_fused", 33.6e6 * M):   # 33.6 MFLOP per match
        check(lib.gim_fine_fused(_p(feat_f0), _p(feat_f1), _p(b_ids), _p(i_ids), _p(j_ids), _p(mkpts1_c), _p(scale1), _p(weights),
                                 _p(ln_params), _p(expec), _p(mk1), _p(d0), _p(d1), M, *geom), "gim_fine_fused")
    return expec, mk1, d0, d1


# ---- gim_lightglue: SuperPoint glue -----------------------------------------------------------------------
def maxpool2x2(x):
    """x [B,H,W,C] NHWC -> new [B,H/2,W/2,C]"""
    _req_cuda(x)
    B, H, W, C = x.shape
    y = torch.empty(B, H // 2, W // 2, C, dtype=x.dtype, device=x.device)
    check(lib.gim_maxpool2x2(_p(x), _p(y), B, H, W, C, C, C, gim_dtype(x), _stream()), "gim_maxpool2x2")
    return y


def sp_scores(logits, B, h, w):
    """logits rows [B*h*w, >=65] -> scores [B, 8h, 8w] fp32"""
    _req_cuda(logits)
    out = torch.empty(B, 8 * h, 8 * w, dtype=torch.float32, device=logits.device)
    check(lib.gim_sp_scores(_p(logits), _p(out), B, h, w, logits.stride(0), gim_dtype(logits), _stream()), "gim_sp_scores")
    return out


def sp_nms(scores, radius, border):
    """scores [B,H,W] fp32 -> new [B,H,W]: kept maxima keep their score, others 0, border -1"""
    _req_cuda(scores)
    assert scores.dtype == torch.float32 and scores.is_contiguous()
    B, H, W = scores.shape
    ws = torch.empty(lib.gim_sp_nms_ws_bytes(B, H, W), dtype=torch.uint8, device=scores.device)
    out = torch.empty_like(scores)
    check(lib.gim_sp_nms(_p(scores), _p(out), _p(ws), B, H, W, radius, border, _stream()), "gim_sp_nms")
    return out


def sp_topk(nms_scores, k, thr):
    """-> (kpts [B,k,2] (x,y) fp32, kscores [B,k], nvalid [B] int32 device)"""
    _req_cuda(nms_scores)
    B, H, W = nms_scores.shape
    dev = nms_scores.device
    ws = torch.empty(lib.gim_sp_topk_ws_bytes(B, H, W), dtype=torch.uint8, device=dev)
    kpts = torch.empty(B, k, 2, dtype=torch.float32, device=dev)
    ksc = torch.empty(B, k, dtype=torch.float32, device=dev)
    nv = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.gim_sp_topk(_p(nms_scores), _p(ws), _p(kpts), _p(ksc), _p(nv), B, H, W, k, thr, _stream()), "gim_sp_topk")
    return kpts, ksc, nv


def sp_sample_desc(dense, kpts, h, w, out_f32, out_t, cell=8):
    """dense rows [B*h*w, >=256]; kpts [B,K,2]; out_f32 / out_t row views [B*K, >=256] (either may be None)"""
    _req_cuda(dense, kpts, out_f32, out_t)
    B, K, _ = kpts.shape
    check(lib.gim_sp_sample_desc(_p(dense), _p(kpts), _p(out_f32), _p(out_t), B, K, h, w, 256, dense.stride(0),
                                 out_f32.stride(0) if out_f32 is not None else 4,
                                 out_t.stride(0) if out_t is not None else 4, cell, gim_dtype(dense), _stream()),
          "gim_sp_sample_desc")


# ---- gim_lightglue: matcher -------------------------------------------------------------------------------
def lg_posenc(kpts, size_wh, Wr):
    """kpts [B,K,2], size_wh [B,2] fp32 device, Wr [32,2] -> enc [B*K, 64] (cos | sin)"""
    _req_cuda(kpts, size_wh, Wr)
    B, K, _ = kpts.shape
    enc = torch.empty(B * K, 64, dtype=torch.float32, device=kpts.device)
    check(lib.gim_lg_posenc(_p(kpts), _p(size_wh), _p(Wr), _p(enc), B, K, _stream()), "gim_lg_posenc")
    return enc


def lg_rotary(x, enc, ncols):
    """in place on columns [0, ncols) of the row view x"""
    _req_cuda(x, enc)
    check(lib.gim_lg_rotary(_p(x), _p(enc), x.shape[0], ncols, x.stride(0), gim_dtype(x), _stream()), "gim_lg_rotary")


def lg_transpose(src, dst, nb, S, Sp, C, lens=None):
    """src row view [nb*S, >=C] -> dst [nb, C, Sp] (same dtype); lens: int32 [nb] device, keys per sequence (columns behind them zero)"""
    _req_cuda(src, dst, lens)
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() == nb and lens.is_contiguous()
        check(lib.gim_lg_transpose_varlen(_p(src), _p(dst), _p(lens), nb, S, Sp, C, src.stride(0), gim_dtype(src), _stream()),
              "gim_lg_transpose_varlen")
        return
    check(lib.gim_lg_transpose(_p(src), _p(dst), nb, S, Sp, C, src.stride(0), gim_dtype(src), _stream()), "gim_lg_transpose")


def sdpa(q, k, vt, out, nb, H, L, S, Sp, kv_shift=0, D=64, len_q=None, len_k=None):
    """q row view [nb*L, ..], k row view [nb*S, ..], vt [nb, H*D, Sp], out row view [nb*L, ..]; head dim D in {64, 128}.
    len_q / len_k: int32 [nb] device (both or neither) -- sequence s has len_q[s] of its L queries and attends to len_k[kvseq] keys"""
    _req_cuda(q, k, vt, out, len_q, len_k)
    assert q.dtype == k.dtype == vt.dtype
    assert (len_q is None) == (len_k is None)
    # one 16-bit kind per call (the library routes by it): out is fp32 or of q's kind -- or anything, next to fp32 operands
    assert torch.float32 in (q.dtype, out.dtype) or out.dtype == q.dtype, f"sdpa: {q.dtype} operands with a {out.dtype} output"
    if len_q is not None:
        assert len_q.dtype == len_k.dtype == torch.int32 and len_q.numel() == len_k.numel() == nb
        check(lib.gim_sdpa_varlen(_p(q), _p(k), _p(vt), _p(out), _p(len_q), _p(len_k), nb, H, L, S, Sp, D, q.stride(0), k.stride(0),
                                  out.stride(0), kv_shift, gim_dtype(q), gim_dtype(out), _stream()), "gim_sdpa_varlen")
        return
    check(lib.gim_sdpa(_p(q), _p(k), _p(vt), _p(out), nb, H, L, S, Sp, D, q.stride(0), k.stride(0), out.stride(0),
                       kv_shift, gim_dtype(q), gim_dtype(out), _stream()), "gim_sdpa")


def layernorm_act(x, gamma, beta, out, act=ACT_NONE, eps=1e-5):
    """x fp32 row view [R, C] -> out row view (fp32 / bf16)"""
    _req_cuda(x, gamma, beta, out)
    R, C = x.shape
    check(lib.gim_layernorm_act(_p(x), _p(gamma), _p(beta), _p(out), R, C, x.stride(0), out.stride(0), act,
                                gim_dtype(out), eps, _stream()), "gim_layernorm_act")


def cast_rows(src, dst):
    """fp32 row view -> dst row view of the same shape (fp32 / bf16)"""
    _req_cuda(src, dst)
    R, C = src.shape
    check(lib.gim_cast_rows(_p(src), _p(dst), R, C, src.stride(0), dst.stride(0), gim_dtype(dst), _stream()), "gim_cast_rows")


class AssignResult:
    __slots__ = ("args", "ws", "matches0", "matches1", "mscores0", "mscores1", "pos", "count", "keep", "ragged")


def lg_assign(desc0, desc1, md0, md1, match_w, match_b, threshold, len0=None, len1=None):
    """desc0 [B,M,256] / desc1 [B,N,256] fp32 (row stride 256), md0/md1 = final_proj outputs (contiguous).
    len0 / len1: int32 [B] device (both or neither) -- pair b has len0[b] of its M rows and len1[b] of its N columns."""
    _req_cuda(desc0, desc1, md0, md1, match_w, match_b, len0, len1)
    assert (len0 is None) == (len1 is None)
    B, M, C = md0.shape
    N = md1.shape[1]
    dev = md0.device
    assert md0.is_contiguous() and md1.is_contiguous() and md0.dtype == torch.float32
    assert desc0.dtype == torch.float32 and desc0.stride(-1) == 1 and desc0.stride(-2) == desc1.stride(-2)
    r = AssignResult()
    r.ws = torch.empty(lib.gim_lg_assign_ws_bytes(B, M, N, C), dtype=torch.uint8, device=dev)
    r.matches0 = torch.empty(B, M, dtype=torch.int64, device=dev)
    r.matches1 = torch.empty(B, N, dtype=torch.int64, device=dev)
    r.mscores0 = torch.empty(B, M, dtype=torch.float32, device=dev)
    r.mscores1 = torch.empty(B, N, dtype=torch.float32, device=dev)
    r.pos = torch.empty(B, M, dtype=torch.int32, device=dev)
    r.count = torch.empty(B, dtype=torch.int32, device=dev)
    r.keep = (desc0, desc1, md0, md1, match_w, match_b, len0, len1)
    r.ragged = len0 is not None
    a = _lib.LgAssignArgs()
    a.desc0, a.desc1, a.md0, a.md1 = desc0.data_ptr(), desc1.data_ptr(), md0.data_ptr(), md1.data_ptr()
    a.match_w, a.match_b, a.ws = match_w.data_ptr(), match_b.data_ptr(), r.ws.data_ptr()
    a.matches0, a.matches1 = r.matches0.data_ptr(), r.matches1.data_ptr()
    a.mscores0, a.mscores1 = r.mscores0.data_ptr(), r.mscores1.data_ptr()
    a.pos, a.count = r.pos.data_ptr(), r.count.data_ptr()
    a.B, a.M, a.N, a.C, a.ld_desc, a.threshold = B, M, N, C, desc0.stride(-2), threshold
    r.args = a
    if r.ragged:
        assert len0.dtype == len1.dtype == torch.int32 and len0.numel() == len1.numel() == B
        check(lib.gim_lg_assign_ragged(ctypes.byref(a), _p(len0), _p(len1), _stream()), "gim_lg_assign_ragged")
    else:
        check(lib.gim_lg_assign(ctypes.byref(a), _stream()), "gim_lg_assign")
    return r


def lg_log_assignment(r):
    """Materialise log_assignment [B, M+1, N+1] from a previous lg_assign call's inputs."""
    a = r.args
    if getattr(r, "ragged", False):
        raise _lib.GimHipError("log_assignment is not built for a ragged batch: call forward() on the pair alone")
    out = torch.empty(a.B, a.M + 1, a.N + 1, dtype=torch.float32, device=r.count.device)
    check(lib.gim_lg_log_assignment(ctypes.byref(a), _p(out), _stream()), "gim_lg_log_assignment")
    return out


def lg_emit_matches(r, total, kpts0=None, kpts1=None, scale0=None, scale1=None):
    """Packs the match lists of all pairs (torch.where order).  Returns (matches [total,2] int64, scores [total],
    mkpts0 [total,2] | None, mkpts1, m_bids)."""
    a = r.args
    dev = r.count.device
    matches = torch.empty(total, 2, dtype=torch.int64, device=dev)
    scores = torch.empty(total, dtype=torch.float32, device=dev)
    adapter = kpts0 is not None
    mk0 = torch.empty(total, 2, dtype=torch.float32, device=dev) if adapter else None
    mk1 = torch.empty(total, 2, dtype=torch.float32, device=dev) if adapter else None
    bids = torch.empty(total, dtype=torch.int64, device=dev) if adapter else None
    if total > 0:
        _req_cuda(kpts0, kpts1, scale0, scale1)
        check(lib.gim_lg_emit_matches(_p(r.matches0), _p(r.mscores0), _p(r.pos), _p(r.count), _p(kpts0), _p(kpts1),
                                      _p(scale0), _p(scale1), _p(matches), _p(scores), _p(mk0), _p(mk1), _p(bids),
                                      a.B, a.M, a.N, _stream()), "gim_lg_emit_matches")
    return matches, scores, mk0, mk1, bids


# ---- gim_lightglue: keypoint bank (csrc/lg_bank.hip) ---------------------------------------------------------
def lg_bank_put(kpts, desc, size_wh, Wr, slots, bank_kpts, bank_desc, bank_enc):
    """kpts [n,K,2] fp32, desc [n,K,256] fp32 | None, size_wh [n,2] (w, h) | None, Wr [32,2] | None, slots int32 [n] (device) -> the bank
    arrays bank_kpts [S,K,2] | None, bank_desc [S,K,256] fp32 / fp16, bank_enc [S,K,64]; a None part is left untouched"""
    _req_cuda(kpts, desc, size_wh, Wr, slots, bank_kpts, bank_desc, bank_enc)
    n, K, _ = kpts.shape
    assert kpts.dtype == torch.float32 and kpts.is_contiguous() and slots.dtype == torch.int32 and slots.numel() == n
    assert desc is None or (desc.dtype == torch.float32 and desc.is_contiguous() and desc.shape == (n, K, 256))
    assert bank_desc.is_contiguous() and bank_enc.is_contiguous() and bank_desc.shape[1:] == (K, 256) and bank_enc.shape[1:] == (K, 64)
    check(lib.gim_lg_bank_put(_p(kpts), _p(desc), _p(size_wh), _p(Wr), _p(slots), _p(bank_kpts), _p(bank_desc), _p(bank_enc), n, K,
                              bank_desc.shape[0], gim_dtype(bank_desc), _stream()), "gim_lg_bank_put")


def lg_gather_pairs(bank_desc, bank_enc, idx0, idx1, X32, CAT, enc):
    """bank slots idx0[b] / idx1[b] (int32 device, [B]) -> X32 [2BK, >=256] fp32 row view, CAT [2BK, >=256] 16-bit row view (None in fp32
    mode, where X32 is CAT[:, :256] itself) and enc [2BK, 64]"""
    _req_cuda(bank_desc, bank_enc, idx0, idx1, X32, CAT, enc)
    B, K = idx0.numel(), bank_desc.shape[1]
    assert idx0.dtype == torch.int32 and idx1.dtype == torch.int32 and idx1.numel() == B
    assert X32.dtype == torch.float32 and X32.shape[0] == 2 * B * K and enc.is_contiguous() and enc.shape == (2 * B * K, 64)
    check(lib.gim_lg_gather_pairs(_p(bank_desc), _p(bank_enc), _p(idx0), _p(idx1), _p(X32), _p(CAT), _p(enc), B, K, bank_desc.shape[0],
                                  gim_dtype(bank_desc), gim_dtype(CAT) if CAT is not None else GIM_F32, X32.stride(0),
                                  CAT.stride(0) if CAT is not None else 0, _stream()), "gim_lg_gather_pairs")


def lg_gather_pairs_ragged(bank_desc, bank_enc, counts, idx0, idx1, X32, CAT, enc):
    """lg_gather_pairs for a bank whose slot s holds counts[s] (int32 [S], device) keypoints: rows behind an image's count are zero.
    Returns (len0, len1), int32 [B] device: the counts of the images named by idx0 / idx1."""
    _req_cuda(bank_desc, bank_enc, counts, idx0, idx1, X32, CAT, enc)
    B, K = idx0.numel(), bank_desc.shape[1]
    assert idx0.dtype == torch.int32 and idx1.dtype == torch.int32 and idx1.numel() == B
    assert counts.dtype == torch.int32 and counts.numel() == bank_desc.shape[0] and counts.is_contiguous()
    assert X32.dtype == torch.float32 and X32.shape[0] == 2 * B * K and enc.is_contiguous() and enc.shape == (2 * B * K, 64)
    len0 = torch.empty(B, dtype=torch.int32, device=idx0.device)
    len1 = torch.empty(B, dtype=torch.int32, device=idx0.device)
    check(lib.gim_lg_gather_pairs_ragged(_p(bank_desc), _p(bank_enc), _p(idx0), _p(idx1), _p(counts), _p(X32), _p(CAT), _p(enc), _p(len0),
                                         _p(len1), B, K, bank_desc.shape[0], gim_dtype(bank_desc),
                                         gim_dtype(CAT) if CAT is not None else GIM_F32, X32.stride(0),
                                         CAT.stride(0) if CAT is not None else 0, _stream()), "gim_lg_gather_pairs_ragged")
    return len0, len1


def lg_emit_hloc(r):
    """an lg_assign result -> (matches0 int16 [B,M], matching_scores0 fp16 [B,M]): hloc's match-file datasets for the whole batch"""
    B, M = r.matches0.shape
    if M > 32767:
        raise _lib.GimHipError(f"hloc stores matches0 as int16: {M} keypoints per image do not fit (at most 32767)")
    m16 = torch.empty(B, M, dtype=torch.int16, device=r.matches0.device)
    s16 = torch.empty(B, M, dtype=torch.float16, device=r.matches0.device)
    check(lib.gim_lg_emit_hloc(_p(r.matches0), _p(r.mscores0), _p(m16), _p(s16), B, M, _stream()), "gim_lg_emit_hloc")
    return m16, s16


# ---- gim_dkm -------------------------------------------------------------------------------------------------
def maxpool3x3s2(x):
    """x [B,H,W,C] NHWC -> new [B,(H-1)//2+1,(W-1)//2+1,C] (kernel 3, stride 2, padding 1)"""
    _req_cuda(x)
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=x.dtype, device=x.device)
    check(lib.gim_maxpool3x3s2(_p(x), _p(y), B, H, W, C, C, C, gim_dtype(x), _stream()), "gim_maxpool3x3s2")
    return y


def resize_bilinear(x, size, out_dtype=None):
    """x [B,h,w,C] NHWC contiguous -> new [B,Ho,Wo,C] (bilinear, align_corners=False)"""
    _req_cuda(x)
    B, h, w, C = x.shape
    y = torch.empty(B, size[0], size[1], C, dtype=out_dtype or x.dtype, device=x.device)
    check(lib.gim_resize_bilinear(_p(x), _p(y), B, h, w, size[0], size[1], C, C, C, gim_dtype(x), gim_dtype(y), _stream()),
          "gim_resize_bilinear")
    return y


def resize_image(img, dst, b_off=0):
    """img [B,C,h,w] fp32 NCHW -> dst[b_off:b_off+B] ([.,Ho,Wo,cpad] NHWC), bilinear align_corners=False"""
    _req_cuda(img, dst)
    B, C, h, w = img.shape
    check(lib.gim_resize_image(_p(img), _p(dst), B, C, h, w, dst.shape[1], dst.shape[2], dst.shape[3], b_off, gim_dtype(dst),
                               _stream()), "gim_resize_image")


def grid_sample(feat, grid, out):
    """feat [B,h,w,C]; grid [B,Ho,Wo,2] fp32; out: row view [B*Ho*Wo, >=C] (may be a channel slice)"""
    _req_cuda(feat, grid, out)
    B, h, w, C = feat.shape
    check(lib.gim_grid_sample(_p(feat), _p(grid), _p(out), B, h, w, grid.shape[1], grid.shape[2], C, C, out.stride(0),
                              gim_dtype(feat), _stream()), "gim_grid_sample")


def dkm_disp_emb(flow, wgt, bias, out):
    """flow [B,h,w,2] fp32; wgt [E,2], bias [E] fp32; out row view [B*h*w, >=E]"""
    _req_cuda(flow, wgt, bias, out)
    B, h, w, _ = flow.shape
    check(lib.gim_dkm_disp_emb(_p(flow), _p(wgt), _p(bias), _p(out), B, h, w, wgt.shape[0], out.stride(0), gim_dtype(out),
                               _stream()), "gim_dkm_disp_emb")


def local_corr(f0, f1, flow, r, out):
    """f0, f1 [B,h,w,C] (C = valid channels, row stride = shape[-1]); out row view [B*h*w, >=(2r+1)^2]"""
    _req_cuda(f0, f1, flow, out)
    B, h, w, C = f0.shape
    check(lib.gim_local_corr(_p(f0), _p(f1), _p(flow), _p(out), B, h, w, C, r, f0.stride(2), f1.stride(2), out.stride(0),
                             gim_dtype(f0), gim_dtype(out), _stream()), "gim_local_corr")


def dwconv5x5_bn_relu(x, wgt, scale, shift, cin, cout):
    """x [B,H,W,ldx]; wgt [25,cpad], scale/shift [cpad] fp32 -> new [B,H,W,cpad]"""
    _req_cuda(x, wgt, scale, shift)
    B, H, W, ldx = x.shape
    cpad = wgt.shape[1]
    y = torch.empty(B, H, W, cpad, dtype=x.dtype, device=x.device)
    check(lib.gim_dwconv5x5_bn_relu(_p(x), _p(wgt), _p(scale), _p(shift), _p(y), B, H, W, cin, cout, cpad, ldx, cpad,
                                    gim_dtype(x), _stream()), "gim_dwconv5x5_bn_relu")
    return y


def dwconv5x5_pw(x, wgt, scale, shift, pw_w, pw_b):
    """One ConvRefiner block in one launch (gim_dwconv5x5_pw): x [B,H,W,cs] 16-bit with cs = 144 (or 24 / 32) stored channels -> y [B,H,W,cs] =
    conv1x1(relu(bn(dwconv5x5(x)))) + bias; wgt [25, cs], scale / shift [cs] fp32 as for dwconv5x5_bn_relu; pw_w [NP, KP] in x's dtype, pw_b [NP] fp32
    (NP, KP = 160, 144 for cs = 144; 32, 32 for cs = 24 / 32)."""
    _req_cuda(x, wgt, scale, shift, pw_w, pw_b)
    B, H, W, cs = x.shape
    npc, kp = (160, 144) if cs == 144 else (32, 32)
    assert x.dtype in HALF and x.is_contiguous() and cs in (24, 32, 144) and pw_w.dtype == x.dtype and tuple(pw_w.shape) == (npc, kp) and pw_b.numel() == npc
    assert wgt.shape == (25, cs) and scale.numel() == cs and shift.numel() == cs
    y = torch.empty(B, H, W, cs, dtype=x.dtype, device=x.device)
    check(lib.gim_dwconv5x5_pw(_p(x), _p(wgt), _p(scale), _p(shift), _p(pw_w), _p(pw_b), _p(y), B, H, W, cs, cs, cs, gim_dtype(x), _stream()), "gim_dwconv5x5_pw")
    return y


def row_norms(x, C):
    """x row view [R, >=C] -> [R] fp32 L2 norms"""
    _req_cuda(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(lib.gim_row_norms(_p(x), _p(out), x.shape[0], C, x.stride(0), gim_dtype(x), _stream()), "gim_row_norms")
    return out


def cos_kernel_finish(k, nx, ny, B, n, m, T, eps, diag_add):
    """k: fp32 dot products, rows [B*n, ld]; in place -> exp((k / (nx ny + eps) - 1) / T) (+ diag_add on i == j)"""
    _req_cuda(k, nx, ny)
    check(lib.gim_cos_kernel_finish(_p(k), _p(nx), _p(ny), B, n, m, k.stride(0), T, eps, diag_add, _stream()), "gim_cos_kernel_finish")


def gp_solve(K, F, npad):
    """K [B,n,ld] fp32 (SPD, sigma on the diagonal), F [B,n,nrhs] fp32 -> Xt [B,nrhs,npad] fp32 = (K^-1 F)^T, zero padded.  B <= 16.
    A batch entry whose Cholesky factorisation fails (a pivot that is not positive: K[b] not positive definite, or holding NaN / overflowed
    values) comes back with EVERY element of Xt[b] quiet NaN, the padding columns included; the other entries are unaffected.  Nothing is
    raised for it (the call does not wait for the device): test the result with isnan / isfinite."""
    _req_cuda(K, F)
    B, n, ld = K.shape
    nrhs = F.shape[2]
    assert K.is_contiguous() and F.is_contiguous() and K.dtype == torch.float32 and F.dtype == torch.float32
    ws = torch.empty(lib.gim_gp_solve_ws_bytes(B, n, nrhs), dtype=torch.uint8, device=K.device)
    Xt = torch.empty(B, nrhs, npad, dtype=torch.float32, device=K.device)
    check(lib.gim_gp_solve(_p(K), _p(F), _p(Xt), _p(ws), B, n, ld, nrhs, npad, _stream()), "gim_gp_solve")
    return Xt


def gp_posterior_f64(X, Y, F, out, T=0.2, eps=1e-6, sigma=0.1):
    """GP posterior mean, every step in fp64 (the dense matchers' parity mode): X / Y [B,n,d] fp32 query / support rows (contiguous),
    F [n,nrhs] fp32 -> out: fp32 row view [B*n, >= nrhs] receives K_xy (K_yy + sigma I)^-1 F, K = exp((cos - 1) / T).  B <= 16.
    A direction b whose K_yy + sigma I fails to factor (NaN or overflowed rows in Y[b]) has all n x nrhs elements of its block of `out`
    written as quiet NaN; the other directions are unaffected and the columns of `out` beyond nrhs are never written."""
    _req_cuda(X, Y, F, out)
    B, n, d = X.shape
    nrhs = F.shape[1]
    assert X.is_contiguous() and Y.is_contiguous() and F.is_contiguous() and Y.shape == X.shape and F.shape[0] == n
    assert X.dtype == Y.dtype == F.dtype == out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] >= B * n and out.shape[1] >= nrhs
    ws = torch.empty(lib.gim_gp_posterior_f64_ws_bytes(B, n, d, nrhs), dtype=torch.uint8, device=X.device)
    check(lib.gim_gp_posterior_f64(_p(X), _p(Y), _p(F), _p(out), _p(ws), B, n, d, d, nrhs, out.stride(0), T, eps, sigma, _stream()),
          "gim_gp_posterior_f64")


def global_avgpool(x, out, c_off):
    """x [B,h,w,C] -> out[b, c_off:c_off+C] (fp32 [B, ldo])"""
    _req_cuda(x, out)
    B, h, w, C = x.shape
    check(lib.gim_global_avgpool(_p(x), _p(out), B, h * w, C, C, out.stride(0), c_off, gim_dtype(x), _stream()), "gim_global_avgpool")


def cab_scale_add(g, x1, x2):
    """sigmoid(g[b,c]) * x2 + x1 (x1 may be None = zeros); x2 [B,h,w,C] -> new tensor"""
    _req_cuda(g, x1, x2)
    B, h, w, C = x2.shape
    out = torch.empty_like(x2)
    check(lib.gim_cab_scale_add(_p(g), _p(x1), _p(x2), _p(out), B, h * w, C, g.stride(0), C, C, C, gim_dtype(x2), _stream()),
          "gim_cab_scale_add")
    return out


def dkm_flow_update(flow, cert, d, sx, sy, cert_init=False, roma_layout=False):
    """flow [B,h,w,2], cert [B,h,w,1] fp32 updated in place from d rows [B*h*w, >=3] = [dcert, dx, dy] (DKM) or
    [dx, dy, dcert] (RoMa, roma.py:579)"""
    _req_cuda(flow, cert, d)
    check(lib.gim_dkm_flow_update(_p(flow), _p(cert), _p(d), flow.numel() // 2, d.stride(0), sx, sy,
                                  (1 if cert_init else 0) | (2 if roma_layout else 0), gim_dtype(d), _stream()), "gim_dkm_flow_update")


def dkm_grid_coords(B, h, w, device):
    flow = torch.empty(B, h, w, 2, dtype=torch.float32, device=device)
    check(lib.gim_dkm_grid_coords(_p(flow), B, h, w, _stream()), "gim_dkm_grid_coords")
    return flow


def dkm_black_mask(im, size):
    """im [1,3,h,w] fp32 NCHW -> uint8 [Ho,Wo]"""
    _req_cuda(im)
    m = torch.empty(size[0], size[1], dtype=torch.uint8, device=im.device)
    check(lib.gim_dkm_black_mask(_p(im), _p(m), im.shape[2], im.shape[3], size[0], size[1], _stream()), "gim_dkm_black_mask")
    return m


def dkm_match_post(flow, cert, low, black0, black1, warp, certainty):
    """flow (f0, f1) [H,W,2], cert / low (c0, c1) [H,W,1] of the two directions -> warp [H,2W,4], certainty [H,2W] (written in place)"""
    _req_cuda(flow[0], cert[0], low[0], black0, black1, warp, certainty)
    H, W, _ = flow[0].shape
    for t in (*flow, *cert, *low, warp, certainty):
        assert t.is_contiguous()
    check(lib.gim_dkm_match_post(_p(flow[0]), _p(flow[1]), _p(cert[0]), _p(cert[1]), _p(low[0]), _p(low[1]), _p(black0), _p(black1),
                                 _p(warp), _p(certainty), H, W, _stream()), "gim_dkm_match_post")


class RowMatrixOperand:
    """A row buffer [N_alloc, K] used as the [N][K] "weight" operand of gim_conv2d_bn_act (same fields as
    packing.PackedConv): y[m, n] = sum_k x[m, k] * w[n, k].  N_alloc must cover n rounded up to 64 rows (rows past n
    only produce columns that are never stored) and K must be a multiple of the 128-byte K slab."""
    _ktabs = {}

    def __init__(self, w, n, k):
        from .packing import KTILE_BYTES, NPAD, elem_size, group_elems
        dt = gim_dtype(w)
        es, g = elem_size(dt), group_elems(dt)
        assert w.dim() == 2 and w.stride(1) == 1 and w.stride(0) == k and (k * es) % KTILE_BYTES == 0, (w.shape, w.stride(), k)
        self.npad = (n + NPAD - 1) // NPAD * NPAD
        assert w.shape[0] >= self.npad, f"operand needs {self.npad} allocated rows, has {w.shape[0]}"
        key = (k, dt, str(w.device))
        if key not in RowMatrixOperand._ktabs:
            nkt = k * es // KTILE_BYTES
            gi = torch.arange((nkt + 2) * 8, dtype=torch.int64) * g
            ent = torch.where(gi < k, gi, torch.full_like(gi, 0xFF000000))
            ent = torch.where(ent >= 2 ** 31, ent - 2 ** 32, ent).to(torch.int32)
            RowMatrixOperand._ktabs[key] = ent.to(w.device)
        self.w, self.bias, self.ktab = w, None, RowMatrixOperand._ktabs[key]
        self.kh = self.kw = 1
        self.stride, self.pad = 1, 0
        self.cin = self.cin_pad = k
        self.cout = n
        self.n_store = (n + 3) // 4 * 4 if dt == GIM_F32 else (n + 7) // 8 * 8
        self.kpad, self.dtype = k, dt


def matmul_nt(x, w_rows, n, y):
    """y[:, :n] = x @ w_rows[:n].T on the igemm (x: row view [M, >=K]; w_rows: [N_alloc, K] contiguous; y: row view)."""
    pk = RowMatrixOperand(w_rows, n, w_rows.shape[1])
    M = x.shape[0]
    conv_rows(x, pk, (1, 1, M, 1, M), y)


def kde(x, std, half=False):
    """x [n,4] fp32 contiguous -> density [n]; half: coordinates rounded to fp16 first (RoMa's kde, roma.py:1018-1023)"""
    _req_cuda(x)
    assert x.dim() == 2 and x.shape[1] == 4 and x.is_contiguous() and x.dtype == torch.float32
    d = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(lib.gim_kde(_p(x), _p(d), x.shape[0], -std if half else std, _stream()), "gim_kde")
    return d


def cls_to_flow(logits, B, h, w, ncls):
    """logits rows [B*h*w, >= ncls + 1] fp32 (64x64 anchor classes + certainty) -> (flow [B,h,w,2], certainty [B,h,w,1])"""
    _req_cuda(logits)
    flow = torch.empty(B, h, w, 2, dtype=torch.float32, device=logits.device)
    cert = torch.empty(B, h, w, 1, dtype=torch.float32, device=logits.device)
    check(lib.gim_cls_to_flow(_p(logits), _p(flow), _p(cert), B * h * w, ncls, logits.stride(0), _stream()), "gim_cls_to_flow")
    return flow, cert


def weighted_sample_ws_bytes(n):
    return lib.gim_weighted_sample_ws_bytes(n)


def weighted_sample(w, k, seed, ws=None, out=None):
    """k distinct indices drawn with probability ~ w (fp32 [n], >= k positive entries) -> int64 [k], unordered.
    ws: caller's workspace (contiguous, >= weighted_sample_ws_bytes(n) bytes; its first n 32-bit words are the keys after the
    call); out: caller's int64 [k] result buffer."""
    _req_cuda(w, ws, out)
    assert w.dim() == 1 and w.is_contiguous() and w.dtype == torch.float32
    n = w.shape[0]
    need = weighted_sample_ws_bytes(n)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=w.device)
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= need, (ws.shape, ws.dtype, need)
    if out is None:
        out = torch.empty(k, dtype=torch.int64, device=w.device)
    assert out.dtype == torch.int64 and out.shape == (k,) and out.is_contiguous(), (out.dtype, out.shape)
    check(lib.gim_weighted_sample(_p(w), _p(out), _p(ws), n, k, seed & 0xffffffff, _stream()), "gim_weighted_sample")
    return out


SAMPLE_MAX_PAIRS = 16    # GIM_SAMPLE_MAX_PAIRS of include/gim_hip.h


def balanced_sample_pairs_ws_bytes(B, n, num):
    return lib.gim_balanced_sample_pairs_ws_bytes(B, n, num)


def balanced_sample_pairs_layout(B, n, num):
    """the workspace of gim_balanced_sample_pairs as include/gim_hip.h documents it: region name -> (byte offset, dtype, shape),
    plus "bytes" -> the total.  `state` rows are int32 [16]: n_pos (as counted), k1, k2, then scratch."""
    npad, K1 = (n + 3) // 4 * 4, min(4 * num, n)
    nb1, nb2 = (n + 2047) // 2048, (K1 + 2047) // 2048
    out, off = {}, 0
    for name, dt, shape in (("keys1", torch.int32, (B, npad)), ("rows", torch.float32, (B, K1, 4)), ("rowcert", torch.float32, (B, K1)),
                            ("density", torch.float32, (B, K1)), ("keys2", torch.int32, (B, K1)), ("blocks1", torch.int32, (B, nb1, 2)),
                            ("blocks2", torch.int32, (B, nb2, 2)), ("hist", torch.int32, (B, 4096)), ("state", torch.int32, (B, 16))):
        out[name] = (off, dt, shape)
        off += (4 * math.prod(shape) + 255) // 256 * 256
    out["bytes"] = off
    return out


def balanced_sample_pairs_region(ws, B, n, num, name):
    """one region of a workspace `balanced_sample_pairs` has filled, as a tensor view (keys as int32 bit patterns)"""
    off, dt, shape = balanced_sample_pairs_layout(B, n, num)[name]
    return ws.view(torch.uint8).reshape(-1)[off:off + 4 * math.prod(shape)].view(dt).reshape(shape)


def balanced_sample_pairs(matches, cert, seeds, num, thresh, kde_half, ws=None, out=None):
    """`balanced_sample` of B pairs in one fixed launch sequence with no synchronisation (gim_balanced_sample_pairs): matches [B,n,4]
    (or [B,H,W2,4]) and cert [B,n] (or [B,H,W2]) fp32 contiguous, seeds: B pairs of ints (host) -> (sparse [B,num,4], mconf [B,num],
    count int32 [B]) on the device.  Pair b's first count[b] rows are what balanced_sample(matches[b], cert[b], num, ...) returns when
    its generator draws seeds[b], bit for bit and in its order; the rows behind them are zero.  1 <= B <= SAMPLE_MAX_PAIRS.
    ws: caller's workspace (uint8, >= balanced_sample_pairs_ws_bytes(B, n, num) bytes); out: caller's (sparse, mconf, count)."""
    _req_cuda(matches, cert, ws)
    for t, what in ((matches, "matches"), (cert, "certainty")):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.GimHipError(f"balanced_sample_pairs: {what} must be contiguous fp32, got {t.dtype}, strides {t.stride()}")
    B = cert.shape[0]
    n = cert[0].numel() if B else 0
    if cert.dim() < 2 or matches.shape != cert.shape + (4,) or not 1 <= B <= SAMPLE_MAX_PAIRS or n == 0:
        raise _lib.GimHipError(f"balanced_sample_pairs: matches {tuple(matches.shape)} / certainty {tuple(cert.shape)} "
                               f"(1 <= B <= {SAMPLE_MAX_PAIRS})")
    flat = [int(v) & 0xffffffff for pair in seeds for v in pair]
    if len(flat) != 2 * B or num < 1:
        raise _lib.GimHipError(f"balanced_sample_pairs: {len(flat)} seeds for {B} pairs, num = {num}")
    sd = (ctypes.c_uint32 * (2 * B))(*flat)
    need = balanced_sample_pairs_ws_bytes(B, n, num)
    dev = cert.device
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= need, (ws.shape, ws.dtype, need)
    if out is None:
        out = (torch.empty(B, num, 4, dtype=torch.float32, device=dev), torch.empty(B, num, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))
    sparse, mconf, count = out
    assert sparse.shape == (B, num, 4) and mconf.shape == (B, num) and count.shape == (B,)
    assert sparse.dtype == mconf.dtype == torch.float32 and count.dtype == torch.int32
    assert sparse.is_contiguous() and mconf.is_contiguous() and count.is_contiguous()
    check(lib.gim_balanced_sample_pairs(_p(matches), _p(cert), ctypes.cast(sd, ctypes.c_void_p), _p(sparse), _p(mconf), _p(count), _p(ws),
                                        B, n, int(num), float(thresh), int(bool(kde_half)), _stream()), "gim_balanced_sample_pairs")
    return sparse, mconf, count


def dense_to_pixels(matches, hw0, hw1):
    """matches [n,4] fp32 normalised -> (kpts0 [n,2], kpts1 [n,2]) in pixels of images of size hw0 / hw1 (h, w)"""
    _req_cuda(matches)
    n = matches.shape[0]
    m = matches.contiguous()
    k0 = torch.empty(n, 2, dtype=torch.float32, device=m.device)
    k1 = torch.empty(n, 2, dtype=torch.float32, device=m.device)
    if n == 0:
        return k0, k1
    check(lib.gim_dense_to_pixels(_p(m), _p(k0), _p(k1), n, float(hw0[1]), float(hw0[0]), float(hw1[1]), float(hw1[0]), _stream()),
          "gim_dense_to_pixels")
    return k0, k1


# ---- root_sift baseline ----------------------------------------------------------------------------------------
def nn_match(desc0, desc1, rootsift=False, ratio=0.8, count=None):
    """desc0 [n0,D], desc1 [n1,D] fp32 (D % 16 == 0, 16 <= D <= 256) -> (match0 int32 [n0]: index into desc1 or -1, score0 fp32 [n0]:
    the row maximum of desc0 @ desc1.T): mutual nearest neighbour + Lowe's ratio test (trainer/lightning.py:215-226) in one sweep of
    gim_nn_match; nothing of size n0 x n1 is allocated.  rootsift: rows -> sqrt(d / sum d) first.  ratio <= 0: no ratio test.
    count: optional int32 device tensor whose word [0] receives the number of matched rows (no host synchronisation here)."""
    _req_cuda(desc0, desc1, count)
    assert desc0.dim() == 2 and desc1.dim() == 2 and desc0.shape[1] == desc1.shape[1]
    assert desc0.dtype == torch.float32 and desc1.dtype == torch.float32
    desc0, desc1 = desc0.contiguous(), desc1.contiguous()
    n0, n1, D = desc0.shape[0], desc1.shape[0], desc0.shape[1]
    dev = desc0.device
    if count is None:
        count = torch.empty(1, dtype=torch.int32, device=dev)
    assert count.dtype == torch.int32 and count.numel() >= 1
    if n0 == 0 or n1 == 0:       # the library writes the count only
        match0 = torch.zeros(n0, dtype=torch.int32, device=dev) - 1
        score0 = torch.zeros(n0, dtype=torch.float32, device=dev)
        ws = None
    else:
        match0 = torch.empty(n0, dtype=torch.int32, device=dev)
        score0 = torch.empty(n0, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.gim_nn_match_ws_bytes(n0, n1, D, int(bool(rootsift))), dtype=torch.uint8, device=dev)
    with _Timed("nn_match", 2.0 * n0 * n1 * D):
        check(lib.gim_nn_match(_p(desc0), _p(desc1), n0, n1, D, int(bool(rootsift)), float(ratio), _p(match0), _p(score0), _p(count),
                               _p(ws), _stream()), "gim_nn_match")
    return match0, score0


def nn_bank_put(desc, slot, bank_desc, bank_n, rootsift=True):
    """one image's descriptors [n, D] fp32 (n == 0 allowed) -> slot `slot` of bank_desc [S, R, D] fp32, bank_n [S] int32 (its count), in
    one launch of gim_nn_bank_put.  rootsift: the stored rows are sqrt(d / sum d), bit-equal to what `nn_match` normalises per call."""
    _req_cuda(desc, bank_desc, bank_n)
    assert desc.dim() == 2 and bank_desc.dim() == 3 and desc.dtype == bank_desc.dtype == torch.float32 and bank_n.dtype == torch.int32
    assert bank_desc.is_contiguous() and bank_n.is_contiguous() and bank_n.numel() == bank_desc.shape[0]
    S, R, D = bank_desc.shape
    if desc.shape[1] != D:
        raise _lib.GimHipError(f"nn_bank_put: descriptors of width {desc.shape[1]} into a bank of width {D}")
    desc = desc.contiguous()
    check(lib.gim_nn_bank_put(_p(desc) if desc.shape[0] else None, int(desc.shape[0]), D, int(bool(rootsift)), int(slot), _p(bank_desc),
                              _p(bank_n), S, R, _stream()), "gim_nn_bank_put")


NnPairsPlan = collections.namedtuple("NnPairsPlan", "idx0 idx1 row_off col_off work nsplit")
NnPairsResult = collections.namedtuple("NnPairsResult", "match0 score0 count row_off matches0_i16 matching_scores0_f16")


def nn_pairs_plan(idx0, idx1, counts):
    """The host half of `nn_match_pairs` (gim_nn_match_pairs_plan; no device): slot pairs (idx0[p], idx1[p]) and the per-slot descriptor
    counts [S] -> NnPairsPlan of int32 numpy arrays: row_off / col_off [P + 1] (prefix sums of the counts of the pairs' sides), work
    [W, 4] = (pair, row block, first column tile, one past the last) and the batch's column split.  A slot outside [0, S) raises."""
    i0 = np.ascontiguousarray(np.asarray(idx0, dtype=np.int32).reshape(-1))
    i1 = np.ascontiguousarray(np.asarray(idx1, dtype=np.int32).reshape(-1))
    n = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(-1))
    if i0.shape != i1.shape:
        raise _lib.GimHipError(f"nn_match_pairs: {i0.shape[0]} first slots, {i1.shape[0]} second slots")
    P = i0.shape[0]
    row_off, col_off = np.zeros(P + 1, dtype=np.int32), np.zeros(P + 1, dtype=np.int32)
    nw, ns = ctypes.c_int32(0), ctypes.c_int32(0)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def plan(work):
        check(lib.gim_nn_match_pairs_plan(ptr(i0), ptr(i1), ptr(n), P, int(n.shape[0]), ptr(row_off), ptr(col_off),
                                          ptr(work) if work is not None else None, 0 if work is None else work.shape[0],
                                          ctypes.addressof(nw), ctypes.addressof(ns)), "gim_nn_match_pairs_plan")
    plan(None)                                      # counts the work items
    work = np.zeros((nw.value, 4), dtype=np.int32)
    if nw.value:
        plan(work)
    return NnPairsPlan(i0, i1, row_off, col_off, work, ns.value)


def _upload_i32(a, dev):
    return torch.from_numpy(a).to(dev)


def nn_match_pairs(bank_desc, bank_n, counts, idx0, idx1, ratio=0.8, hloc=False):
    """P pairs of bank slots in one launch sequence of gim_nn_match_pairs (reset, sweep over the work table, final) with no host
    synchronisation.  bank_desc [S, R, D] fp32 / bank_n [S] int32 as `nn_bank_put` filled them, counts: the HOST mirror of bank_n,
    idx0 / idx1: host sequences of slots.  -> NnPairsResult: ragged match0 int32 / score0 fp32 [row_off[P]] (pair p owns
    row_off[p]:row_off[p + 1]; bit-equal to `nn_match` on that pair), count int32 [P] on the device, row_off as a host array, and with
    `hloc` the same rows as hloc stores them: matches0_i16 int16, matching_scores0_f16 fp16 = (1 + score0) / 2 on matches, else 0."""
    _req_cuda(bank_desc, bank_n)
    assert bank_desc.dim() == 3 and bank_desc.dtype == torch.float32 and bank_desc.is_contiguous() and bank_n.dtype == torch.int32
    S, R, D = bank_desc.shape
    dev = bank_desc.device
    if hloc and R > 32767:
        raise _lib.GimHipError(f"nn_match_pairs: max_rows={R} descriptors do not fit hloc's int16 matches0 (at most 32767)")
    pl = nn_pairs_plan(idx0, idx1, counts)
    P, W = pl.idx0.shape[0], pl.work.shape[0]
    rows0, rows1 = int(pl.row_off[P]), int(pl.col_off[P])
    match0 = torch.empty(rows0, dtype=torch.int32, device=dev)
    score0 = torch.empty(rows0, dtype=torch.float32, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    m16 = torch.empty(rows0, dtype=torch.int16, device=dev) if hloc else None
    s16 = torch.empty(rows0, dtype=torch.float16, device=dev) if hloc else None
    if P == 0:
        return NnPairsResult(match0, score0, count, pl.row_off, m16, s16)
    # one upload: the index arrays, the offsets and the work table
    tab = _upload_i32(np.concatenate([pl.idx0, pl.idx1, pl.row_off, pl.col_off, pl.work.reshape(-1)]), dev)
    o = [0, P, 2 * P, 3 * P + 1, 4 * P + 2]
    i0, i1, ro, co, wk = (tab[o[k]:] for k in range(5))
    ws = torch.empty(lib.gim_nn_match_pairs_ws_bytes(rows0, rows1), dtype=torch.uint8, device=dev) if rows0 else None
    flops = 2.0 * D * float(np.sum((pl.row_off[1:] - pl.row_off[:-1]).astype(np.float64) * (pl.col_off[1:] - pl.col_off[:-1])))
    with _Timed("nn_match_pairs", flops):
        check(lib.gim_nn_match_pairs(_p(bank_desc), _p(bank_n), _p(i0), _p(i1), _p(ro), _p(co), _p(wk) if W else None, P, W, pl.nsplit,
                                     rows0, rows1, S, R, D, float(ratio), _p(match0), _p(score0), _p(count), int(bool(hloc)), _p(m16),
                                     _p(s16), _p(ws), _stream()), "gim_nn_match_pairs")
    return NnPairsResult(match0, score0, count, pl.row_off, m16, s16)


# ---- RANSAC hypothesis scoring (gim_amd/pose.py) -----------------------------------------------------------------
def _ransac_points(x0, x1, offsets, B):
    """checks of the point arguments shared by ransac_score / ransac_mask -> (offsets int32 [B + 1] on the device, Ptot)"""
    for t in (x0, x1):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous():
            raise _lib.GimHipError(f"ransac points must be contiguous fp64 [P, 2], got {t.dtype} {tuple(t.shape)}")
    if x0.shape != x1.shape or x0.device != x1.device:
        raise _lib.GimHipError("ransac points x0 and x1 differ in shape or device")
    P = x0.shape[0]
    if offsets is None:
        return torch.tensor([0, P], dtype=torch.int32, device=x0.device), P
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] != B + 1 or not offsets.is_contiguous() or offsets.device != x0.device:
        raise _lib.GimHipError(f"ransac offsets must be contiguous int32 [B + 1 = {B + 1}] on the points' device")
    # the kernels trust the offsets, so they are read back once here (B + 1 words; the callers wait for the counts anyway)
    o = offsets.tolist()
    if o[0] != 0 or o[-1] != P or any(a > b for a, b in zip(o, o[1:])):
        raise _lib.GimHipError(f"ransac offsets must rise from 0 to the point count {P}, got {o[:8]}{'...' if len(o) > 8 else ''}")
    return offsets, P


def _score_args(word, models, x0, x1, valid, offsets):
    """The checks of ransac_score / magsac_score on the models, the points and `valid`; `word` names the scorer in a refusal.
    -> (valid as uint8 or None, offsets int32 [B + 1] on the device, B, K, Ptot)"""
    _req_cuda(models, x0, x1, valid, offsets)
    single = offsets is None
    want = 3 if single else 4
    if models.dtype != torch.float64 or models.dim() != want or models.shape[-2:] != (3, 3) or not models.is_contiguous():
        raise _lib.GimHipError(f"{word} models must be contiguous fp64 {'[K,3,3]' if single else '[B,K,3,3]'}, got {models.dtype} {tuple(models.shape)}")
    B, K = (1, models.shape[0]) if single else models.shape[:2]
    offsets, P = _ransac_points(x0, x1, offsets, B)
    if models.device != x0.device:
        raise _lib.GimHipError(f"{word} models and points are on different devices")
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
        if valid.dtype != torch.uint8 or valid.shape != models.shape[:-2] or not valid.is_contiguous() or valid.device != x0.device:
            raise _lib.GimHipError(f"{word} valid must be contiguous bool / uint8 {tuple(models.shape[:-2])} on the models' device")
    return valid, offsets, B, K, P


def ransac_score(models, x0, x1, thr2, valid=None, offsets=None):
    """Inlier counts of candidate models over matched points (gim_ransac_score; fp64, the arithmetic of pose.sampson_error).
    One pair: models fp64 [K,3,3], x0 / x1 fp64 [P,2], valid bool / uint8 [K] or None -> int32 [K].
    B pairs: offsets int32 [B+1] (pair b owns the points offsets[b] .. offsets[b+1] of the concatenated x0 / x1), models [B,K,3,3],
    valid [B,K] -> int32 [B,K].  An invalid or NaN model counts 0."""
    valid, offsets, B, K, P = _score_args("ransac", models, x0, x1, valid, offsets)
    if P == 0 or B * K == 0:      # nothing to read: every count is 0
        return torch.zeros(models.shape[:-2], dtype=torch.int32, device=x0.device)
    counts = torch.empty(models.shape[:-2], dtype=torch.int32, device=x0.device)
    check(lib.gim_ransac_score(_p(models), _p(valid), _p(x0), _p(x1), _p(offsets), B, K, float(thr2), _p(counts), _stream()),
          "gim_ransac_score")
    return counts


def _model_mask(word, word_dev, symbol, models, x0, x1, thr2, offsets):
    """The one body of ransac_mask / homography_mask: the library's `symbol`; `word` names the models and `word_dev` the caller in
    a refusal."""
    _req_cuda(models, x0, x1, offsets)
    single = offsets is None
    if models.dtype != torch.float64 or models.shape != ((3, 3) if single else (models.shape[0], 3, 3)) or not models.is_contiguous():
        raise _lib.GimHipError(f"{word} must be contiguous fp64 {'[3,3]' if single else '[B,3,3]'}, got {models.dtype} {tuple(models.shape)}")
    B = 1 if single else models.shape[0]
    offsets, P = _ransac_points(x0, x1, offsets, B)
    if models.device != x0.device:
        raise _lib.GimHipError(f"{word_dev} and points are on different devices")
    mask = torch.empty(P, dtype=torch.uint8, device=x0.device)
    if P and B:
        check(getattr(lib, symbol)(_p(models), _p(x0), _p(x1), _p(offsets), B, float(thr2), _p(mask), _stream()), symbol)
    return mask.view(torch.bool)


def ransac_mask(models, x0, x1, thr2, offsets=None):
    """Inlier mask of one model per pair (gim_ransac_mask): model fp64 [3,3] (one pair) or [B,3,3] with offsets int32 [B+1]
    -> bool [Ptot], sampson_error(model of the point's pair) <= thr2."""
    return _model_mask("ransac_mask models", "ransac models", "gim_ransac_mask", models, x0, x1, thr2, offsets)


# ---- homography RANSAC step and perspective warp (gim_amd/pose.py, gim_amd/demo.py) ---------------------------------------
def _minimal_step(word, symbol, m, k, x0, x1, idx, thr2, offsets):
    """The one body of homography_step / fundamental_step / essential_step: samples of m points, k models per sample (None: one, and
    no model axis), the library's `symbol`, `word` names the step in a refusal.  The outputs are zero-filled: without a launch
    (B * K == 0, or no points, when every index is outside its pair) nothing is valid."""
    _req_cuda(x0, x1, idx, offsets)
    single = offsets is None
    if idx.dtype != torch.int32 or idx.dim() != (2 if single else 3) or idx.shape[-1] != m or not idx.is_contiguous():
        raise _lib.GimHipError(f"{word} idx must be contiguous int32 {f'[K,{m}]' if single else f'[B,K,{m}]'}, got {idx.dtype} {tuple(idx.shape)}")
    B, K = (1, idx.shape[0]) if single else idx.shape[:2]
    offsets, P = _ransac_points(x0, x1, offsets, B)
    if idx.device != x0.device:
        raise _lib.GimHipError(f"{word} idx and points are on different devices")
    lead = tuple(idx.shape[:-1]) + (() if k is None else (k,))
    models = torch.zeros(*lead, 3, 3, dtype=torch.float64, device=x0.device)
    valid = torch.zeros(lead, dtype=torch.uint8, device=x0.device)
    counts = torch.zeros(lead, dtype=torch.int32, device=x0.device)
    if B * K and P:
        check(getattr(lib, symbol)(_p(x0), _p(x1), _p(offsets), B, _p(idx), K, float(thr2), _p(models), _p(valid), _p(counts), _stream()),
              symbol)
    return models, valid.view(torch.bool), counts


def homography_step(src, dst, idx, thr2, offsets=None):
    """Four-point homographies dst ~ H src of the samples `idx`, solved and scored in one launch (gim_homography_step; fp64, the
    arithmetic and validity rules of pose.homography_4pt / pose.transfer_error).  One pair: src / dst fp64 [P,2], idx int32 [K,4]
    -> (models fp64 [K,3,3] with h33 = 1, valid bool [K], counts int32 [K]).  B pairs: offsets int32 [B+1] over the concatenated
    points, idx [B,K,4] relative to each pair's offset -> [B,K,3,3], [B,K], [B,K].  A rejected sample: zero model, valid 0, count 0."""
    return _minimal_step("homography", "gim_homography_step", 4, None, src, dst, idx, thr2, offsets)


def fundamental_step(x0, x1, idx, thr2, offsets=None):
    """Seven-point fundamental matrices x1^T F x0 = 0 of the samples `idx`, solved and scored in one launch (gim_fundamental_step;
    fp64, the arithmetic and validity rules of pose.seven_point_ge / pose.sampson_error).  One pair: x0 / x1 fp64 [P,2], idx int32
    [K,7] -> (models fp64 [K,3,3,3] of unit Frobenius norm, valid bool [K,3], counts int32 [K,3]): up to three models per sample, in
    the order of their roots.  B pairs: offsets int32 [B+1] over the concatenated points, idx [B,K,7] relative to each pair's offset
    -> [B,K,3,3,3], [B,K,3], [B,K,3].  A rejected sample or an unused slot: zero model, valid 0, count 0."""
    return _minimal_step("fundamental", "gim_fundamental_step", 7, 3, x0, x1, idx, thr2, offsets)


def essential_step(x0, x1, idx, thr2, offsets=None):
    """Five-point essential matrices x1^T E x0 = 0 of the samples `idx`, solved and scored in one launch (gim_essential_step; fp64,
    the arithmetic and validity rules of pose.five_point_ge / pose.sampson_error).  One pair: x0 / x1 fp64 [P,2] in normalised
    camera coordinates, idx int32 [K,5] -> (models fp64 [K,10,3,3] of unit Frobenius norm, valid bool [K,10], counts int32 [K,10]):
    up to ten models per sample, in the order of their roots.  B pairs: offsets int32 [B+1] over the concatenated points, idx
    [B,K,5] relative to each pair's offset -> [B,K,10,3,3], [B,K,10], [B,K,10].  A rejected sample or an unused slot: zero model,
    valid 0, count 0."""
    return _minimal_step("essential", "gim_essential_step", 5, 10, x0, x1, idx, thr2, offsets)


def recover_pose(E, x0, x1, mask=None, offsets=None, distance_thresh=1e9):
    """cv2.recoverPose for one pair or a batch in one launch (gim_recover_pose; fp64, the arithmetic of pose.recover_pose_ge): E is
    decomposed into its four (R, t) candidates, every match triangulated under each and tested for lying in front of both cameras
    nearer than distance_thresh.  One pair: E fp64 [3,3], x0 / x1 fp64 [P,2] in normalised camera coordinates, mask bool / uint8 [P]
    or None -> (n_good int32 [4] per candidate (R1,t), (R2,t), (R1,-t), (R2,-t); best int32 []: the first maximum; R fp64 [3,3]
    and t fp64 [3] of the winner; mask_out bool [P]: good under the winner).  B pairs: E [B,3,3], offsets int32 [B+1] over the
    concatenated points, mask [Ptot] -> [B,4], [B], [B,3,3], [B,3], [Ptot].  An E that is not finite or all zero: n_good 0,
    best -1, zero R and t, mask_out False; a pair without points: n_good 0, best 0, the first candidate."""
    _req_cuda(E, x0, x1, mask, offsets)
    single = offsets is None
    if E.dtype != torch.float64 or E.shape != ((3, 3) if single else (E.shape[0], 3, 3)) or not E.is_contiguous():
        raise _lib.GimHipError(f"recover_pose E must be contiguous fp64 {'[3,3]' if single else '[B,3,3]'}, got {E.dtype} {tuple(E.shape)}")
    B = 1 if single else E.shape[0]
    offsets, P = _ransac_points(x0, x1, offsets, B)
    if E.device != x0.device:
        raise _lib.GimHipError("recover_pose E and points are on different devices")
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype != torch.uint8 or mask.shape != (P,) or not mask.is_contiguous() or mask.device != x0.device:
            raise _lib.GimHipError(f"recover_pose mask must be contiguous bool / uint8 [{P}] on the points' device")
    dev = x0.device
    R = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(B, 3, dtype=torch.float64, device=dev)
    n_good = torch.empty(B, 4, dtype=torch.int32, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    mask_out = torch.empty(P, dtype=torch.uint8, device=dev)
    if B:
        # without points nothing reads x0, x1 or writes mask_out, but the entry point refuses a NULL pointer: 16 bytes stand in
        pad = torch.empty(2, dtype=torch.float64, device=dev) if P == 0 else None
        px0, px1, pm = (_p(pad),) * 3 if P == 0 else (_p(x0), _p(x1), _p(mask_out))
        check(lib.gim_recover_pose(_p(E), px0, px1, _p(offsets), B, _p(mask) if mask is not None and P else None, float(distance_thresh),
                                   _p(R), _p(t), _p(n_good), _p(best), pm, _stream()), "gim_recover_pose")
    if single:
        return n_good[0], best[0], R[0], t[0], mask_out.view(torch.bool)
    return n_good, best, R, t, mask_out.view(torch.bool)


def model_refit(kind, a, b, models, thr2, mask=None, offsets=None, rounds=1):
    """Least-squares refit of a model on its inliers and up to `rounds` rounds of refit / re-score, one launch for one pair or a
    batch (gim_model_refit; fp64, the arithmetic of pose.refit_ge).  kind 0: homographies b ~ H a (normalised DLT, transfer error);
    kind 1: fundamental matrices b^T F a = 0 (normalised eight-point, rank 2, Sampson error).  One pair: a / b fp64 [P,2], models
    fp64 [3,3], mask bool / uint8 [P] or None (None: the model's own mask under thr2) -> (model fp64 [3,3]: the last accepted refit,
    or the input when none was; mask bool [P] of that model; counts int32 [2]: inliers at the start and at the end; accepted int32
    []: rounds accepted).  B pairs: models [B,3,3], offsets int32 [B+1] over the concatenated points, mask [Ptot] -> [B,3,3],
    [Ptot], [B,2], [B].  A model that is all zero or not finite: its pair is skipped -- zero model, mask and counts, accepted -1."""
    kind, rounds = int(kind), int(rounds)
    if kind not in (0, 1):
        raise _lib.GimHipError(f"model_refit kind={kind}: 0 (homography) or 1 (fundamental matrix)")
    if not 1 <= rounds <= 8:
        raise _lib.GimHipError(f"model_refit rounds={rounds}: 1 <= rounds <= 8")
    _req_cuda(a, b, models, mask, offsets)
    single = offsets is None
    if models.dtype != torch.float64 or models.shape != ((3, 3) if single else (models.shape[0], 3, 3)) or not models.is_contiguous():
        raise _lib.GimHipError(f"model_refit models must be contiguous fp64 {'[3,3]' if single else '[B,3,3]'}, got {models.dtype} {tuple(models.shape)}")
    B = 1 if single else models.shape[0]
    offsets, P = _ransac_points(a, b, offsets, B)
    if models.device != a.device:
        raise _lib.GimHipError("model_refit models and points are on different devices")
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype != torch.uint8 or mask.shape != (P,) or not mask.is_contiguous() or mask.device != a.device:
            raise _lib.GimHipError(f"model_refit mask must be contiguous bool / uint8 [{P}] on the points' device")
    dev = a.device
    out = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
    accepted = torch.empty(B, dtype=torch.int32, device=dev)
    mask_out = torch.empty(P, dtype=torch.uint8, device=dev)
    if B:
        # without points nothing reads a, b or writes mask_out, but the entry point refuses a NULL pointer: 16 bytes stand in
        pad = torch.empty(2, dtype=torch.float64, device=dev) if P == 0 else None
        pa, pb, pm = (_p(pad),) * 3 if P == 0 else (_p(a), _p(b), _p(mask_out))
        with torch.cuda.device(dev):
            check(lib.gim_model_refit(kind, pa, pb, _p(offsets), B, _p(models), _p(mask) if mask is not None and P else None, float(thr2),
                                      rounds, _p(out), pm, _p(counts), _p(accepted), _stream()), "gim_model_refit")
    if single:
        return out[0], mask_out.view(torch.bool), counts[0], accepted[0]
    return out, mask_out.view(torch.bool), counts, accepted


def _on(device, a, dtype):
    """a tensor argument as it is, anything else (an int, a list, an array) as a tensor of `dtype` on `device`"""
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.atleast_1d(np.asarray(a)).astype(dtype), device=device)


def ransac_sample(offsets_or_P, first, count, K, m, seed):
    """The sample indices of one RANSAC step of B pairs, drawn on the device in one launch (gim_ransac_sample; the arithmetic of
    pose.device_samples: Philox4x32-10 words, Floyd's m distinct draws, m in (4, 5, 7)).  offsets_or_P: offsets int32 [B+1] over the
    concatenated points, or one pair's point count P; first int64 [B]: the ordinal of each pair's first sample of this step; count
    int32 [B]: the samples each pair uses (tensors on the device, or ints / sequences, which are uploaded); seed: 64 unsigned bits.
    -> idx int32 [B,K,m] ([K,m] for a point count): slot s of pair b is sample number first[b] + s of the pair's run; slots at or
    beyond count[b], and every slot of a pair with fewer than m points, hold -1."""
    K, m, seed = int(K), int(m), int(seed)
    if m not in (4, 5, 7):
        raise _lib.GimHipError(f"ransac_sample m={m}: 4, 5 or 7")
    if not 0 <= seed < 1 << 64 or K < 0:
        raise _lib.GimHipError(f"ransac_sample seed={seed} K={K}: a seed of 64 unsigned bits, K >= 0")
    tensors = [t for t in (offsets_or_P, first, count) if isinstance(t, torch.Tensor)]
    device = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    single = not isinstance(offsets_or_P, torch.Tensor) and np.ndim(offsets_or_P) == 0
    if single and not 0 <= int(offsets_or_P) < 1 << 31:
        raise _lib.GimHipError(f"ransac_sample P={offsets_or_P}: 0 <= P < 2^31")
    offsets = _on(device, [0, int(offsets_or_P)] if single else offsets_or_P, np.int32)
    first, count = _on(device, first, np.int64), _on(device, count, np.int32)
    _req_cuda(offsets, first, count)
    B = offsets.shape[0] - 1
    for t, dt, n, name in ((offsets, torch.int32, B + 1, "offsets"), (first, torch.int64, B, "first"), (count, torch.int32, B, "count")):
        if t.dtype != dt or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous() or t.device != device or n < 0:
            raise _lib.GimHipError(f"ransac_sample {name} must be contiguous {dt} [{n}] on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    idx = torch.empty(B, K, m, dtype=torch.int32, device=device)
    if idx.numel():
        with torch.cuda.device(device):
            check(lib.gim_ransac_sample(_p(offsets), B, _p(first), _p(count), K, m, seed, _p(idx), _stream()), "gim_ransac_sample")
    return idx[0] if single else idx


def ransac_records(counts, nb, floor):
    """The samples of a RANSAC step that set a new strict maximum of the inlier count, found on the device (gim_ransac_records; the
    rule of pose.step_records).  counts int32 [B,K,k], k in (1, 3, 10): the counts of homography_step / fundamental_step /
    essential_step; nb int32 [B]: the samples in use; floor int32 [B]: the count to beat (tensors on the device, or ints / sequences,
    which are uploaded).  -> rec int32 [B, 1 + 3 K]: rec[b, 0] = n_rec, then the triples (s, j_s, c_s) in ascending s; the words
    beyond the last triple are unspecified."""
    _req_cuda(counts)
    if counts.dtype != torch.int32 or counts.dim() != 3 or counts.shape[2] not in (1, 3, 10) or not counts.is_contiguous():
        raise _lib.GimHipError(f"ransac_records counts must be contiguous int32 [B,K,k], k in (1, 3, 10), got {counts.dtype} {tuple(counts.shape)}")
    B, K, k = counts.shape
    nb, floor = _on(counts.device, nb, np.int32), _on(counts.device, floor, np.int32)
    for t, name in ((nb, "nb"), (floor, "floor")):
        if t.dtype != torch.int32 or t.shape != (B,) or not t.is_contiguous() or t.device != counts.device:
            raise _lib.GimHipError(f"ransac_records {name} must be contiguous int32 [{B}] on the counts' device, got {t.dtype} {tuple(t.shape)}")
    rec = torch.empty(B, 1 + 3 * K, dtype=torch.int32, device=counts.device)
    if B:
        with torch.cuda.device(counts.device):
            check(lib.gim_ransac_records(_p(counts), _p(nb), _p(floor), B, K, k, _p(rec), _stream()), "gim_ransac_records")
    return rec


def magsac_score(kind, models, a, b, thr2, max_thr2=None, valid=None, offsets=None):
    """MAGSAC++ quality and inlier count of candidate models over matched points in one launch (gim_magsac_score; fp64, the
    arithmetic of pose.magsac_quality).  kind 1: fundamental matrices under the Sampson error (ransac_score's); kind 0: homographies
    b ~ M a under the forward transfer error (homography_mask's).  max_thr2: the squared k sigma bound the gain is marginalised up
    to (None: thr2).  Shapes as in ransac_score: models fp64 [K,3,3] (one pair) or [B,K,3,3] with offsets int32 [B+1], valid bool /
    uint8 [K] / [B,K] or None -> (quality int64, counts int32) of the models' leading shape.  An invalid model or one with an entry
    that is not finite: 0 and 0."""
    kind = int(kind)
    max_thr2 = float(thr2 if max_thr2 is None else max_thr2)
    if kind not in (0, 1):
        raise _lib.GimHipError(f"magsac_score kind={kind}: 0 (homography) or 1 (fundamental matrix)")
    if not (np.isfinite(max_thr2) and max_thr2 > 0.0):
        raise _lib.GimHipError(f"magsac_score max_thr2={max_thr2}: finite and positive")
    valid, offsets, B, K, P = _score_args("magsac", models, a, b, valid, offsets)
    if P == 0 or B * K == 0:      # nothing to read: every quality and count is 0
        return (torch.zeros(models.shape[:-2], dtype=torch.int64, device=a.device), torch.zeros(models.shape[:-2], dtype=torch.int32, device=a.device))
    quality = torch.empty(models.shape[:-2], dtype=torch.int64, device=a.device)
    counts = torch.empty(models.shape[:-2], dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        check(lib.gim_magsac_score(kind, _p(models), _p(valid), _p(a), _p(b), _p(offsets), B, K, float(thr2), max_thr2, _p(quality), _p(counts),
                                   _stream()), "gim_magsac_score")
    return quality, counts


def ransac_records64(quality, counts, nb, floor_q, min_count):
    """ransac_records keyed on an int64 quality (gim_ransac_records64; the rule of pose.step_records64).  quality int64 [B,K,k] and
    counts int32 [B,K,k], k in (1, 3, 10): magsac_score's outputs over a step's models; nb int32 [B]; floor_q int64 [B]: the quality
    to beat (tensors on the device, or ints / sequences, which are uploaded); min_count: a slot with fewer inliers has key 0.
    -> rec int64 [B, 1 + 4 K]: rec[b, 0] = n_rec, then (s, j_s, c_s, Q_s) in ascending s; the words beyond are unspecified."""
    _req_cuda(quality, counts)
    if quality.dtype != torch.int64 or quality.dim() != 3 or quality.shape[2] not in (1, 3, 10) or not quality.is_contiguous():
        raise _lib.GimHipError(f"ransac_records64 quality must be contiguous int64 [B,K,k], k in (1, 3, 10), got {quality.dtype} {tuple(quality.shape)}")
    if counts.dtype != torch.int32 or counts.shape != quality.shape or not counts.is_contiguous() or counts.device != quality.device:
        raise _lib.GimHipError(f"ransac_records64 counts must be contiguous int32 {tuple(quality.shape)} on the quality's device")
    B, K, k = quality.shape
    nb, floor_q = _on(quality.device, nb, np.int32), _on(quality.device, floor_q, np.int64)
    for t, dt, name in ((nb, torch.int32, "nb"), (floor_q, torch.int64, "floor_q")):
        if t.dtype != dt or t.shape != (B,) or not t.is_contiguous() or t.device != quality.device:
            raise _lib.GimHipError(f"ransac_records64 {name} must be contiguous {dt} [{B}] on the quality's device, got {t.dtype} {tuple(t.shape)}")
    rec = torch.empty(B, 1 + 4 * K, dtype=torch.int64, device=quality.device)
    if B:
        with torch.cuda.device(quality.device):
            check(lib.gim_ransac_records64(_p(quality), _p(counts), _p(nb), _p(floor_q), int(min_count), B, K, k, _p(rec), _stream()),
                  "gim_ransac_records64")
    return rec


def homography_mask(model, src, dst, thr2, offsets=None):
    """Inlier mask of one homography per pair (gim_homography_mask): model fp64 [3,3] (one pair) or [B,3,3] with offsets int32 [B+1]
    -> bool [Ptot], transfer_error(model of the point's pair) <= thr2."""
    return _model_mask("homography_mask model", "homography model", "gim_homography_mask", model, src, dst, thr2, offsets)


def warp_perspective(image, H, out_hw):
    """cv2.warpPerspective(image, H, (out_w, out_h)) with exact bilinear weights and a zero border (gim_warp_perspective).
    image: uint8 or fp32 [B,C,H,W] or [C,H,W] on the device, contiguous, C <= 4; H: 3x3 or [B,3,3] tensor or array (any device or
    the host; it is read on the host), mapping image pixels to output pixels; out_hw = (out_h, out_w).  -> the image's dtype,
    [B,C,out_h,out_w] or [C,out_h,out_w].  A singular H or one with an entry that is not finite raises before any launch."""
    _req_cuda(image)
    if image.dtype not in (torch.uint8, torch.float32) or image.dim() not in (3, 4) or not image.is_contiguous():
        raise _lib.GimHipError(f"warp_perspective image must be contiguous uint8 / fp32 [B,C,H,W] or [C,H,W], got {image.dtype} {tuple(image.shape)}")
    img = image if image.dim() == 4 else image[None]
    B, C, Hs, Ws = img.shape
    if not 1 <= C <= 4 or Hs < 1 or Ws < 1:
        raise _lib.GimHipError(f"warp_perspective takes 1 to 4 channels of a non-empty image, got {tuple(img.shape)}")
    Hn = np.array(H.detach().cpu().numpy() if isinstance(H, torch.Tensor) else H, dtype=np.float64)
    if Hn.shape == (3, 3):
        Hn = np.broadcast_to(Hn, (B, 3, 3))
    if Hn.shape != (B, 3, 3):
        raise _lib.GimHipError(f"warp_perspective H must be [3,3] or [B = {B},3,3], got {tuple(Hn.shape)}")
    if not np.isfinite(Hn).all():
        raise _lib.GimHipError("warp_perspective: H has an entry that is not finite")
    det = (Hn[:, 0, 0] * (Hn[:, 1, 1] * Hn[:, 2, 2] - Hn[:, 1, 2] * Hn[:, 2, 1]) - Hn[:, 0, 1] * (Hn[:, 1, 0] * Hn[:, 2, 2] - Hn[:, 1, 2] * Hn[:, 2, 0]) +
           Hn[:, 0, 2] * (Hn[:, 1, 0] * Hn[:, 2, 1] - Hn[:, 1, 1] * Hn[:, 2, 0]))     # by cofactors: exact zero for a repeated or zero row
    if not (np.isfinite(det).all() and (det != 0.0).all()):
        raise _lib.GimHipError(f"warp_perspective: singular H (det = {det.tolist()})")
    Hd, Wd = int(out_hw[0]), int(out_hw[1])
    if Hd < 0 or Wd < 0:
        raise _lib.GimHipError(f"warp_perspective: out_hw = {tuple(out_hw)}")
    out = torch.empty(B, C, Hd, Wd, dtype=img.dtype, device=img.device)
    if out.numel():
        d_H = torch.from_numpy(np.ascontiguousarray(Hn)).to(img.device)
        check(lib.gim_warp_perspective(_p(img), 0 if img.dtype == torch.uint8 else 1, B, C, Hs, Ws, _p(d_H), _p(out), Hd, Wd, _stream()),
              "gim_warp_perspective")
    return out if image.dim() == 4 else out[0]


# ---- gim_semseg ------------------------------------------------------------------------------------------------
PPM_SCALES = (1, 2, 3, 6)
PPM_BINS = 50            # 1 + 4 + 9 + 36 pooled vectors per image, bins of scale s from offset PPM_OFFSETS[s]
PPM_OFFSETS = {1: 0, 2: 1, 3: 5, 6: 14}


def ppm_pool(x, C=None):
    """x [B,H,W,ld] NHWC (ld >= C channels, e.g. the conv_last concat buffer) -> new fp32 [B,50,C]: adaptive average pooling to the
    scales 1, 2, 3, 6 (bin order of PPM_OFFSETS, row-major per scale) in one launch (gim_ppm_pool)"""
    _req_cuda(x)
    B, H, W, ld = x.shape
    C = ld if C is None else C
    assert x.stride(2) == ld and x.stride(-1) == 1 and x.stride(0) == H * W * ld
    out = torch.empty(B, PPM_BINS, C, dtype=torch.float32, device=x.device)
    check(lib.gim_ppm_pool(_p(x), _p(out), B, H, W, C, ld, gim_dtype(x), _stream()), "gim_ppm_pool")
    return out


def ppm_upsample_concat(br, y, c_off):
    """br fp32 [B,50,Cb] (the four branches after 1x1 conv + BN + ReLU) -> bilinear (align_corners=False) to y's h x w, written into
    channels c_off + i Cb .. of y [B,h,w,ld] (gim_ppm_upsample_concat), in place"""
    _req_cuda(br, y)
    B, h, w, ld = y.shape
    assert br.dtype == torch.float32 and br.is_contiguous() and br.shape[:2] == (B, PPM_BINS) and y.is_contiguous()
    Cb = br.shape[2]
    assert c_off + 4 * Cb <= ld
    check(lib.gim_ppm_upsample_concat(_p(br), _p(y), B, h, w, Cb, ld, c_off, gim_dtype(y), _stream()), "gim_ppm_upsample_concat")


def seg_head_argmax(logits, C, size, prob=False, flag=None):
    """logits fp32 [B,h,w,ld] (C classes) -> uint8 class map [B,H,W] of the bilinear (align_corners=False) upsampling to size = (H, W)
    and, prob=True, the fp32 maximum softmax probability [B,H,W] (gim_seg_head_argmax; the full-resolution logits are never stored).
    flag: int32 device word ORed with 1 when a logit is not finite.  Returns cls or (cls, prob)."""
    _req_cuda(logits, flag)
    B, h, w, ld = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous() and C <= ld
    H, W = int(size[0]), int(size[1])
    cls = torch.empty(B, H, W, dtype=torch.uint8, device=logits.device)
    pr = torch.empty(B, H, W, dtype=torch.float32, device=logits.device) if prob else None
    if flag is not None:
        assert flag.dtype == torch.int32 and flag.numel() >= 1
    with _Timed("seg_head_argmax", 10.0 * B * H * W * C):   # 4 taps (7 flops) + the exponential / compare per class and pixel
        check(lib.gim_seg_head_argmax(_p(logits), _p(cls), _p(pr), _p(flag), B, h, w, C, ld, H, W, _stream()), "gim_seg_head_argmax")
    return (cls, pr) if prob else cls


# ---- dense SfM: dense matches of a pair list -> keypoints and keypoint-indexed matches (gim_amd/dense_sfm.py) ------------------
AggState = collections.namedtuple("AggState", "kpts0 kpts1 scores geom votes cell_n cell_off max_error patch")
AggBatch = collections.namedtuple("AggBatch", "P row_lo row_hi offsets slot0 slot1 host_offsets host_slot0 host_slot1")
AggKeypoints = collections.namedtuple("AggKeypoints", "id_grid keypoints score cells kp_off host_kp_off nearest")
AggMatches = collections.namedtuple("AggMatches", "matches0 scores_f16 row_len koff0")


def agg_patch(max_error, cell_size):
    """patch = max(cell_size, max_error) of match_dense.py:64-65 as the integer the kernels take; GimHipError for a geometry they refuse
    (patch / int(max_error) not an integer in 1..8, max_error > patch / 2) -- checked by the library, no device involved"""
    ps = max(cell_size if cell_size is not None else max_error, max_error)
    if not (ps == int(ps) and 1 <= ps <= 4096):
        raise _lib.GimHipError(f"dense aggregation: patch = max(cell_size, max_error) = {ps} must be an integer in 1..4096")
    if lib.gim_agg_bins(float(max_error), int(ps)) == 0:
        msg = lib.gim_last_error()
        raise _lib.GimHipError(f"dense aggregation: max_error={max_error} cell_size={cell_size}: {msg.decode() if msg else ''}")
    return int(ps)


def agg_bins(max_error, patch):
    return int(lib.gim_agg_bins(float(max_error), int(patch)))


def agg_grid(width, height, patch):
    """(Gw, Gh) of an image: cells 0 .. W // patch + 1 per axis"""
    return int(width) // patch + 2, int(height) // patch + 2


def agg_batch(offsets, slot0, slot1, n_slots, pool_rows, device):
    """host lists of a batch of pairs -- offsets [P + 1] rising pool rows, slot0 / slot1 [P] -- checked here (the kernels get a launch
    shape from them) and uploaded in one copy -> AggBatch"""
    o = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    s0 = np.ascontiguousarray(np.asarray(slot0, dtype=np.int64).reshape(-1))
    s1 = np.ascontiguousarray(np.asarray(slot1, dtype=np.int64).reshape(-1))
    P = s0.shape[0]
    if s1.shape[0] != P or o.shape[0] != P + 1:
        raise _lib.GimHipError(f"dense aggregation: {P} first slots, {s1.shape[0]} second slots, {o.shape[0]} offsets (P, P, P + 1)")
    if P and (o[0] < 0 or o[-1] > pool_rows or np.any(o[1:] < o[:-1])):
        raise _lib.GimHipError(f"dense aggregation: offsets must rise within the pool's {pool_rows} rows, got {o[:8].tolist()}{'...' if P > 7 else ''}")
    for s in (s0, s1):
        bad = np.flatnonzero((s < 0) | (s >= n_slots))
        if bad.size:
            raise _lib.GimHipError(f"dense aggregation: pair {int(bad[0])} names slot {int(s[bad[0]])} outside [0, {n_slots})")
    tab = _upload_i32(np.concatenate([o, s0, s1]).astype(np.int32), device)
    return AggBatch(P, int(o[0]) if P else 0, int(o[-1]) if P else 0, tab[:P + 1], tab[P + 1:2 * P + 1], tab[2 * P + 1:], o, s0, s1)


def _agg_state_check(st):
    _req_cuda(st.kpts0, st.kpts1, st.scores, st.geom, st.votes, st.cell_n)
    assert st.kpts0.dtype == st.kpts1.dtype == st.scores.dtype == torch.float32 and st.geom.dtype == st.cell_n.dtype == torch.int32
    assert st.votes.dtype == torch.int64 and all(t.is_contiguous() for t in (st.kpts0, st.kpts1, st.scores, st.geom, st.votes, st.cell_n))
    rows, S, cells = st.scores.shape[0], st.geom.shape[0], st.cell_n.shape[0]
    if st.kpts0.shape != (rows, 2) or st.kpts1.shape != (rows, 2) or st.geom.shape != (S, 4):
        raise _lib.GimHipError(f"dense aggregation: pool {tuple(st.kpts0.shape)} / {tuple(st.kpts1.shape)} / {tuple(st.scores.shape)}, geom {tuple(st.geom.shape)}")
    if st.votes.numel() != cells * agg_bins(st.max_error, st.patch) or len(st.cell_off) != S + 1 or st.cell_off[-1] != cells:
        raise _lib.GimHipError(f"dense aggregation: {st.votes.numel()} vote sums for {cells} cells of {agg_bins(st.max_error, st.patch)} bins")
    return rows, S, cells


def agg_vote(st, batch):
    """gim_agg_vote: the matches of the batch's pairs vote in the cells of both images -> dropped int32 [P] on the device (matches that
    did not count: outside their image, or a score that is not finite and in [0, 65536))"""
    rows, S, cells = _agg_state_check(st)
    dropped = torch.empty(batch.P, dtype=torch.int32, device=st.scores.device)
    if batch.P:
        check(lib.gim_agg_vote(_p(st.kpts0), _p(st.kpts1), _p(st.scores), _p(batch.offsets), _p(batch.slot0), _p(batch.slot1), _p(st.geom),
                               _p(st.votes), _p(st.cell_n), _p(dropped), batch.P, batch.row_lo, batch.row_hi, rows, S, cells,
                               float(st.max_error), int(st.patch), _stream()), "gim_agg_vote")
    return dropped


def agg_finalize(st, max_kps=None):
    """gim_agg_finalize + the per-image ordering + gim_agg_keypoints -> AggKeypoints.  Ids: without max_kps the raster order of the
    voted cells; with max_kps the first max_kps cells in (score descending, raster) order.  One read-back: the voted cells per image."""
    rows, S, cells = _agg_state_check(st)
    if max_kps is not None and max_kps < 1:
        raise _lib.GimHipError(f"dense aggregation: max_kps={max_kps} (None or >= 1)")
    dev = st.scores.device
    key = torch.empty(cells, dtype=torch.int64, device=dev)
    cbin = torch.empty(cells, dtype=torch.int32, device=dev)
    check(lib.gim_agg_finalize(_p(st.votes), _p(st.cell_n), cells, float(st.max_error), int(st.patch), _p(key), _p(cbin), _stream()),
          "gim_agg_finalize")
    off = [int(x) for x in st.cell_off]
    voted = key > 0
    counts = torch.stack([voted[off[s]:off[s + 1]].sum() for s in range(S)]).tolist() if S else []
    keep = [c if not max_kps else min(c, int(max_kps)) for c in counts]
    kp_off = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    n_sel = int(kp_off[-1])
    if not max_kps:
        sel = torch.nonzero(voted).reshape(-1).to(torch.int32)             # raster order within a slot, slots in order
    else:
        parts = []
        for s in range(S):
            if keep[s]:
                order = torch.sort(key[off[s]:off[s + 1]], descending=True, stable=True).indices[:keep[s]]
                parts.append((order + off[s]).to(torch.int32))
        sel = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int32, device=dev)
    sel = sel.contiguous()
    kp_off_dev = _upload_i32(kp_off.astype(np.int32), dev)
    sel_slot = torch.repeat_interleave(torch.arange(S, dtype=torch.int32, device=dev), torch.as_tensor(keep, dtype=torch.int64, device=dev),
                                       output_size=n_sel) if n_sel else torch.empty(0, dtype=torch.int32, device=dev)
    id_grid = torch.empty(cells, dtype=torch.int32, device=dev)
    keypoints = torch.empty(n_sel, 2, dtype=torch.float32, device=dev)
    score = torch.empty(n_sel, dtype=torch.float64, device=dev)
    kcells = torch.empty(n_sel, 2, dtype=torch.int32, device=dev)
    check(lib.gim_agg_keypoints(_p(st.votes), _p(cbin), _p(st.geom), _p(sel), _p(sel_slot), _p(kp_off_dev), n_sel, S, cells,
                                float(st.max_error), int(st.patch), _p(id_grid), _p(keypoints), _p(score), _p(kcells), _stream()),
          "gim_agg_keypoints")
    return AggKeypoints(id_grid, keypoints, score, kcells, kp_off_dev, kp_off, bool(max_kps))


def agg_assign(st, kp, batch):
    """gim_agg_assign: keypoint-indexed one-to-one matches of the batch's pairs -> AggMatches: matches0 int32 / scores_f16 fp16 rows
    padded to the keypoint count of each pair's first image (pair p owns koff0[p]:koff0[p + 1], a host array), row_len int32 [P] on the
    device = max matched id0 + 1, the length hloc's matches0 has.  No host synchronisation."""
    rows, S, cells = _agg_state_check(st)
    _req_cuda(kp.id_grid, kp.keypoints, kp.kp_off)
    dev = st.scores.device
    K = np.diff(kp.host_kp_off)
    koff0 = np.concatenate([[0], np.cumsum(K[batch.host_slot0])]).astype(np.int64)
    koff1 = np.concatenate([[0], np.cumsum(K[batch.host_slot1])]).astype(np.int64)
    rows0, rows1, n = int(koff0[-1]), int(koff1[-1]), batch.row_hi - batch.row_lo
    if max(rows0, rows1) > 0x7fffffff:
        raise _lib.GimHipError(f"dense aggregation: {rows0} / {rows1} keypoint rows in one batch do not fit int32: use fewer pairs per batch")
    matches0 = torch.empty(rows0, dtype=torch.int32, device=dev)
    s16 = torch.empty(rows0, dtype=torch.float16, device=dev)
    row_len = torch.empty(batch.P, dtype=torch.int32, device=dev)
    if batch.P:
        ko = _upload_i32(np.concatenate([koff0, koff1]).astype(np.int32), dev)
        ws = torch.empty(max(int(lib.gim_agg_assign_ws_bytes(n, rows0, rows1)), 8), dtype=torch.uint8, device=dev)
        check(lib.gim_agg_assign(_p(st.kpts0), _p(st.kpts1), _p(st.scores), _p(batch.offsets), _p(batch.slot0), _p(batch.slot1), _p(st.geom),
                                 _p(kp.id_grid), _p(kp.keypoints), _p(kp.kp_off), _p(ko[:batch.P + 1]), _p(ko[batch.P + 1:]), batch.P,
                                 batch.row_lo, batch.row_hi, rows, S, cells, int(kp.keypoints.shape[0]), rows0, rows1, float(st.max_error),
                                 int(st.patch), int(kp.nearest), _p(matches0), _p(s16), _p(row_len), _p(ws), _stream()), "gim_agg_assign")
    return AggMatches(matches0, s16, row_len, koff0)


# ---- feature bank of the dense matchers (csrc/dense_bank.hip) ------------------------------------------------------------------------------
def dense_gather_pairs(levels, idx, n_slots):
    """levels: [(slab [n_slots, ...], dst [n_entries, ...])] contiguous device tensors with equal bytes per block (a multiple of 16);
    idx: int32 device tensor [n_entries].  Block d of every dst receives slot idx[d] of its slab (gim_dense_gather_pairs: one launch
    per 8 levels; an index outside [0, n_slots) leaves its blocks untouched; nothing waits for the indices)."""
    _req_cuda(idx, *[t for lv in levels for t in lv])
    if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
        raise _lib.GimHipError(f"dense_gather_pairs: idx must be a contiguous int32 vector, got {idx.dtype} {tuple(idx.shape)}")
    n = idx.numel()
    for i in range(0, len(levels), _lib.DenseGatherArgs.MAX):
        args = _lib.DenseGatherArgs()
        chunk = levels[i:i + _lib.DenseGatherArgs.MAX]
        for k, (slab, dst) in enumerate(chunk):
            bb = slab[0].numel() * slab.element_size()
            if not (slab.is_contiguous() and dst.is_contiguous() and slab.shape[0] == n_slots and dst.shape[0] == n
                    and (n == 0 or dst[0].numel() * dst.element_size() == bb)):
                raise _lib.GimHipError(f"dense_gather_pairs: level {i + k}: slab {tuple(slab.shape)} / destination {tuple(dst.shape)} for "
                                       f"{n_slots} slots and {n} entries")
            args.slab[k], args.dst[k], args.slot_bytes[k] = slab.data_ptr(), dst.data_ptr(), bb
        args.n_levels = len(chunk)
        check(lib.gim_dense_gather_pairs(ctypes.byref(args), _p(idx), n, int(n_slots), _stream()), "gim_dense_gather_pairs")


def dense_pair_geometry(rows, device):
    """rows: one 16-tuple per pair in the field order of struct gim_dense_pair_geom -> fp32 [B, 16] on the device"""
    t = torch.tensor(rows, dtype=torch.float32).reshape(-1, 16)
    return t.to(device, non_blocking=True)


def dense_emit_pairs(sparse, mconf, geom, rescale):
    """sparse [B,num,4], mconf [B,num] fp32, geom [B,16] (dense_pair_geometry) -> (keypoints0 [B,num,2], keypoints1 [B,num,2],
    scores [B,num], count int32 [B]) on the device: per pair the kept rows in input order at the front (gim_dense_emit_pairs)."""
    _req_cuda(sparse, mconf, geom)
    B, num = mconf.shape
    assert sparse.shape == (B, num, 4) and geom.shape == (B, 16)
    assert sparse.dtype == mconf.dtype == geom.dtype == torch.float32
    assert sparse.is_contiguous() and mconf.is_contiguous() and geom.is_contiguous()
    dev = sparse.device
    k0 = torch.empty(B, num, 2, dtype=torch.float32, device=dev)
    k1 = torch.empty(B, num, 2, dtype=torch.float32, device=dev)
    sc = torch.empty(B, num, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.gim_dense_emit_pairs(_p(sparse), _p(mconf), _p(geom), _p(k0), _p(k1), _p(sc), _p(count), B, num, int(bool(rescale)), _stream()),
          "gim_dense_emit_pairs")
    return k0, k1, sc, count


# ---- video pseudo-labels (gim_amd/video_labels.py; csrc/label_link.hip) -------------------------------------------------------------
LABEL_MAX_KEY = 1 << 24        # csrc/label_key.h GIM_LABEL_MAX_KEY: the largest key range w * (h + 1)


def _label_sizes(width, height, B):
    """(width, height) per link as a host int32 [B,2]; raises before anything touches the device"""
    wh = np.stack(np.broadcast_arrays(np.asarray(width, dtype=np.int64).reshape(-1), np.asarray(height, dtype=np.int64).reshape(-1)), 1)
    if wh.shape[0] == 1 and B != 1:
        wh = np.repeat(wh, B, 0)
    if wh.shape[0] != B:
        raise ValueError(f"label_link: {wh.shape[0]} (width, height) pairs for {B} links")
    if B and (wh.min() < 1 or (wh[:, 0] * (wh[:, 1] + 1)).max() > LABEL_MAX_KEY):
        raise ValueError(f"label_link: width and height must be >= 1 and width * (height + 1) <= 2^24, got {wh.tolist()}")
    return np.ascontiguousarray(wh, dtype=np.int32)


def label_link_max_keys(width, height):
    """the table length a workspace needs for these frame sizes: the largest w * (h + 1) + 1"""
    w, h = np.asarray(width, dtype=np.int64).reshape(-1), np.asarray(height, dtype=np.int64).reshape(-1)
    wh = _label_sizes(w, h, max(w.size, h.size)).astype(np.int64)
    return int((wh[:, 0] * (wh[:, 1] + 1)).max()) + 1 if len(wh) else 1


def label_link_workspace(B, max_keys, device):
    """a zeroed workspace for label_link calls of up to B links and max_keys slots; every call leaves it zeroed again"""
    nbytes = lib.gim_label_link_ws_bytes(int(B), int(max_keys))
    if nbytes < 0:
        raise _lib.GimHipError(f"label_link_workspace B={B} max_keys={max_keys}")
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=device)


def label_link(lab0, lab1, width, height, *, offsets0=None, offsets1=None, workspace=None, out=None, ij=None):
    """walk.py:link on the device (gim_label_link: three launches, no host read).  lab0 fp32 [N,4] and lab1 fp32 [M,4]: labels
    (x0, y0, x1, y1) of the frame pairs a->b and b->c; width, height: the size of the frames the labels are in.  Rows of lab0 and lab1
    that share the rounded pixel round(x) + round(y) * width of frame b are joined, the last row of a pixel on either side, in
    ascending lab0 row -> (out fp32 [N,4]: (lab0[i, 0:2], lab1[j, 2:4]) in the first count rows; ij int32 [N,2]; count int32 [B];
    dropped int32 [B,2]: the rows of either side whose key is not finite or outside [0, width * (height + 1)], which are ignored).
    B links at once: the labels concatenated, offsets0 / offsets1 int32 [B+1] (device tensors, or sequences, which are uploaded) and
    width / height ints or one per link; link b's rows are out[offsets0[b] : offsets0[b] + count[b]], ij is relative to the link.
    workspace: label_link_workspace(...) to reuse across calls (zero on entry, zero again afterwards); out / ij: buffers to write into
    (rows beyond a link's count are not touched)."""
    _req_cuda(lab0, lab1, workspace, out, ij)
    for t, name in ((lab0, "lab0"), (lab1, "lab1")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous() or t.device != lab0.device:
            raise _lib.GimHipError(f"label_link {name} must be contiguous fp32 [n,4] on one device, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if (offsets0 is None) != (offsets1 is None):
        raise _lib.GimHipError("label_link takes both offsets or neither")
    dev, N, M = lab0.device, lab0.shape[0], lab1.shape[0]
    single = offsets0 is None
    if not single:
        offsets0, offsets1 = _on(dev, offsets0, np.int32), _on(dev, offsets1, np.int32)
        for t, name in ((offsets0, "offsets0"), (offsets1, "offsets1")):
            if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < 1 or t.shape != offsets0.shape or not t.is_contiguous() or t.device != dev:
                raise _lib.GimHipError(f"label_link {name} must be contiguous int32 [B+1] on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    B = 1 if single else offsets0.shape[0] - 1
    if B > 65535:
        raise _lib.GimHipError(f"label_link B={B}: at most 65535 links")
    wh = _label_sizes(width, height, B)
    need = int((wh[:, 0].astype(np.int64) * (wh[:, 1] + 1)).max()) + 1 if B else 1
    if workspace is None:
        workspace = label_link_workspace(B, need, dev)
        max_keys = need
    else:
        if workspace.dtype != torch.int32 or workspace.dim() != 1 or not workspace.is_contiguous() or workspace.device != dev:
            raise _lib.GimHipError(f"label_link workspace must be contiguous int32 [.] on {dev} (label_link_workspace)")
        max_keys = min(workspace.shape[0] // (2 * B), LABEL_MAX_KEY + 1) if B else need
        if max_keys < need:
            raise _lib.GimHipError(f"label_link workspace has {workspace.shape[0]} words, {B} links of {need} keys need {2 * B * need}")
    if out is None:
        out = torch.empty(N, 4, dtype=torch.float32, device=dev)
    if ij is None:
        ij = torch.empty(N, 2, dtype=torch.int32, device=dev)
    for t, dt, k, name in ((out, torch.float32, 4, "out"), (ij, torch.int32, 2, "ij")):
        if t.dtype != dt or t.shape != (N, k) or not t.is_contiguous() or t.device != dev:
            raise _lib.GimHipError(f"label_link {name} must be contiguous {dt} [{N},{k}] on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    count = torch.empty(B, dtype=torch.int32, device=dev)
    dropped = torch.empty(B, 2, dtype=torch.int32, device=dev)
    if B:
        wh_dev = None if B == 1 else torch.from_numpy(wh).to(dev)
        with torch.cuda.device(dev):
            check(lib.gim_label_link(_p(lab0) if N else None, _p(offsets0), N, _p(lab1) if M else None, _p(offsets1), M,
                                     wh.ctypes.data_as(ctypes.c_void_p), _p(wh_dev), B, max_keys, _p(workspace), _p(out) if N else None,
                                     _p(ij) if N else None, _p(count), _p(dropped), _stream()), "gim_label_link")
    return out, ij, count, dropped


def label_pack(k0, k1, keep=None, moved_thr=0.0, affine=None, vratio=1.0, out=None):
    """The tail of a labelling step in one launch (gim_label_pack; video_preprocessor.py:513-555).  k0, k1 fp32 [n,2]: the matched
    keypoints of a pair; keep bool / uint8 [n] or None: the inlier mask; moved_thr > 0: rows with |dx| < moved_thr and |dy| < moved_thr
    are dropped (static matches: watermarks); affine: 8 numbers (sx0, sy0, ox0, oy0, sx1, sy1, ox1, oy1) -> (x * s + o) * vratio in
    fp64, rounded to fp32; without it the fp32 product x * vratio -> (out fp32 [n,4]: the kept rows (x0, y0, x1, y1) in input order in
    the first count rows, count int32 [])."""
    _req_cuda(k0, k1, keep, out)
    for t, name in ((k0, "k0"), (k1, "k1")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or t.shape != k0.shape or not t.is_contiguous() or t.device != k0.device:
            raise _lib.GimHipError(f"label_pack {name} must be contiguous fp32 [n,2] on one device, got {t.dtype} {tuple(t.shape)} on {t.device}")
    n, dev = k0.shape[0], k0.device
    if keep is not None:
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        if keep.dtype != torch.uint8 or keep.shape != (n,) or not keep.is_contiguous() or keep.device != dev:
            raise _lib.GimHipError(f"label_pack keep must be contiguous bool / uint8 [{n}] on the points' device")
    a = None
    if affine is not None:
        a = np.ascontiguousarray(affine, dtype=np.float64).reshape(-1)
        if a.shape != (8,):
            raise ValueError(f"label_pack affine: 8 numbers (sx0, sy0, ox0, oy0, sx1, sy1, ox1, oy1), got {a.shape[0]}")
    if out is None:
        out = torch.empty(n, 4, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.shape != (n, 4) or not out.is_contiguous() or out.device != dev:
        raise _lib.GimHipError(f"label_pack out must be contiguous fp32 [{n},4] on the points' device")
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.gim_label_pack(_p(k0) if n else None, _p(k1) if n else None, _p(keep) if n else None, n, float(moved_thr),
                                 a.ctypes.data_as(ctypes.c_void_p) if a is not None else None, float(vratio), _p(out) if n else None, _p(count),
                                 _stream()), "gim_label_pack")
    return out, count[0]


# ---- frame preparation of the video labeller (gim_amd/frame_prep.py) -----------------------------------------------
class FramePrepResult(NamedTuple):
    buffers: dict                      # output name -> the flat ragged buffer of the batch (absent: no job asked for it)
    kept: Optional[torch.Tensor]       # int32 [J]: the sum of every job's mask, or None
    plan: object                       # frame_prep.Plan: the tables and every job's (offset, shape) per output

    def get(self, job, name):
        """the output `name` of job `job`, a view of the batch's buffer in its own shape"""
        off, shape = self.plan.views[job][name]
        n = int(np.prod(shape))
        return self.buffers[name][off:off + n].view(shape)


def frame_prep(frames, seg, exclude, jobs, kept=True, buffers=None, guard=0):
    """J jobs of crop + area resize + class mask + the matchers' inputs in one launch (gim_frame_prep; the reference's
    video_preprocessor.py:292-366, :406-493, :603-621).  frames uint8 [S,H,W,3] RGB; seg uint8 [S,Hs,Ws] class maps or None (no job
    may ask for a mask then, and `kept` is not computed); exclude: a uint8 [256] device tensor (non-zero: excluded), or what
    frame_prep.exclude_table takes; jobs: a sequence of (slot, box (x0, y0, x1, y1) | None, (wn, hn), flags) with frame_prep's OUT_*
    flags.  -> FramePrepResult: ragged flat buffers per output, get(job, name) for a job's view, kept int32 [J].  Every output equals
    frame_prep.frame_prep_np bit for bit.  An empty job list launches nothing.  buffers: {name: flat tensor} to write into instead of
    fresh ones (at least plan.elems long each); guard: elements left untouched in front of and behind every job's output."""
    from . import frame_prep as fp
    _req_cuda(frames, seg)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise _lib.GimHipError(f"frame_prep frames must be contiguous uint8 [S,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
    dev = frames.device
    S, H, W = frames.shape[:3]
    if seg is not None and (seg.dtype != torch.uint8 or seg.dim() != 3 or seg.shape[0] != S or not seg.is_contiguous() or seg.device != dev):
        raise _lib.GimHipError(f"frame_prep seg must be contiguous uint8 [{S},Hs,Ws] on {dev}, got {seg.dtype} {tuple(seg.shape)} on {seg.device}")
    jobs = list(jobs)
    for slot, _, _, flags in jobs:
        if not 0 <= int(slot) < S:
            raise _lib.GimHipError(f"frame_prep: slot {slot} is outside [0, {S})")
        if seg is None and int(flags) & (fp.OUT_MASK | fp.OUT_MASK8 | fp.MASKED):
            raise _lib.GimHipError("frame_prep: a job asks for a mask and there are no class maps")
    try:
        pl = fp.plan((H, W), jobs, guard=int(guard))
    except ValueError as e:
        raise _lib.GimHipError(str(e)) from e
    J, n_work = pl.jobs.shape[0], pl.work.shape[0]
    dtypes = (torch.uint8, torch.uint8, torch.uint8, torch.float32, torch.float32, torch.float32)
    if buffers is None:
        bufs = {name: torch.empty(n, dtype=dt, device=dev) for name, n, dt in zip(fp.OUTPUTS, pl.elems, dtypes) if n}
    else:
        bufs = {name: buffers[name] for name, n in zip(fp.OUTPUTS, pl.elems) if n}
        for name, n, dt in zip(fp.OUTPUTS, pl.elems, dtypes):
            t = bufs.get(name)
            if t is not None and (t.dtype != dt or t.dim() != 1 or t.shape[0] < n or not t.is_contiguous() or t.device != dev):
                raise _lib.GimHipError(f"frame_prep buffers[{name!r}] must be contiguous {dt} [>= {n}] on {dev}")
    want_kept = bool(kept) and seg is not None
    kept_t = torch.empty(J, dtype=torch.int32, device=dev) if want_kept else None
    if J == 0:
        return FramePrepResult(bufs, kept_t, pl)
    if isinstance(exclude, torch.Tensor):
        if exclude.dtype != torch.uint8 or exclude.shape != (256,) or not exclude.is_contiguous() or exclude.device != dev:
            raise _lib.GimHipError(f"frame_prep exclude must be contiguous uint8 [256] on {dev}")
        excl = exclude
    else:
        excl = torch.from_numpy(fp.exclude_table(exclude if exclude is not None else [])).to(dev)
    # one upload: the job table and, behind it (J * 128 bytes: 16-byte aligned), the work table
    host = np.concatenate([pl.jobs.reshape(-1), np.ascontiguousarray(pl.work).reshape(-1).view(np.int64)])
    tab = torch.from_numpy(host).to(dev)
    jobs_dev, work_dev = tab, tab[J * fp.JOB_WORDS:]
    elems = np.asarray([bufs[name].shape[0] if name in bufs else 0 for name in fp.OUTPUTS], dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with torch.cuda.device(dev):
        with _Timed("frame_prep", 0.0):
            check(lib.gim_frame_prep(_p(frames), S, H, W, _p(seg), seg.shape[1] if seg is not None else 0,
                                     seg.shape[2] if seg is not None else 0, _p(excl), vp(pl.jobs), _p(jobs_dev), J, vp(pl.work),
                                     _p(work_dev), n_work, vp(elems), *(_p(bufs.get(name)) for name in fp.OUTPUTS), _p(kept_t),
                                     _stream()), "gim_frame_prep")
    return FramePrepResult(bufs, kept_t, pl)
