"""What the two dense matchers (gim_dkm, gim_roma) are made of: the ConvRefiner cascade and the GP of the reference's
`networks/dkm/models/dkm.py` / `networks/roma/roma.py` (RoMa's are DKM's with other sizes), and the shared part of their
`RegressionMatcher` surface -- `match`, the head and tail of `match_batch`, `sample` and the caller-side adapter.

Each engine keeps its encoder, its coarse stage and its `_decode` / `match_batch` body (gim_amd/dkm/dkm.py, gim_amd/roma/roma.py).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import GIM_F32, GimHipError
from .packing import PRECISION_DTYPE, cstore, is_half, pack_conv, torch_dtype
from .switches import flag, tri_flag

HIDDEN_BLOCKS = 8


def refiner_dims(refiner_table, scale):
    """(input channels, hidden channels) of the scale's ConvRefiner; refiner_table[scale] = (feature channels, displacement
    embedding channels, local-correlation radius or None)"""
    c, e, r = refiner_table[scale]
    in_dim = 2 * c + e + ((2 * r + 1) ** 2 if r else 0)
    return in_dim, {"2": 128 + 16, "1": 24}.get(scale, in_dim)


# ---------------------------------------------------------------------------------------- parameter containers
class GP(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.pos_conv = nn.Conv2d(2, dim, 1)


def _block(ci, co, bn_momentum):
    return nn.Sequential(nn.Conv2d(ci, co, 5, 1, 2, groups=ci), nn.BatchNorm2d(co, momentum=bn_momentum), nn.ReLU(inplace=True),
                         nn.Conv2d(co, co, 1))


class ConvRefiner(nn.Module):
    def __init__(self, in_dim, hid, emb_dim, bn_momentum=0.1):
        super().__init__()
        self.block1 = _block(in_dim, hid, bn_momentum)
        self.hidden_blocks = nn.Sequential(*[_block(hid, hid, bn_momentum) for _ in range(HIDDEN_BLOCKS)])
        self.out_conv = nn.Conv2d(hid, 3, 1)
        self.disp_emb = nn.Conv2d(2, emb_dim, 1)


def _bn_after_bias(bn, bias):
    """eval BatchNorm applied to conv(x) + bias == BatchNorm with mean - bias applied to conv(x)"""
    return (bn.weight, bn.bias, bn.running_mean - bias, bn.running_var, bn.eps)


# ---------------------------------------------------------------------------------------- ConvRefiner
def pack_refiner(P, s, ref, in_dim, hid, dt, device):
    """ConvRefiner `ref` of scale s -> P[cr{s}.{i}.dw / .pw / .pwf], P[cr{s}.out / .emb / .cin_store]"""
    blocks = [ref.block1] + list(ref.hidden_blocks)
    for i, blk in enumerate(blocks):
        conv, bn, _, pw = blk
        ci = in_dim if i == 0 else hid
        cpad = cstore(hid, dt)
        sc = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        W = torch.zeros(25, cpad)
        W[:, :hid] = conv.weight.detach().float().reshape(hid, 25).t().cpu()
        scale, shift = torch.zeros(cpad), torch.zeros(cpad)
        scale[:hid] = sc.cpu()
        shift[:hid] = (bn.bias.detach().float() + (conv.bias.detach().float() - bn.running_mean.detach().float()) * sc).cpu()
        P[f"cr{s}.{i}.dw"] = (W.to(device), scale.to(device), shift.to(device), ci, hid)
        P[f"cr{s}.{i}.pw"] = pack_conv(pw.weight, None, dt, device, cin_pad=cpad, bias=pw.bias)
        if dt != GIM_F32 and cpad in (24, 32, 144) and ci == hid:   # refiner blocks that fit one launch (gim_dwconv5x5_pw): dw 5x5 + BN + ReLU + 1x1
            npc, kp = (160, 144) if cpad == 144 else (32, 32)
            wf, bf = torch.zeros(npc, kp), torch.zeros(npc)
            wf[:hid, :hid] = pw.weight.detach().float().reshape(hid, hid).cpu()
            bf[:hid] = pw.bias.detach().float().cpu()
            P[f"cr{s}.{i}.pwf"] = (wf.to(device).to(torch_dtype(dt)).contiguous(), bf.to(device))
    P[f"cr{s}.out"] = pack_conv(ref.out_conv.weight, None, dt, device, cin_pad=cstore(hid, dt), bias=ref.out_conv.bias)
    P[f"cr{s}.emb"] = (ref.disp_emb.weight.detach().float().reshape(-1, 2).contiguous().to(device),
                       ref.disp_emb.bias.detach().float().contiguous().to(device))
    P[f"cr{s}.cin_store"] = cstore(in_dim, dt)


def refine(P, s, dt, x, y, flow, cert, ins, full_hw, dims, fused, emb_scale=None, roma_layout=False):
    """ConvRefiner.forward + the flow / certainty update of Decoder.forward (dkm.py:75-123, 498-514; roma.py:529-580, 318-331).
    dims = (c, e, r) of the engine's refiner table; fused: wide-enough blocks as one launch (gim_dwconv5x5_pw);
    emb_scale: RoMa's disp_emb(40/32 * scale_factor * (flow - coords)), roma.py:545-547; roma_layout: its (dx, dy, certainty) order."""
    tdt = torch_dtype(dt)
    b, h, w, _ = x.shape
    c, e, r = dims
    cs = P[f"cr{s}.cin_store"]
    dev = x.device
    g = 8 if is_half(dt) else 4
    ew, eb = P[f"cr{s}.emb"]
    if emb_scale is not None:
        ew = ew * emb_scale
    if c % g == 0:
        D = torch.zeros(b, h, w, cs, dtype=tdt, device=dev)
        rows = D.view(b * h * w, cs)
        D[..., :c].copy_(x[..., :c])
        ops.grid_sample(y, flow, rows[:, c:2 * c])
        ops.dkm_disp_emb(flow, ew, eb, rows[:, 2 * c:])
        if r:
            ops.local_corr(x, y, flow, r, rows[:, 2 * c + e:])
    else:  # scale 1: 3 image / 9 projected channels (stored with padding) -> assemble the 12- / 24-channel input with copies
        xh = torch.empty(b * h * w, x.shape[3], dtype=tdt, device=dev)
        ops.grid_sample(y, flow, xh)
        emb = torch.empty(b * h * w, cstore(e, dt), dtype=tdt, device=dev)
        ops.dkm_disp_emb(flow, ew, eb, emb)
        D = torch.zeros(b, h, w, cs, dtype=tdt, device=dev)
        D[..., :c].copy_(x[..., :c])
        D[..., c:2 * c].copy_(xh.view(b, h, w, -1)[..., :c])
        D[..., 2 * c:2 * c + e].copy_(emb.view(b, h, w, -1)[..., :e])
    d = D
    for i in range(1 + HIDDEN_BLOCKS):
        W_, sc, sh, ci, co = P[f"cr{s}.{i}.dw"]
        pwf = P.get(f"cr{s}.{i}.pwf") if fused else None
        if pwf is not None and d.shape[3] == W_.shape[1] and d.is_contiguous():
            d = ops.dwconv5x5_pw(d, W_, sc, sh, *pwf)   # the whole block in one launch: the depthwise output never leaves the CU
            continue
        d = ops.dwconv5x5_bn_relu(d, W_, sc, sh, ci, co)
        d = ops.conv2d(d, P[f"cr{s}.{i}.pw"])
    out = torch.empty(b * h * w, P[f"cr{s}.out"].n_store, dtype=torch.float32, device=dev)
    ops.linear(d.view(b * h * w, d.shape[3]), P[f"cr{s}.out"], out)
    ops.dkm_flow_update(flow, cert, out, ins / (4.0 * full_hw[1]), ins / (4.0 * full_hw[0]), roma_layout=roma_layout)


# ---------------------------------------------------------------------------------------- GP
def gp_features(pos_conv, h, w, dim):
    """f = cos(8 pi pos_conv(coords)) of GP.get_pos_enc (dkm.py:314-331, roma.py:94-108): constant per (h, w); built on the host
    with the reference's fp32 ops as rows [h*w, dim] (the engines cache it on the device)."""
    ys = torch.linspace(-1 + 1 / h, 1 - 1 / h, h)
    xs = torch.linspace(-1 + 1 / w, 1 - 1 / w, w)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    coords = torch.stack((gx, gy))[None]
    f = torch.cos(8 * math.pi * F.conv2d(coords, pos_conv.weight.detach().float().cpu(), pos_conv.bias.detach().float().cpu()))
    return f[0].permute(1, 2, 0).reshape(h * w, dim).contiguous()


def gp_posterior(a32, nb, h, w, f, out, exact):
    """GP.forward, no_cov (dkm.py:340-370, roma.py:110-136) for all nb = 2 * pairs directions (image d is matched against image
    (d + nb/2) % nb).  a32: fp32 rows [nb*hw (+64 slack), 512] of the projected features; f: gp_features rows [hw, dim] on the
    device; writes mu into `out` (row view [nb*hw, dim]).  exact (fp32 `out` only): every step in fp64 (gim_gp_posterior_f64);
    otherwise the fp32 kernel matrix on the MFMA + fp64 Cholesky."""
    dev = a32.device
    n = h * w
    half = nb // 2
    dim = f.shape[1]
    if exact and out.dtype == torch.float32:
        X = a32[:nb * n].view(nb, n, 512)
        ops.gp_posterior_f64(X, X.roll(-half, 0).contiguous(), f, out, 0.2, 1e-6, 0.1)   # support of direction b: image (b + half) % nb
        return
    nrm = ops.row_norms(a32[:nb * n], 512)
    ld = (n + 63) // 64 * 64
    npad = (n + 31) // 32 * 32
    Kyy = torch.zeros(nb, n, ld, dtype=torch.float32, device=dev)
    Kxy = torch.zeros(nb, n, max(ld, npad), dtype=torch.float32, device=dev)
    for b in range(nb):
        o = (b + half) % nb                              # support of direction b = the other image of its pair
        ops.matmul_nt(a32[o * n:(o + 1) * n], a32[o * n:], n, Kyy[b])
        ops.matmul_nt(a32[b * n:(b + 1) * n], a32[o * n:], n, Kxy[b])
    ny = nrm.view(nb, n).roll(-half, 0).contiguous().view(-1)
    ops.cos_kernel_finish(Kyy.view(nb * n, ld), ny, ny, nb, n, n, 0.2, 1e-6, 0.1)        # K_yy + sigma_noise I
    ops.cos_kernel_finish(Kxy.view(nb * n, Kxy.shape[2]), nrm, ny, nb, n, n, 0.2, 1e-6, 0.0)
    Xt = ops.gp_solve(Kyy, f[None].expand(nb, n, dim).contiguous(), npad)
    for b in range(nb):
        ops.matmul_nt(Kxy[b][:, :npad], Xt[b], dim, out[b * n:(b + 1) * n])      # mu = K_xy (K_yy + sigma I)^-1 f


# ---------------------------------------------------------------------------------------- the matcher surface
class DenseFeatures:
    """What `DenseMatcher.extract` returns: `tensors` {kind: [N, ...]} -- the per-image state of N images -- and the `tag`
    (`DenseMatcher.feature_tag()`) it was computed under."""

    def __init__(self, tensors, tag):
        self.tensors, self.tag = tensors, tag

    def __len__(self):
        return next(iter(self.tensors.values())).shape[0]

    @property
    def nbytes_per_image(self):
        return sum(t[0].numel() * t.element_size() for t in self.tensors.values())


class DenseMatcher(nn.Module):
    """What `RegressionMatcher` of gim_dkm and gim_roma have in common.  A subclass sets `engine`, `max_batch`, `kde_half`, creates
    `self.precision` and its parameter tree, and provides `_prepack(device)` (-> `self._packed = (P, dt, device)`), `_state` (everything computed from one image alone) and
    `_match_state` (everything that depends on both images of a pair); `match_batch` and `match_features` are built from the two."""
    engine = None       # name in messages
    max_batch = None    # pairs per match_batch call
    kde_half = False    # sample(): the KDE on fp16-rounded coordinates (roma.py:1018-1023)

    def __init__(self, h, w, sample_mode, upsample_preds, symmetric, name):
        super().__init__()
        self.w_resized, self.h_resized = w, h
        self.sample_mode = sample_mode
        self.upsample_preds = upsample_preds
        self.symmetric = symmetric
        self.name = name
        self.sample_thresh = 0.05
        # GP posterior entirely in fp64 (kernel entries, Cholesky, products; csrc/gp_solve.hip: gim_gp_posterior_f64).  None = in
        # the fp32 parity mode only: the system's condition number (~2e4) turns fp32 rounding of the kernel ENTRIES into ~1e-4 of mu,
        # the one term of the engine's deviation that is not the reference's own (tests/test_gpu_gp_pins.py)
        self.gp_exact = tri_flag("gp_exact")
        # 16-bit modes: the 144- and 24-channel ConvRefiner blocks (scales 2 and 1, both passes) as ONE launch each (gim_dwconv5x5_pw, round 5)
        self.refiner_fused = flag("refiner_fused", True)
        self._packed = None
        self._epoch = 0      # moves with every weight change / device move: per-image state extracted before it is stale (feature_tag)

    def _gp_is_exact(self):
        return (self.precision == "fp32") if self.gp_exact is None else self.gp_exact

    def _images(self, dt, im1, im2, hs, ws):
        """[B,3,H,W] x 2 -> NHWC [2B, hs, ws, cpad]: queries first, then supports (extract_backbone_features, dkm.py:572-581,
        roma.py:668-678); im2 None: the images of im1 alone (extract)"""
        ims = [im1] if im2 is None else [im1, im2]
        x = torch.empty(sum(im.shape[0] for im in ims), hs, ws, cstore(3, dt), dtype=torch_dtype(dt), device=im1.device)
        off = 0
        for im in ims:
            ops.resize_image(im, x, off)
            off += im.shape[0]
        return x

    def _black(self, ims, hs, ws):
        """the black-pixel masks of the match() tail (dkm.py:726-729), one per image: uint8 [sum B_i, hs, ws]"""
        return torch.stack([ops.dkm_black_mask(im[b:b + 1], (hs, ws)) for im in ims for b in range(im.shape[0])])

    # ---- weight / device changes move the epoch of the per-image state ----------------------------------------------------------------
    def load_state_dict(self, state_dict, *a, **k):
        self._epoch = getattr(self, "_epoch", 0) + 1
        return super().load_state_dict(state_dict, *a, **k)

    def _apply(self, fn, *a, **k):
        self._epoch = getattr(self, "_epoch", 0) + 1
        return super()._apply(fn, *a, **k)

    def _ensure_packed(self, device):
        if self._packed is None or self._packed[2] != device or self._packed[1] != PRECISION_DTYPE[self.precision]:
            self._prepack(device)
        return self._packed[0], self._packed[1]

    def _tag_extra(self):
        return ()

    def feature_tag(self):
        """what per-image state depends on besides the image: weights (epoch), precision, the two resolutions and the engine's switches.
        A DenseFeatureBank holds state of ONE tag."""
        return (id(self), self._epoch, self.precision, self.h_resized, self.w_resized, bool(self.upsample_preds),
                tuple(self.upsample_res) if self.upsample_preds else None) + tuple(self._tag_extra())

    def _out_size(self):
        return tuple(self.upsample_res) if self.upsample_preds else (self.h_resized, self.w_resized)

    # ---- per-image state: extract once, match many times ---------------------------------------------------------------------------------
    @torch.no_grad()
    def extract(self, images):
        """[N,3,H,W] images, padded and masked as match() gets them -> DenseFeatures: everything match_batch computes from ONE image
        alone, at the module's precision, as tensors with a leading N -- the low-resolution levels `_decode` reads (the coarse scales as
        their projections), the high-resolution levels of the upsampling pass (scales 8, 4, 2, 1 only) and the black-pixel mask of the
        match() tail.  gim_amd.dense_bank.DenseFeatureBank stores them; `match_features` matches pairs of stored images."""
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise GimHipError(f"extract takes [N,3,H,W] images, got {tuple(getattr(images, 'shape', ()))}")
        if not images.is_cuda:
            raise GimHipError(f"gim_amd {self.engine} needs device (cuda/HIP) tensors: there is no CPU fallback")
        if not self.symmetric:
            raise NotImplementedError("only symmetric matching is built")
        P, dt = self._ensure_packed(images.device)
        st = self._state(P, dt, images.contiguous().float(), None)
        return DenseFeatures({k: v for k, v in st.items() if not k.endswith(".rows")}, self.feature_tag())

    def _pair_index(self, slots0, slots1, n_slots, device):
        if torch.is_tensor(slots0) != torch.is_tensor(slots1):
            raise GimHipError("match_features: slots0 and slots1 must both be sequences of ints or both int32 device tensors")
        if torch.is_tensor(slots0):
            if slots0.dtype != torch.int32 or slots1.dtype != torch.int32 or slots0.device != device or slots1.device != device:
                raise GimHipError(f"match_features: slot tensors must be int32 on {device}")
            s0, s1 = slots0.reshape(-1), slots1.reshape(-1)
        else:
            s0, s1 = [int(v) for v in slots0], [int(v) for v in slots1]
            bad = [v for v in s0 + s1 if not 0 <= v < n_slots]
            if bad:
                raise GimHipError(f"match_features: slot {bad[0]} is outside [0, {n_slots})")
            both = torch.tensor(s0 + s1 + s1 + s0, dtype=torch.int32).to(device, non_blocking=True)
            B = len(s0)
            if len(s1) != B:
                raise GimHipError(f"match_features: {B} slots on side 0, {len(s1)} on side 1")
            return B, both[:2 * B], both[2 * B:]
        if s0.numel() != s1.numel():
            raise GimHipError(f"match_features: {s0.numel()} slots on side 0, {s1.numel()} on side 1")
        return s0.numel(), torch.cat((s0, s1)), torch.cat((s1, s0))

    @torch.no_grad()
    def match_features(self, bank, slots0, slots1):
        """`match_batch` from stored state: pair b matches the images in slots0[b] / slots1[b] of `bank` (a DenseFeatureBank of this
        module) -> (warp [B,Hs,2Ws,4], certainty [B,Hs,2Ws]), B <= max_batch.  Two gim_dense_gather_pairs launch sequences build the
        query batch (slots0 | slots1) and the support batch (slots1 | slots0) of every level; everything behind them is match_batch's."""
        bank.check(self)                       # raises for another module's bank, empties a stale one (then the slots name nothing)
        if bank.slabs is None:
            raise GimHipError("match_features: the bank is empty (never filled, or invalidated by a weight / device / precision change)")
        dev = bank.device
        P, dt = self._ensure_packed(dev)
        B, iq, isup = self._pair_index(slots0, slots1, bank.capacity, dev)
        if not 1 <= B <= self.max_batch:
            raise GimHipError(f"match_features takes 1..{self.max_batch} pairs per call, got {B}")
        q, sup = {}, {}

        def gather(names, idx, out):
            levels = []
            for nm in names:
                slab = bank.slabs[nm]
                if nm in self.slack_names:   # GEMM operand rows: 64 zero rows behind the last image
                    rows = torch.zeros(2 * B * slab.shape[1] + 64, slab.shape[2], dtype=slab.dtype, device=dev)
                    out[nm + ".rows"] = rows
                    out[nm] = rows[:2 * B * slab.shape[1]].view(2 * B, *slab.shape[1:])
                else:
                    out[nm] = torch.empty(2 * B, *slab.shape[1:], dtype=slab.dtype, device=dev)
                levels.append((slab, out[nm]))
            ops.dense_gather_pairs(levels, idx, bank.capacity)

        first = [nm for nm in bank.slabs if nm in self.first_names]
        gather(first, iq, q)
        pending = self._begin(P, dt, q, B)
        gather([nm for nm in bank.slabs if nm not in self.first_names], iq, q)
        gather([nm for nm in bank.slabs if nm in self.support_names], isup, sup)
        out = self._match_state(P, dt, q, sup, B, pending)
        return self._after_match(out, lambda: self.match_features(bank, slots0, slots1))

    first_names = ()      # state the work of `_begin` reads (gathered first)
    support_names = ()    # state the refiners read as the OTHER image of the pair
    slack_names = ()      # state that is a GEMM row operand (64 slack rows)

    def _begin(self, P, dt, q, B):
        return None

    def _after_match(self, out, again):
        return out

    def _finish(self, im1, im2, flow, cert, low, hs, ws):
        """`_finish_state` with the black masks computed from the two image batches"""
        return DenseMatcher._finish_state(self, DenseMatcher._black(self, [im1, im2], hs, ws), flow, cert, low, hs, ws)

    def _finish_state(self, black, flow, cert, low, hs, ws):
        """tail of match_batch (dkm.py:686-752, roma.py:880-917): flow / cert / low [2B,hs,ws,*] of both directions and the black masks
        [2B,hs,ws] of the images -> (warp [B,hs,2ws,4], certainty [B,hs,2ws])"""
        B, dev = flow.shape[0] // 2, flow.device
        warp = torch.empty(B, hs, 2 * ws, 4, dtype=torch.float32, device=dev)
        certainty = torch.empty(B, hs, 2 * ws, dtype=torch.float32, device=dev)
        for b in range(B):
            ops.dkm_match_post((flow[b], flow[b + B]), (cert[b], cert[b + B]), (low[b], low[b + B]), black[b], black[b + B], warp[b], certainty[b])
        return warp, certainty

    @torch.no_grad()
    def match_batch(self, ims1, ims2):
        """B independent pairs in one pass ([B,3,H,W] x 2 -> warp [B,Hs,2Ws,4], certainty [B,Hs,2Ws]); result b equals
        `match(ims1[b:b+1], ims2[b:b+1])`.  (The reference's own batched mode cannot upsample and masks with pair 0's black pixels,
        dkm.py:662,723-724; batching here is the engine's, as SURVEY 8d prescribes for the batch-4 config.)  It is "extract both, then
        the body `match_features` shares": one decode path."""
        P, dt, im1, im2 = self._enter(ims1, ims2)
        B = im1.shape[0]
        pending = []
        st = self._state(P, dt, im1, im2, after_low=lambda q: pending.append(self._begin(P, dt, q, B)))
        out = self._match_state(P, dt, st, None, B, pending[0] if pending else None)
        return self._after_match(out, lambda: self.match_batch(ims1, ims2))

    @torch.no_grad()
    def match(self, im1, im2, *args, batched=False):
        """RegressionMatcher.match (dkm.py:654-752, roma.py:816-917), tensor inputs as gim calls it (`demo.py:433`,
        `lightning.py:135`): [1,3,H,W] x 2 -> (warp [Hs, 2Ws, 4], certainty [Hs, 2Ws])."""
        if batched or not self.symmetric:
            raise NotImplementedError(f"gim runs {self.engine} symmetric and non-batched (lightning.py:30-37); use match_batch for several pairs")
        if im1.dim() != 4 or im1.shape[0] != 1:
            raise GimHipError(f"match() takes [1,3,H,W] images, got {tuple(im1.shape)}")
        warp, certainty = self.match_batch(im1, im2)
        return warp[0], certainty[0]

    def _enter(self, im1, im2):
        """head of match_batch: argument checks, packing on demand -> (P, dt, im1, im2 as contiguous fp32)"""
        if not self.symmetric:
            raise NotImplementedError("only symmetric matching is built")
        if not im1.is_cuda:
            raise GimHipError(f"gim_amd {self.engine} needs device (cuda/HIP) tensors: there is no CPU fallback")
        if im1.dim() != 4 or im1.shape[1] != 3 or im1.shape != im2.shape or not 1 <= im1.shape[0] <= self.max_batch:
            raise GimHipError(f"match takes two [B,3,H,W] batches of equal shape with B <= {self.max_batch}, "
                              f"got {tuple(im1.shape)} / {tuple(im2.shape)}")
        P, dt = self._ensure_packed(im1.device)
        return P, dt, im1.contiguous().float(), im2.contiguous().float()

    @torch.no_grad()
    def sample(self, dense_matches, dense_certainty, num=10000):
        """RegressionMatcher.sample (dkm.py:583-620, roma.py:680-714).  The two multinomial draws are `gim_weighted_sample` (seeded
        from torch's generator), the balanced-sampling density is the HIP KDE kernel; samples come back as an unordered set."""
        return balanced_sample(dense_matches, dense_certainty, num, self.sample_mode, self.sample_thresh, kde_half=self.kde_half)

    @torch.no_grad()
    def sample_batch(self, dense_matches, dense_certainty, num=10000):
        """`sample()` of B pairs at once: dense_matches [B,H,2W,4], dense_certainty [B,H,2W] (what `match_batch` / `match_features`
        return) -> (sparse [B,num,4], mconf [B,num], count int32 [B]), all on the device and with no synchronisation.  Pair b's first
        count[b] rows are the rows of `sample(dense_matches[b], dense_certainty[b], num)`, bit for bit and in its order; the rows behind
        them are zero (mconf 0).  The seeds are drawn from torch's CPU generator as B successive `sample()` calls draw them, so
        `torch.manual_seed` reproduces the batch and leaves the generator where those calls leave it.  One fixed launch sequence per
        ops.SAMPLE_MAX_PAIRS pairs (gim_balanced_sample_pairs); the workspace is kept on the module per (B, n, num)."""
        if "threshold" not in self.sample_mode or "balanced" not in self.sample_mode:
            raise NotImplementedError("gim uses sample_mode='threshold_balanced' (DKMv3.py:5, roma.py:645)")
        if dense_certainty.dim() != 3 or dense_matches.shape != dense_certainty.shape + (4,) or dense_certainty.shape[0] < 1:
            raise GimHipError(f"sample_batch takes matches [B,H,2W,4] and certainty [B,H,2W], got {tuple(dense_matches.shape)} / "
                              f"{tuple(dense_certainty.shape)}")
        B, dev = dense_certainty.shape[0], dense_certainty.device
        n = dense_certainty[0].numel()
        seeds = [torch.randint(0, 2 ** 31 - 1, (2,)).tolist() for _ in range(B)]     # pair order: the stream of B sample() calls
        sparse = torch.empty(B, num, 4, dtype=torch.float32, device=dev)
        mconf = torch.empty(B, num, dtype=torch.float32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        cache = self.__dict__.setdefault("_sample_ws", {})
        for lo in range(0, B, ops.SAMPLE_MAX_PAIRS):
            hi = min(B, lo + ops.SAMPLE_MAX_PAIRS)
            key = (hi - lo, n, num, str(dev))
            if key not in cache:
                cache[key] = torch.empty(ops.balanced_sample_pairs_ws_bytes(hi - lo, n, num), dtype=torch.uint8, device=dev)
            ops.balanced_sample_pairs(dense_matches[lo:hi], dense_certainty[lo:hi], seeds[lo:hi], num, self.sample_thresh, self.kde_half,
                                      ws=cache[key], out=(sparse[lo:hi], mconf[lo:hi], count[lo:hi]))
        return sparse, mconf, count


@torch.no_grad()
def balanced_sample(dense_matches, dense_certainty, num, sample_mode, sample_thresh, kde_half):
    """`sample()` of both dense matchers (dkm.py:583-620, roma.py:680-714): certainty above the threshold counts as 1, draw
    4 * num matches without replacement, re-draw num of them with weights 1 / (1 + KDE density)."""
    if "threshold" not in sample_mode or "balanced" not in sample_mode:
        raise NotImplementedError("gim uses sample_mode='threshold_balanced' (DKMv3.py:5, roma.py:645)")
    cert_ = dense_certainty.reshape(-1).contiguous()
    matches = dense_matches.reshape(-1, 4)
    cert = torch.where(cert_ > sample_thresh, torch.ones_like(cert_), cert_)   # dense_certainty[> thresh] = 1
    n_pos = int((cert > 0).sum())
    if n_pos == 0:
        cert, n_pos = cert + 1e-8, cert.numel()
    seeds = torch.randint(0, 2 ** 31 - 1, (2,)).tolist()      # torch's (CPU) generator: torch.manual_seed makes sample() reproducible
    # the kernel returns an unordered set (atomic compaction); sorting makes sample() reproducible from the seed
    good = ops.weighted_sample(cert, min(4 * num, cert.numel(), n_pos), seeds[0]).sort().values
    gm, gc = matches[good].contiguous(), cert_[good]
    density = ops.kde(gm, 0.1, half=kde_half)
    p = torch.where(density < 10, torch.full_like(density, 1e-7), 1 / (density + 1))
    bal = ops.weighted_sample(p.contiguous(), min(num, len(gc)), seeds[1]).sort().values
    return gm[bal], gc[bal]


@torch.no_grad()
def gim_dkm_inference(model, data, num=5000):
    """`Trainer.gim_dkm_inference` (trainer/lightning.py:134-156; the same adapter serves gim_roma, lightning.py:125): match + sample +
    pixel coordinates + `mconf > 0` filter, written into `data` (hw0_i, hw1_i, mkpts0_f, mkpts1_f, m_bids, mconf).  data: color0 /
    color1 [1,3,H,W], imsize0 / imsize1 [1,2] = (height, width) of the un-padded images."""
    dense_matches, dense_certainty = model.match(data["color0"], data["color1"])
    sparse_matches, mconf = model.sample(dense_matches, dense_certainty, num)
    h0, w0 = (float(v) for v in data["imsize0"][0])
    h1, w1 = (float(v) for v in data["imsize1"][0])
    kpts0, kpts1 = ops.dense_to_pixels(sparse_matches, (h0, w0), (h1, w1))
    mask = mconf > 0
    data.update({"hw0_i": data["color0"].shape[2:], "hw1_i": data["color1"].shape[2:], "mkpts0_f": kpts0[mask], "mkpts1_f": kpts1[mask],
                 "m_bids": torch.where(mconf[None])[0], "mconf": mconf[mask]})
