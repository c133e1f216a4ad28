"""gim_roma on MI355X: the reference's `RoMa(img_size=[672])` / `RegressionMatcher` surface
(`networks/roma/roma.py:636-917, 1124-1266`) over hand-written HIP.

Drop-in contract:
  * `RoMa(img_size, **kwargs)` returns a module whose `state_dict()` has the reference's tensors (`encoder.cnn.layers.*`
    = torchvision vgg19_bn.features[:40], `decoder.embedding_decoder.*`, `decoder.gps.16.*`, `decoder.proj.*`,
    `decoder.conv_refiner.*`), so gim_roma checkpoints load with the reference's prefix rule (`demo.py:365-371`);
  * the DINOv2 ViT-L/14 weights are NOT part of that state_dict in the reference either (`self.dinov2_vitl14 =
    [dinov2_vitl14]`, roma.py:612); the reference downloads them inside the constructor, this module takes them as a
    plain state dict: `RoMa(img_size, dinov2_weights=sd)` or `model.load_dinov2(sd)` (names of `dino.py`'s
    `vit_large`: cls_token, pos_embed, patch_embed.proj.*, blocks.N.*, norm.*);
  * `h_resized, w_resized, upsample_preds, upsample_res, symmetric, sample_thresh, attenuate_cert` are plain
    attributes read at call time;
  * `match(im_A, im_B)` takes [1,3,H,W] fp32 tensors and returns `(warp [Hs, 2Ws, 4], certainty [Hs, 2Ws])`,
    `sample(dense_matches, dense_certainty, num)` returns `([n,4], [n])` like roma.py:680-714.
  * built: symmetric, non-batched matching with or without the upsampling pass (what gim runs).

Every stage of `match()` is a libgimhip launch: VGG / patch-embed / 1x1 convolutions and all Linear layers of the two
transformers on the implicit-GEMM kernel (LayerScale folded into proj / fc2, the residual add in its epilogue, exact
GELU in fc1's epilogue), attention on the flash SDPA kernel (DINOv2 16 x 64, decoder 8 x 128), the GP on the fp32-MFMA
products + fp64 Cholesky of `csrc/gp_solve.hip`, the refiners on `csrc/dkm.hip`.  Constant tables (bicubic-resized
position embedding, the GP's Fourier features) are built once per shape on the host with the reference's own fp32 ops.
No CPU / eager fallback.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import ACT_GELU, ACT_NONE, ACT_RELU, GIM_F32, GimHipError
from ..dense import (GP, ConvRefiner, DenseMatcher, _bn_after_bias, gim_dkm_inference, gp_features, gp_posterior, pack_refiner, refine,
                     refiner_dims)
from ..packing import PRECISION_DTYPE, cstore, pack_conv, torch_dtype
from ..precision import resolve as resolve_precision

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M"]      # vgg19_bn.features[:40]
REFINER = {"16": (512, 128, 7), "8": (512, 64, 3), "4": (256, 32, 2), "2": (64, 16, None), "1": (9, 6, None)}
PROJ = {"16": (1024, 512), "8": (512, 512), "4": (256, 256), "2": (128, 64), "1": (64, 9)}
GP_DIM, DEC_DIM, DEC_HEADS, DEC_BLOCKS, CLS_RES = 512, 1024, 8, 5, 64
VIT_DIM, VIT_DEPTH, VIT_HEADS, VIT_PATCH, VIT_GRID = 1024, 24, 16, 14, 37                      # vit_large, img_size 518


# ---------------------------------------------------------------------------------------- parameter containers
class _VGG19(nn.Module):
    def __init__(self):
        super().__init__()
        layers, ci = [], 3
        for v in VGG_CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(ci, v, 3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
                ci = v
        self.layers = nn.ModuleList(layers)


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.cnn = _VGG19()


class _Attention(nn.Module):
    def __init__(self, dim, qkv_bias):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)


class _Block(nn.Module):
    """dino.py:114-168 `Block(dim, heads)` as the decoder builds it: qkv_bias=False, no LayerScale"""

    def __init__(self, dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _Attention(dim, False)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim)


class _TransformerDecoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = nn.Sequential(*[_Block(DEC_DIM) for _ in range(DEC_BLOCKS)])
        self.to_out = nn.Linear(DEC_DIM, CLS_RES ** 2 + 1)


class _Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.embedding_decoder = _TransformerDecoder()
        self.gps = nn.ModuleDict({"16": GP(GP_DIM)})
        self.proj = nn.ModuleDict({s: nn.Sequential(nn.Conv2d(ci, co, 1, 1), nn.BatchNorm2d(co)) for s, (ci, co) in PROJ.items()})
        self.conv_refiner = nn.ModuleDict({s: ConvRefiner(*refiner_dims(REFINER, s), REFINER[s][1], bn_momentum=0.01) for s in REFINER})


class _Workspace:
    """scratch rows of one transformer pass (activation dtype T): LayerNorm output, qkv, V^T, attention output, MLP hidden"""

    def __init__(self, nb, n, dim, tdt, dev):
        R = nb * n
        self.Sp = (n + 63) // 64 * 64
        self.xn = torch.empty(R, dim, dtype=tdt, device=dev)
        self.qkv = torch.empty(R, 3 * dim, dtype=tdt, device=dev)
        self.vt = torch.empty(nb, dim, self.Sp, dtype=tdt, device=dev)
        self.att = torch.empty(R, dim, dtype=tdt, device=dev)
        self.hid = torch.empty(R, 4 * dim, dtype=tdt, device=dev)


class RegressionMatcher(DenseMatcher):
    engine, max_batch, kde_half = "RoMa", 4, True      # the KDE of sample() runs on fp16-rounded coordinates like roma.py:1018-1023

    def __init__(self, h=448, w=448, sample_mode="threshold_balanced", upsample_preds=True, symmetric=True, name=None,
                 attenuate_cert=True, precision=None, dinov2_weights=None):
        super().__init__(h, w, sample_mode, upsample_preds, symmetric, name)
        self.attenuate_cert = attenuate_cert
        self.encoder = _Encoder()
        self.decoder = _Decoder()
        self.upsample_res = (14 * 16 * 6, 14 * 16 * 6)
        # round 6: IEEE fp16 is gim_roma's default 16-bit mode (gim_amd/precision.py has the argument; bf16 moves the warp by ~3 px at 560 x 560,
        # fp16 stays < 5e-6 of scale from the fp32 mode: tests/test_gpu_roma.py, tests/test_gpu_dense_fullsize.py); `_fp16_checked` = the
        # output check of match_batch below has passed once for the current weights
        self.precision = resolve_precision(precision, "gim_roma", default="fp16")
        self._fp16_default = precision is None and self.precision == "fp16"
        self._fp16_checked = False
        self._dino = [None]          # a list, like roma.py:612: the ViT is not a registered sub-module / not in state_dict()
        self._tables = {}
        if dinov2_weights is not None:
            self.load_dinov2(dinov2_weights)

    # ---- weights -------------------------------------------------------------------------------------------------
    def load_dinov2(self, state_dict):
        """DINOv2 ViT-L/14 weights by `dino.py` name; replaces the download of roma.py:596-604."""
        need = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias"]
        for i in range(VIT_DEPTH):
            need += [f"blocks.{i}.{k}" for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                                                "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight",
                                                "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma")]
        missing = [k for k in need if k not in state_dict]
        if missing:
            raise GimHipError(f"DINOv2 weights: {len(missing)} tensors missing, e.g. {missing[:3]}")
        if tuple(state_dict["pos_embed"].shape) != (1, VIT_GRID ** 2 + 1, VIT_DIM):
            raise GimHipError(f"DINOv2 weights: pos_embed {tuple(state_dict['pos_embed'].shape)} is not ViT-L/14 @518")
        self._dino[0] = {k: state_dict[k].detach().float().cpu() for k in need}
        self._epoch += 1
        self._fp16_checked = False
        self._packed = None
        self._tables = {}

    def load_state_dict(self, state_dict, *a, **k):
        self._packed = None
        self._fp16_checked = False
        self._tables = {}
        return super().load_state_dict(state_dict, *a, **k)

    def _apply(self, fn, *a, **k):
        self._packed = None
        self._tables = {}
        return super()._apply(fn, *a, **k)

    def get_output_resolution(self):
        return self.upsample_res if self.upsample_preds else (self.h_resized, self.w_resized)

    # ---- one-time packing ----------------------------------------------------------------------------------------
    @staticmethod
    def _pack_block(P, p, dt, device, n1, qkv_w, qkv_b, proj_w, proj_b, n2, fc1_w, fc1_b, fc2_w, fc2_b, ls1=None, ls2=None):
        f = lambda t: t.detach().float().contiguous().to(device)  # noqa: E731
        P[p + "n1"], P[p + "n2"] = (f(n1[0]), f(n1[1])), (f(n2[0]), f(n2[1]))
        P[p + "qkv"] = pack_conv(qkv_w, None, dt, device, bias=qkv_b)
        if ls1 is not None:     # LayerScale (dino.py:155-160): x + gamma * f(x) -> gamma folded into the producing Linear
            proj_w, proj_b = proj_w.detach().float() * ls1.float()[:, None], proj_b.detach().float() * ls1.float()
            fc2_w, fc2_b = fc2_w.detach().float() * ls2.float()[:, None], fc2_b.detach().float() * ls2.float()
        P[p + "proj"] = pack_conv(proj_w, None, dt, device, bias=proj_b)
        P[p + "fc1"] = pack_conv(fc1_w, None, dt, device, bias=fc1_b)
        P[p + "fc2"] = pack_conv(fc2_w, None, dt, device, bias=fc2_b)

    def _prepack(self, device):
        if self._dino[0] is None:
            raise GimHipError("RoMa needs the DINOv2 ViT-L/14 weights: RoMa(img_size, dinov2_weights=sd) or model.load_dinov2(sd)")
        dt = PRECISION_DTYPE[self.precision]
        P = {}
        layers = self.encoder.cnn.layers
        idx = 0
        for v in VGG_CFG:
            if v == "M":
                idx += 1
                continue
            conv, bn = layers[idx], layers[idx + 1]
            P[f"vgg{idx}"] = pack_conv(conv.weight, _bn_after_bias(bn, conv.bias), dt, device, pad=1,
                                       cin_pad=cstore(conv.in_channels, dt))
            idx += 3
        d = self._dino[0]
        P["patch"] = pack_conv(d["patch_embed.proj.weight"], None, dt, device, stride=VIT_PATCH, cin_pad=cstore(3, dt),
                               bias=d["patch_embed.proj.bias"])
        for i in range(VIT_DEPTH):
            b = f"blocks.{i}."
            self._pack_block(P, f"vit{i}.", dt, device, (d[b + "norm1.weight"], d[b + "norm1.bias"]), d[b + "attn.qkv.weight"],
                             d[b + "attn.qkv.bias"], d[b + "attn.proj.weight"], d[b + "attn.proj.bias"],
                             (d[b + "norm2.weight"], d[b + "norm2.bias"]), d[b + "mlp.fc1.weight"], d[b + "mlp.fc1.bias"],
                             d[b + "mlp.fc2.weight"], d[b + "mlp.fc2.bias"], d[b + "ls1.gamma"], d[b + "ls2.gamma"])
        P["vit.norm"] = (d["norm.weight"].to(device), d["norm.bias"].to(device))
        dec = self.decoder
        for i, blk in enumerate(dec.embedding_decoder.blocks):
            self._pack_block(P, f"dec{i}.", dt, device, (blk.norm1.weight, blk.norm1.bias), blk.attn.qkv.weight, blk.attn.qkv.bias,
                             blk.attn.proj.weight, blk.attn.proj.bias, (blk.norm2.weight, blk.norm2.bias), blk.mlp.fc1.weight,
                             blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
        to_out = dec.embedding_decoder.to_out
        P["to_out"] = pack_conv(to_out.weight, None, dt, device, bias=to_out.bias)
        for s, seq in dec.proj.items():
            P["proj" + s] = pack_conv(seq[0].weight, _bn_after_bias(seq[1], seq[0].bias), dt, device)
        for s, ref in dec.conv_refiner.items():
            pack_refiner(P, s, ref, *refiner_dims(REFINER, s), dt, device)
        self._packed = (P, dt, device)

    def _gp_features(self, h, w, device):
        """f = cos(8 pi pos_conv(coords)) of GP.get_pos_enc (roma.py:94-108): constant per (h, w); built once on the host
        with the reference's fp32 ops, cached on the device as rows [h*w, 512]."""
        key = ("gp", h, w, str(device))
        if key not in self._tables:
            self._tables[key] = gp_features(self.decoder.gps["16"].pos_conv, h, w, GP_DIM).to(device)
        return self._tables[key]

    def _pos_table(self, hs, ws, device):
        """interpolate_pos_encoding (dino.py:457-488) -> (cls row [1024] = cls_token + pos[0], patch rows [h0*w0, 1024]).
        The reference passes (w, h) = x.shape[2:] = (H, W), so the bicubic scale factors are ((h0 + .1) / 37, (w0 + .1) / 37)
        on the (row, column) axes of the 37 x 37 table."""
        key = ("pos", hs, ws, str(device))
        if key not in self._tables:
            d = self._dino[0]
            pe = d["pos_embed"]
            h0, w0 = hs // VIT_PATCH, ws // VIT_PATCH
            if h0 * w0 == VIT_GRID ** 2 and hs == ws:
                patch = pe[0, 1:]
            else:
                g = VIT_GRID
                patch = F.interpolate(pe[:, 1:].reshape(1, g, g, -1).permute(0, 3, 1, 2),
                                      scale_factor=((h0 + 0.1) / g, (w0 + 0.1) / g), mode="bicubic")
                assert patch.shape[-2:] == (h0, w0)
                patch = patch.permute(0, 2, 3, 1).reshape(h0 * w0, -1)
            self._tables[key] = ((d["cls_token"][0, 0] + pe[0, 0]).contiguous().to(device), patch.contiguous().to(device))
        return self._tables[key]

    # ---- stages ---------------------------------------------------------------------------------------------------
    def _vgg(self, P, x):
        """VGG19.forward (roma.py:144-152): activations before each max-pool -> {1: 64, 2: 128, 4: 256, 8: 512 channels}"""
        feats, scale, idx = {}, 1, 0
        for v in VGG_CFG:
            if v == "M":
                feats[scale] = x
                scale *= 2
                if scale <= 8:
                    x = ops.maxpool2x2(x)
                idx += 1
                continue
            x = ops.conv2d(x, P[f"vgg{idx}"], ACT_RELU)
            idx += 3
        return feats

    @staticmethod
    def _vit_block(P, p, x32, ws, nb, n, heads, eps):
        """one pre-norm transformer block (dino.py:143-168, eval) on the fp32 residual stream x32 [nb*n, C], in place"""
        C = x32.shape[1]
        R = nb * n
        ops.layernorm_act(x32, *P[p + "n1"], ws.xn, ACT_NONE, eps)
        ops.linear(ws.xn, P[p + "qkv"], ws.qkv)
        ops.lg_transpose(ws.qkv[:, 2 * C:], ws.vt, nb, n, ws.Sp, C)
        ops.sdpa(ws.qkv[:, :C], ws.qkv[:, C:2 * C], ws.vt, ws.att, nb, heads, n, n, ws.Sp, D=C // heads)
        ops.conv_rows(ws.att, P[p + "proj"], (1, 1, R, 1, R), x32, ACT_NONE, x32)           # x += [ls1 *] proj(attn)
        ops.layernorm_act(x32, *P[p + "n2"], ws.xn, ACT_NONE, eps)
        ops.linear(ws.xn, P[p + "fc1"], ws.hid, ACT_GELU)
        ops.conv_rows(ws.hid, P[p + "fc2"], (1, 1, R, 1, R), x32, ACT_NONE, x32)            # x += [ls2 *] fc2(gelu(fc1))

    def _dino_features(self, P, dt, x):
        """forward_features(x)['x_norm_patchtokens'] (dino.py:490-540, roma.py:624-631): x NHWC [nb,hs,ws,cpad] ->
        [nb, hs/14, ws/14, 1024]"""
        tdt = torch_dtype(dt)
        nb, hs, ws, cp = x.shape
        if hs % VIT_PATCH or ws % VIT_PATCH:
            raise GimHipError(f"h_resized / w_resized must be multiples of {VIT_PATCH} (DINOv2 patch size), got {(hs, ws)}")
        dev = x.device
        h0, w0 = hs // VIT_PATCH, ws // VIT_PATCH
        n = h0 * w0 + 1
        cls_row, pos = self._pos_table(hs, ws, dev)
        tok = torch.empty(nb, n, VIT_DIM, dtype=torch.float32, device=dev)
        tok[:, 0] = cls_row
        for b in range(nb):      # patch embedding (14x14 / stride 14 conv) + position rows in the epilogue's residual add
            ops.conv_rows(x[b].view(hs * ws, cp), P["patch"], (1, hs, ws, h0, w0), tok[b, 1:], ACT_NONE, pos)
        x32 = tok.view(nb * n, VIT_DIM)
        wsp = _Workspace(nb, n, VIT_DIM, tdt, dev)
        for i in range(VIT_DEPTH):
            self._vit_block(P, f"vit{i}.", x32, wsp, nb, n, VIT_HEADS, 1e-6)
        feat = torch.empty(nb, h0, w0, VIT_DIM, dtype=tdt, device=dev)
        for b in range(nb):
            ops.layernorm_act(tok[b, 1:], *P["vit.norm"], feat[b].view(h0 * w0, VIT_DIM), ACT_NONE, 1e-6)
        return feat

    def _encode(self, P, dt, x, upsample=False):
        """CNNandDinov2.forward (roma.py:617-633)"""
        feats = self._vgg(P, x)
        if not upsample:
            feats[16] = self._dino_features(P, dt, x)
        return feats

    def _project(self, P, dt, feat, s, out32=False):
        """proj[s] = 1x1 conv + BatchNorm (roma.py:1220-1234) -> NHWC [nb,h,w,cstore(co)]"""
        nb, h, w, _ = feat.shape
        if not out32:
            return ops.conv2d(feat, P["proj" + s])
        a32 = torch.zeros(nb * h * w + 64, P["proj" + s].n_store, dtype=torch.float32, device=feat.device)
        ops.linear(feat.view(nb * h * w, feat.shape[3]), P["proj" + s], a32)
        return a32

    def _gp(self, a32, nb, h, w, out):
        """GP.forward (dense.gp_posterior): a32 fp32 rows [nb*hw (+64 slack), 512] -> mu into `out` (row view [nb*hw, 512])"""
        gp_posterior(a32, nb, h, w, self._gp_features(h, w, a32.device), out, self._gp_is_exact())

    def _coarse(self, P, dt, a32, nb, h, w):
        """scale 16 of Decoder.forward behind its projection (roma.py:263-296): a32 = the fp32 proj16 rows [nb*hw + 64 slack, 512] of
        the stacked pair batch -> GP -> TransformerDecoder -> cls_to_flow_refine -> (flow [nb,h,w,2], certainty [nb,h,w,1])"""
        tdt = torch_dtype(dt)
        n, dev = h * w, a32.device
        x32 = torch.empty(nb * n, DEC_DIM, dtype=torch.float32, device=dev)
        self._gp(a32, nb, h, w, x32[:, :GP_DIM])
        ops.cast_rows(a32[:nb * n], x32[:, GP_DIM:])                       # tokens = cat(gp_posterior, features)
        wsp = _Workspace(nb, n, DEC_DIM, tdt, dev)
        for i in range(DEC_BLOCKS):
            self._vit_block(P, f"dec{i}.", x32, wsp, nb, n, DEC_HEADS, 1e-5)
        ops.cast_rows(x32, wsp.xn)
        logits = torch.empty(nb * n, P["to_out"].n_store, dtype=torch.float32, device=dev)
        ops.linear(wsp.xn, P["to_out"], logits)
        return ops.cls_to_flow(logits, nb, h, w, CLS_RES ** 2)

    def _refine(self, P, s, dt, x, y, flow, cert, ins, full_hw, scale_factor):
        refine(P, s, dt, x, y, flow, cert, ins, full_hw, REFINER[s], self.refiner_fused, emb_scale=40.0 / 32.0 * scale_factor,
               roma_layout=True)

    support_names = ("lo1", "lo2", "lo4", "lo8", "a16", "hi1", "hi2", "hi4", "hi8")
    slack_names = ("a32_16",)

    def _tag_extra(self):
        return (id(self._dino[0]),)

    def _state(self, P, dt, im1, im2, after_low=None):
        """everything match_batch computes from one image alone, for the images of im1 (and im2 behind them): {kind: [nb, ...]}
          lo1 / lo2 / lo4 / lo8     proj[s] of the low-resolution VGG levels -- what the refiners read, smaller than what it projects
          a32_16                    proj16 of the DINOv2 tokens as fp32 rows (GP and decoder tokens; `.rows`: with the 64 slack rows)
          a16                       the same at the module's precision (refiner 16)
          hi1 / hi2 / hi4 / hi8     proj[s] of the upsampling pass's VGG levels
          black                     the black-pixel mask of the match() tail at the output resolution"""
        tdt = torch_dtype(dt)
        st = {}
        feats = self._encode(P, dt, self._images(dt, im1, im2, self.h_resized, self.w_resized))
        for sc in (1, 2, 4, 8):
            st[f"lo{sc}"] = self._project(P, dt, feats[sc], str(sc))
        nb, h, w, _ = feats[16].shape
        a32 = self._project(P, dt, feats[16], "16", out32=True)
        st["a32_16"], st["a32_16.rows"] = a32[:nb * h * w].view(nb, h * w, 512), a32
        if dt == GIM_F32:
            st["a16"] = a32[:nb * h * w].view(nb, h, w, 512)
        else:
            st["a16"] = torch.empty(nb, h, w, 512, dtype=tdt, device=a32.device)
            ops.cast_rows(a32[:nb * h * w], st["a16"].view(nb * h * w, 512))
        del feats
        if after_low is not None:
            after_low(st)
        if self.upsample_preds:
            feats = self._encode(P, dt, self._images(dt, im1, im2, *self.upsample_res), upsample=True)
            for sc in (1, 2, 4, 8):
                st[f"hi{sc}"] = self._project(P, dt, feats[sc], str(sc))
        st["black"] = self._black([im1] if im2 is None else [im1, im2], *self._out_size())
        return st

    def _decode(self, P, dt, f1, upsample=False, flow=None, cert=None, scale_factor=1.0, a32=None, sup=None):
        """Decoder.forward on the symmetric pair (f2 = f1 with the two images swapped) -> {scale: (flow, certainty)}.  f1: per scale
        the PROJECTED features the refiner reads, a32: the fp32 proj16 rows of `_coarse`, sup: f1 in support order (match_features
        gathers it; None: the two halves of f1 are swapped with a copy)"""
        scales = ["8", "4", "2", "1"] if upsample else ["16", "8", "4", "2", "1"]
        sizes = {s: tuple(f1[s].shape[1:3]) for s in f1}
        full = sizes[1]
        nb = f1[1].shape[0]
        half = nb // 2
        coarsest = int(scales[0])
        if upsample:
            flow = ops.resize_bilinear(flow, sizes[coarsest])
            cert = ops.resize_bilinear(cert, sizes[coarsest])
        out = {}
        for s in scales:
            ins = int(s)
            a = f1[ins]
            if s == "16":
                flow, cert = self._coarse(P, dt, a32, nb, *sizes[16])
                out["gm"] = (flow.clone(), cert.clone())
            y = sup[ins] if sup is not None else torch.cat((a[half:], a[:half]))
            self._refine(P, s, dt, a, y, flow, cert, ins, full, scale_factor)
            out[ins] = (flow, cert)
            if s != "1":
                flow = ops.resize_bilinear(flow, sizes[ins // 2])
                cert = ops.resize_bilinear(cert, sizes[ins // 2])
        return out

    def _match_state(self, P, dt, q, sup, B, pending):
        dev = q["lo1"].device
        hs, ws = self.h_resized, self.w_resized
        f1 = {1: q["lo1"], 2: q["lo2"], 4: q["lo4"], 8: q["lo8"], 16: q["a16"]}
        y1 = None if sup is None else {1: sup["lo1"], 2: sup["lo2"], 4: sup["lo4"], 8: sup["lo8"], 16: sup["a16"]}
        cor = self._decode(P, dt, f1, a32=q["a32_16.rows"], sup=y1)
        stages = {"low": cor}
        if self.upsample_preds:
            hs, ws = self.upsample_res
        if self.attenuate_cert:
            low = ops.resize_bilinear(cor[16][1], (hs, ws))
        else:
            low = torch.zeros(2 * B, hs, ws, 1, dtype=torch.float32, device=dev)
        if self.upsample_preds:
            sf = math.sqrt(self.upsample_res[0] * self.upsample_res[1] / (self.w_resized * self.h_resized))
            f1 = {sc: q[f"hi{sc}"] for sc in (1, 2, 4, 8)}
            y1 = None if sup is None else {sc: sup[f"hi{sc}"] for sc in (1, 2, 4, 8)}
            cor = self._decode(P, dt, f1, upsample=True, flow=cor[1][0], cert=cor[1][1], scale_factor=sf, sup=y1)
            stages["high"] = cor
        flow, cert = cor[1]
        warp, certainty = self._finish_state(q["black"], flow, cert, low, hs, ws)
        self._debug = stages
        return warp, certainty

    def _after_match(self, out, again):
        """fp16 as the DEFAULT mode carries a range check of what it hands out (an explicit precision='fp16' is the caller's decision):
        every stored activation of this engine sits behind a BatchNorm / LayerNorm, so an overflow needs pathological weights -- it then
        surfaces as inf / nan in the flow or certainty logits (no ReLU between the refiners' last convolution and these outputs).  One
        reduction + host sync on the first calls after a weight change; a trip switches the module to bf16 for good and runs the call
        again (`again`: match_batch re-encodes; match_features finds its bank stale -- the precision is part of the tag -- and raises,
        the caller extracts again)."""
        warp, certainty = out
        if self._fp16_default and self.precision == "fp16" and not self._fp16_checked:
            if bool(torch.isfinite(warp).all()) and bool(torch.isfinite(certainty).all()):
                self._fp16_checked = True
            else:
                import warnings
                warnings.warn("gim_amd RoMa: non-finite outputs in the default fp16 mode (activations beyond 65504?); switching this module to bf16")
                self.precision, self._packed = "bf16", None
                return again()
        return warp, certainty


def RoMa(img_size, pretrained_backbone=False, **kwargs):
    """`networks/roma/roma.py:1124-1266`: img_size = [s] or [h, w]; kwargs go to RegressionMatcher (plus `precision`,
    `dinov2_weights`).  `pretrained_backbone` is ignored: checkpoints are loaded by the caller (`demo.py:365-371`)."""
    assert img_size is not None and isinstance(img_size, list) and len(img_size) <= 2
    if len(img_size) == 1:
        img_size = img_size * 2
    h, w = img_size
    kwargs.pop("device", None)
    return RegressionMatcher(h=h, w=w, **kwargs)


def random_dinov2_weights(dev, seed=0):
    """Synthetic ViT-L/14 weights with the magnitudes of a trained network (LayerScale ~0.2) for benchmarks -- there is no
    checkpoint in the container; generated on `dev` (300 M values), returned on the host by `dino.py` name."""
    g = torch.Generator(device=dev).manual_seed(seed)
    D = VIT_DIM

    def rn(*shape, s=1.0):
        return (torch.randn(*shape, generator=g, device=dev) * s).cpu()
    sd = {"cls_token": rn(1, 1, D, s=0.02), "pos_embed": rn(1, VIT_GRID ** 2 + 1, D, s=0.02),
          "patch_embed.proj.weight": rn(D, 3, 14, 14, s=1 / 24.0), "patch_embed.proj.bias": rn(D, s=0.02),
          "norm.weight": 1 + rn(D, s=0.1), "norm.bias": rn(D, s=0.02)}
    for i in range(VIT_DEPTH):
        b = f"blocks.{i}."
        for nm in ("norm1", "norm2"):
            sd[b + nm + ".weight"], sd[b + nm + ".bias"] = 1 + rn(D, s=0.1), rn(D, s=0.02)
        sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"] = rn(3 * D, D, s=1 / 32.0), rn(3 * D, s=0.02)
        sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"] = rn(D, D, s=1 / 32.0), rn(D, s=0.02)
        sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = rn(4 * D, D, s=1 / 32.0), rn(4 * D, s=0.02)
        sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = rn(D, 4 * D, s=1 / 64.0), rn(D, s=0.02)
        sd[b + "ls1.gamma"], sd[b + "ls2.gamma"] = 0.2 + rn(D, s=0.05), 0.2 + rn(D, s=0.05)
    return sd


@torch.no_grad()
def gim_roma_inference(model, data, num=5000):
    """`Trainer.gim_dkm_inference` (trainer/lightning.py:134-156) -- the same adapter serves gim_roma (lightning.py:125)."""
    return gim_dkm_inference(model, data, num)
