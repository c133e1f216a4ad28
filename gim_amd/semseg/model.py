"""gim_semseg on MI355X: the CSAIL ADE20K-150 segmenter that gim's SfM and video paths run before matching
(`networks/mit_semseg/models/models.py`: `ResnetDilated` :208-268 over `resnet50` of `resnet.py:95-135`, `PPMDeepsup` :438-495,
`SegmentationModule` :21-47, `ModelBuilder` :50-157).

Drop-in contract:
  * `ModelBuilder.build_encoder(arch='resnet50dilated', fc_dim=2048, weights=...)` / `build_decoder(arch='ppm_deepsup', fc_dim=2048,
    num_class=150, weights=..., use_softmax=True)` return modules with the reference's parameter names, so `encoder_epoch_20.pth` /
    `decoder_epoch_20.pth` load as the reference loads them (strict=False; the deep-supervision keys load and stay unused);
    `weights=''` keeps the module's own init -- nothing is ever downloaded;
  * `SegmentationModule(enc, dec, crit)(feed_dict, segSize=...)` returns the reference's softmax scores [B,150,H,W] (contract parity:
    it materialises the full-resolution tensor);
  * `SegmentationModule.segment(img_data, segSize)` -> uint8 class map [B,H,W] on the fast path: the full-resolution logits are never
    stored (gim_seg_head_argmax).

The nn.Module tree only holds parameters.  The forward is libgimhip launches: deep stem (3 x conv3x3 + BN + ReLU) and the bottlenecks on
the implicit GEMM (BatchNorm folded at pack time, residual + ReLU in the epilogue, dilated 3x3s through the K-group table), the PPM's
pooling / upsampling and the inference head in csrc/semseg.hip.  Layer 4's last convolution writes channels 0..2047 of the 4096-channel
concat buffer that conv_last reads; the pyramid branches fill channels 2048..4095.  No CPU / eager fallback.
"""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import ACT_NONE, ACT_RELU, GIM_F32, GimHipError
from ..packing import PRECISION_DTYPE, bn_params as _bn, cstore, pack_conv, torch_dtype
from ..precision import resolve as resolve_precision
from ..resnet50 import LAYERS, add_layers, bottleneck, pack_bottlenecks

FC_DIM, NUM_CLASS, PPM_DIM = 2048, 150, 512


def dilation_schedule(li, bi):
    """(stride, dilation) of block bi's 3x3 in layer li for dilate_scale = 8 (models.py:216-250: _nostride_dilate)"""
    if li == 2 and bi == 0:
        return 2, 1
    if li == 3:
        return 1, (1 if bi == 0 else 2)
    if li == 4:
        return 1, (2 if bi == 0 else 4)
    return 1, 1


def downsample_stride(li):
    return 2 if li == 2 else 1


def _schedule(li, bi):
    return (*dilation_schedule(li, bi), downsample_stride(li))


# ---------------------------------------------------------------------------------------- parameter containers
class ResnetDilated(nn.Module):
    """resnet50 (deep stem, inplanes 128: resnet.py:95-135) with the dilate_scale = 8 schedule, parameter names of models.py:208-233"""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = nn.Conv2d(64, 64, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(64)
        self.conv3 = nn.Conv2d(64, 128, 3, 1, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(128)
        add_layers(self, 128, _schedule)


def _cbr(ci, co, k):
    return nn.Sequential(nn.Conv2d(ci, co, k, 1, k // 2, bias=False), nn.BatchNorm2d(co), nn.ReLU(inplace=True))


class PPMDeepsup(nn.Module):
    """models.py:438-464 parameter layout: ppm.{0..3}.{1,2}, cbr_deepsup.*, conv_last.{0,1,4}, conv_last_deepsup.*"""

    def __init__(self, num_class=NUM_CLASS, fc_dim=FC_DIM, use_softmax=True, pool_scales=ops.PPM_SCALES):
        super().__init__()
        assert tuple(pool_scales) == ops.PPM_SCALES
        self.use_softmax = use_softmax
        self.num_class = num_class
        self.ppm = nn.ModuleList([nn.Sequential(nn.AdaptiveAvgPool2d(s), nn.Conv2d(fc_dim, PPM_DIM, 1, bias=False), nn.BatchNorm2d(PPM_DIM),
                                                nn.ReLU(inplace=True)) for s in pool_scales])
        self.cbr_deepsup = nn.Sequential(nn.Conv2d(fc_dim // 2, fc_dim // 4, 3, 1, 1, bias=False), nn.BatchNorm2d(fc_dim // 4), nn.ReLU(inplace=True))
        self.conv_last = nn.Sequential(nn.Conv2d(fc_dim + len(pool_scales) * PPM_DIM, PPM_DIM, 3, padding=1, bias=False),
                                       nn.BatchNorm2d(PPM_DIM), nn.ReLU(inplace=True), nn.Dropout2d(0.1), nn.Conv2d(PPM_DIM, num_class, 1))
        self.conv_last_deepsup = nn.Conv2d(fc_dim // 4, num_class, 1, 1, 0)
        self.dropout_deepsup = nn.Dropout2d(0.1)


def _weights_init(m):
    """ModelBuilder.weights_init (models.py:52-60)"""
    name = m.__class__.__name__
    if name.find("Conv") != -1:
        nn.init.kaiming_normal_(m.weight.data)
    elif name.find("BatchNorm") != -1:
        m.weight.data.fill_(1.)
        m.bias.data.fill_(1e-4)


class ModelBuilder:
    weights_init = staticmethod(_weights_init)

    @staticmethod
    def build_encoder(arch="resnet50dilated", fc_dim=512, weights=""):
        if arch.lower() != "resnet50dilated":
            raise NotImplementedError(f"gim_semseg builds the encoder 'resnet50dilated' only, not {arch!r}")
        if fc_dim != FC_DIM:
            raise NotImplementedError(f"resnet50dilated has fc_dim {FC_DIM}, got {fc_dim}")
        enc = ResnetDilated()
        if weights:
            enc.load_state_dict(torch.load(weights, map_location="cpu"), strict=False)
        return enc

    @staticmethod
    def build_decoder(arch="ppm_deepsup", fc_dim=512, num_class=150, weights="", use_softmax=False):
        if arch.lower() != "ppm_deepsup":
            raise NotImplementedError(f"gim_semseg builds the decoder 'ppm_deepsup' only, not {arch!r}")
        if fc_dim != FC_DIM or not 1 <= num_class <= 256:
            raise NotImplementedError(f"ppm_deepsup on fc_dim {FC_DIM} with <= 256 classes, got fc_dim {fc_dim}, {num_class} classes")
        dec = PPMDeepsup(num_class=num_class, fc_dim=fc_dim, use_softmax=use_softmax)
        dec.apply(_weights_init)
        if weights:
            dec.load_state_dict(torch.load(weights, map_location="cpu"), strict=False)
        return dec


class SegmentationModule(nn.Module):
    """models.py:21-47.  `precision`: 'bf16' (default), 'fp16' or 'fp32' (exact fp32 products), resolved like the other ResNet-50 engines."""

    def __init__(self, net_enc, net_dec, crit=None, deep_sup_scale=None, precision=None):
        super().__init__()
        self.encoder = net_enc
        self.decoder = net_dec
        self.crit = crit
        self.deep_sup_scale = deep_sup_scale
        self.precision = resolve_precision(precision, "gim_semseg")
        self._packs = {}

    def load_state_dict(self, *a, **k):
        self._packs = {}
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._packs = {}
        return super()._apply(fn, *a, **k)

    # ---- one-time packing ------------------------------------------------------------------------------------------
    def _pack(self, device, precision):
        key = (str(device), precision)
        if key in self._packs:
            return self._packs[key]
        dt = PRECISION_DTYPE[precision]
        enc, dec = self.encoder, self.decoder
        P = {}
        P["c1"] = pack_conv(enc.conv1.weight, _bn(enc.bn1), dt, device, stride=2, pad=1, cin_pad=cstore(3, dt))
        P["c2"] = pack_conv(enc.conv2.weight, _bn(enc.bn2), dt, device, pad=1)
        P["c3"] = pack_conv(enc.conv3.weight, _bn(enc.bn3), dt, device, pad=1)
        pack_bottlenecks(P, enc, LAYERS, dt, device, _schedule)
        # the four branch 1x1s run on the fp32 pooled vectors (50 rows per image: exact fp32 products in every mode)
        for i, s in enumerate(ops.PPM_SCALES):
            P[f"ppm{s}"] = pack_conv(dec.ppm[i][1].weight, _bn(dec.ppm[i][2]), GIM_F32, device)
        P["cl0"] = pack_conv(dec.conv_last[0].weight, _bn(dec.conv_last[1]), dt, device, pad=1)
        P["cl4"] = pack_conv(dec.conv_last[4].weight, None, dt, device, bias=dec.conv_last[4].bias)
        self._packs[key] = (P, dt)
        return P, dt

    # ---- stages ------------------------------------------------------------------------------------------------------
    def _logits(self, img, precision, health):
        """img [B,3,H,W] fp32 normalised (device) -> fp32 logits [B,h8,w8,n_store] (conv_last[4] output, NHWC)"""
        P, dt = self._pack(img.device, precision)
        tdt = torch_dtype(dt)
        B, _, H, W = img.shape
        x = torch.empty(B, H, W, cstore(3, dt), dtype=tdt, device=img.device)
        ops.nchw_to_nhwc(img.contiguous().float(), x)
        x = ops.conv2d(x, P["c1"], ACT_RELU)
        x = ops.conv2d(x, P["c2"], ACT_RELU)
        x = ops.conv2d(x, P["c3"], ACT_RELU)
        x = ops.maxpool3x3s2(x)
        cat = None
        for li, (_, nblk) in enumerate(LAYERS, start=1):
            for bi in range(nblk):
                p = f"l{li}.{bi}."
                if li < 4 or bi < nblk - 1:
                    x = bottleneck(x, P, p, health)
                    continue
                # the last block: conv3 goes straight into channels 0..2047 of conv_last's concat buffer (row stride 4096)
                o = ops.conv2d(x, P[p + "c1"], ACT_RELU)
                o = ops.conv2d(o, P[p + "c2"], ACT_RELU)
                b_, h8, w8, cs = o.shape
                cat = torch.empty(b_, h8, w8, FC_DIM + 4 * PPM_DIM, dtype=tdt, device=img.device)
                rows = b_ * h8 * w8
                ops.conv_rows(o.view(-1, cs), P[p + "c3"], (1, 1, rows, 1, rows), cat.view(rows, -1)[:, :FC_DIM], ACT_RELU,
                              res=x.view(rows, -1), health=health)
        B, h8, w8, _ = cat.shape
        pooled = ops.ppm_pool(cat, FC_DIM)
        br = torch.empty(B, ops.PPM_BINS, PPM_DIM, dtype=torch.float32, device=img.device)
        for s in ops.PPM_SCALES:
            off, n = ops.PPM_OFFSETS[s], s * s
            for b in range(B):
                ops.linear(pooled[b, off:off + n], P[f"ppm{s}"], br[b, off:off + n], ACT_RELU)
        ops.ppm_upsample_concat(br, cat, FC_DIM)
        x = ops.conv2d(cat, P["cl0"], ACT_RELU)
        return ops.conv2d(x, P["cl4"], ACT_NONE, out_dtype=torch.float32)

    def _check(self, img):
        if not img.is_cuda:
            raise GimHipError("gim_amd semseg needs device (cuda/HIP) tensors: there is no CPU fallback")
        if img.dim() != 4 or img.shape[1] != 3:
            raise GimHipError(f"img_data must be [B,3,H,W], got {tuple(img.shape)}")

    def logits(self, img_data, precision=None):
        """the 1/8 logits [B,150,h8,w8] fp32 (conv_last output before the head; tests / diagnostics)"""
        self._check(img_data)
        lg = self._logits(img_data, precision or self.precision, None)
        return lg[..., :self.decoder.num_class].permute(0, 3, 1, 2).contiguous()

    def segment(self, img_data, segSize, with_prob=False):
        """img_data [B,3,H,W] normalised fp32 (device) -> uint8 class map [B,*segSize] (and, with_prob, the fp32 maximum softmax
        probability).  The logits are checked for non-finite values (and, in fp16, every residual store for overflow): one word read
        back with the map; a 16-bit run that trips it is repeated in fp32 with a warning."""
        self._check(img_data)
        prec = self.precision
        while True:
            flag = torch.zeros(1, dtype=torch.int32, device=img_data.device)
            lg = self._logits(img_data, prec, flag)
            out = ops.seg_head_argmax(lg, self.decoder.num_class, segSize, prob=with_prob, flag=flag)
            if int(flag.item()) == 0:
                return out
            if prec == "fp32":
                warnings.warn("gim_semseg: non-finite logits in the fp32 mode: the class map is not meaningful", RuntimeWarning)
                return out
            warnings.warn(f"gim_semseg: the {prec} forward left the 16-bit range (health word {int(flag.item())}): repeating it in fp32",
                          RuntimeWarning)
            prec = "fp32"

    def forward(self, feed_dict, *, segSize=None):
        if segSize is None:
            raise NotImplementedError("gim_semseg is inference only (training / deep supervision are not built)")
        img = feed_dict["img_data"]
        self._check(img)
        lg = self.logits(img)
        x = F.interpolate(lg, size=tuple(segSize), mode="bilinear", align_corners=False)
        return F.softmax(x, dim=1)
