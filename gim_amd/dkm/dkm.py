"""gim_dkm on MI355X: the reference's `DKMv3(...)` / `RegressionMatcher` surface
(`networks/dkm/models/model_zoo/DKMv3.py:5-145`, `networks/dkm/models/dkm.py:537-752`) over hand-written HIP.

Drop-in contract:
  * `DKMv3(weights, h, w, symmetric=True, sample_mode='threshold_balanced', upsample_preds=...)` returns a module whose
    `state_dict()` has the reference's 811 tensors (`encoder.net.*` = torchvision resnet50 names, `decoder.*`), so
    gim_dkm checkpoints load with the reference's prefix rules (`demo.py:364-376`);
  * `h_resized, w_resized, upsample_preds, upsample_res, symmetric, sample_thresh,
    use_soft_mutual_nearest_neighbours` are plain attributes read at call time (callers mutate them after
    construction, `trainer/lightning.py:32-37`);
  * `match(im1, im2)` takes [1,3,H,W] fp32 tensors and returns `(warp [Hs, 2Ws, 4], certainty [Hs, 2Ws])`,
    `sample(dense_matches, dense_certainty, num)` returns `([n,4], [n])` like `dkm.py:583-620`.
  * built: symmetric, non-batched matching with or without the upsampling pass (the configuration gim runs).

The nn.Module tree only holds parameters.  Every stage of `match()` is a libgimhip launch (convolutions, 1x1
projections and the GP's kernel / posterior products on the implicit-GEMM kernel; the rest in `csrc/dkm.hip`,
`csrc/gp_solve.hip`).  Constant tables (the GP's Fourier features of the pixel grid) are built once per shape on the
host with the reference's own fp32 ops.  `sample()` draws with torch's generator like the reference (the RNG contract
is "same distribution"); the KDE is a HIP kernel.  No CPU / eager fallback.
"""
import torch
import torch.nn as nn

from .. import ops
from .._lib import ACT_RELU, GIM_F32, GimHipError
from ..dense import (GP, ConvRefiner, DenseMatcher, _bn_after_bias, balanced_sample, gim_dkm_inference,  # noqa: F401  (re-exported)
                     gp_features, gp_posterior, pack_refiner, refine, refiner_dims)
from ..packing import PRECISION_DTYPE, bn_params as _bn, cstore, pack_conv, torch_dtype
from ..precision import resolve as resolve_precision
from ..resnet50 import LAYERS, add_layers, bottleneck, pack_bottlenecks
from ..switches import flag

REFINER = {"16": (512, 128, 7), "8": (512, 64, 3), "4": (256, 32, 2), "2": (64, 16, None), "1": (3, 6, None)}
GP_DIM, DFN_DIM, FEAT_DIM = 256, 384, 256


def _stride_schedule(li, bi):
    """torchvision resnet50: layers 2..4 halve the resolution in their first block; no dilation"""
    first = 2 if li > 1 and bi == 0 else 1
    return first, 1, first


# ---------------------------------------------------------------------------------------- parameter containers
class _ResNet50(nn.Module):
    """torchvision resnet50 parameter layout without fc (encoders.py:30-41)"""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        add_layers(self, 64, _stride_schedule)


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = _ResNet50()


class _RRB(nn.Module):
    def __init__(self, ci, co):
        super().__init__()
        self.conv1 = nn.Conv2d(ci, co, 1)
        self.conv2 = nn.Conv2d(co, co, 3, 1, 1)
        self.bn = nn.BatchNorm2d(co)
        self.conv3 = nn.Conv2d(co, co, 3, 1, 1)


class _CAB(nn.Module):
    def __init__(self, ci, co):
        super().__init__()
        self.conv1 = nn.Conv2d(ci, co, 1)
        self.conv2 = nn.Conv2d(co, co, 1)


class _DFN(nn.Module):
    def __init__(self):
        super().__init__()
        ks = ("32", "16")
        self.feat_input_modules = nn.ModuleDict({k: nn.Conv2d(512, FEAT_DIM, 1) for k in ks})
        self.pred_input_modules = nn.ModuleDict({k: nn.Identity() for k in ks})
        self.rrb_d = nn.ModuleDict({k: _RRB(GP_DIM + FEAT_DIM, DFN_DIM) for k in ks})
        self.cab = nn.ModuleDict({k: _CAB(2 * DFN_DIM, DFN_DIM) for k in ks})
        self.rrb_u = nn.ModuleDict({k: _RRB(DFN_DIM, DFN_DIM) for k in ks})
        self.terminal_module = nn.ModuleDict({k: nn.Conv2d(DFN_DIM, 3, 1) for k in ks})


class _Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.embedding_decoder = _DFN()
        self.gps = nn.ModuleDict({"32": GP(GP_DIM), "16": GP(GP_DIM)})
        self.proj = nn.ModuleDict({"16": nn.Conv2d(1024, 512, 1), "32": nn.Conv2d(2048, 512, 1)})
        self.conv_refiner = nn.ModuleDict({s: ConvRefiner(*refiner_dims(REFINER, s), REFINER[s][1]) for s in REFINER})


class RegressionMatcher(DenseMatcher):
    engine, max_batch, kde_half = "DKM", 8, False

    def __init__(self, h=384, w=512, sample_mode="threshold_balanced", upsample_preds=True, symmetric=True, name=None,
                 use_soft_mutual_nearest_neighbours=False, precision=None, **kwargs):
        super().__init__(h, w, sample_mode, upsample_preds, symmetric, name)
        self.encoder = _Encoder()
        self.decoder = _Decoder()
        self.upsample_res = (1152, 1536)
        self.use_soft_mutual_nearest_neighbours = use_soft_mutual_nearest_neighbours
        self.precision = resolve_precision(precision, "gim_dkm")
        self._gp_f = {}
        self.overlap_gp = flag("dkm_overlap", True)   # GP on a side stream beside the high-res encoder

    def load_state_dict(self, state_dict, *a, **k):
        self._packed = None
        self._gp_f.clear()
        return super().load_state_dict(state_dict, *a, **k)

    def _apply(self, fn, *a, **k):
        self._packed = None
        self._gp_f = {}
        return super()._apply(fn, *a, **k)

    # ---- one-time packing -------------------------------------------------------------------------------------
    def _prepack(self, device):
        dt = PRECISION_DTYPE[self.precision]
        P = {}
        net = self.encoder.net
        P["stem"] = pack_conv(net.conv1.weight, _bn(net.bn1), dt, device, stride=2, pad=3, cin_pad=cstore(3, dt))
        pack_bottlenecks(P, net, LAYERS, dt, device, _stride_schedule)
        dec = self.decoder
        for s in ("32", "16"):
            P["proj" + s] = pack_conv(dec.proj[s].weight, None, dt, device, bias=dec.proj[s].bias)
            e = dec.embedding_decoder
            P["fin" + s] = pack_conv(e.feat_input_modules[s].weight, None, dt, device, bias=e.feat_input_modules[s].bias)
            for nm, rrb in (("rd" + s, e.rrb_d[s]), ("ru" + s, e.rrb_u[s])):
                P[nm + ".c1"] = pack_conv(rrb.conv1.weight, None, dt, device, bias=rrb.conv1.bias)
                P[nm + ".c2"] = pack_conv(rrb.conv2.weight, _bn_after_bias(rrb.bn, rrb.conv2.bias), dt, device, pad=1)
                P[nm + ".c3"] = pack_conv(rrb.conv3.weight, None, dt, device, pad=1, bias=rrb.conv3.bias)
            # CAB's two 1x1 convs act on [b, 768] pooled vectors: fp32 operands (a 2-row GEMM)
            P["cab" + s + ".c1"] = pack_conv(e.cab[s].conv1.weight, None, GIM_F32, device, bias=e.cab[s].conv1.bias)
            P["cab" + s + ".c2"] = pack_conv(e.cab[s].conv2.weight, None, GIM_F32, device, bias=e.cab[s].conv2.bias)
            P["term" + s] = pack_conv(e.terminal_module[s].weight, None, dt, device, bias=e.terminal_module[s].bias)
        for s, ref in dec.conv_refiner.items():
            pack_refiner(P, s, ref, *refiner_dims(REFINER, s), dt, device)
        self._packed = (P, dt, device)

    def _gp_features(self, s, h, w, device):
        """f = cos(8 pi pos_conv(coords)) of GP.get_pos_enc (dkm.py:314-331): constant per (scale, h, w); built once on the
        host with the reference's fp32 ops, cached on the device as rows [h*w, 256]."""
        key = (s, h, w, str(device))
        if key not in self._gp_f:
            self._gp_f[key] = gp_features(self.decoder.gps[s].pos_conv, h, w, GP_DIM).to(device)
        return self._gp_f[key]

    # ---- stages ---------------------------------------------------------------------------------------------------
    def _encode(self, P, x, top=32):
        """x [nb,hs,ws,cpad] NHWC -> {1: x, 2, 4, 8, 16, 32} (encoders.py:43-62); top = 8: layers 3 and 4 are not computed (the
        upsampling pass reads scales 8, 4, 2, 1 only)"""
        feats = {1: x}
        x = ops.conv2d(x, P["stem"], ACT_RELU)
        feats[2] = x
        x = ops.maxpool3x3s2(x)
        for li, (_, nblk) in enumerate(LAYERS, start=1):
            for bi in range(nblk):
                x = bottleneck(x, P, f"l{li}.{bi}.")
            feats[2 ** (li + 1)] = x
            if 2 ** (li + 1) >= top:
                break
        return feats

    def _rrb(self, P, nm, x):
        x = ops.conv2d(x, P[nm + ".c1"])
        r = ops.conv2d(x, P[nm + ".c2"], ACT_RELU)
        return ops.conv2d(r, P[nm + ".c3"], ACT_RELU, res=x)       # relu(x + conv3(r))

    def _gp(self, P, s, a32, nb, h, w, tdt, out):
        """GP.forward of scale s (dense.gp_posterior): a32 fp32 rows [nb*hw (+64 slack), 512] -> mu into `out` (row view [nb*hw, 256], dtype tdt)"""
        gp_posterior(a32, nb, h, w, self._gp_features(s, h, w, a32.device), out, self._gp_is_exact())

    def _refine(self, P, s, dt, x, y, flow, cert, ins, full_hw):
        refine(P, s, dt, x, y, flow, cert, ins, full_hw, REFINER[s], self.refiner_fused)

    first_names = ("a32_32", "a32_16", "fin32", "fin16")
    support_names = ("lo1", "lo2", "lo4", "lo8", "a16", "hi1", "hi2", "hi4", "hi8")
    slack_names = ("a32_32", "a32_16")

    def _tag_extra(self):
        return ()

    def _state(self, P, dt, im1, im2, after_low=None):
        """everything match_batch computes from one image alone, for the images of im1 (and im2 behind them): {kind: [nb, ...]}
          lo1 / lo2 / lo4 / lo8     low-resolution pyramid levels the refiners read
          a32_32 / a32_16           proj32 / proj16 rows in fp32 (what the GP reads; `.rows`: the same buffer with its 64 slack rows)
          a16                       proj16 at the module's precision (refiner 16)
          fin32 / fin16             the feature half of the DFN's input, feat_input_modules(proj)
          hi1 / hi2 / hi4 / hi8     the pyramid of the upsampling pass (layers 3, 4 of that ResNet are never read: not computed)
          black                     the black-pixel mask of the match() tail at the output resolution
        after_low(state): called when the low-resolution part stands (match_batch starts the GP on its side stream there)."""
        tdt = torch_dtype(dt)
        hs, ws = self.h_resized, self.w_resized
        if hs % 32 or ws % 32:
            raise GimHipError(f"h_resized / w_resized must be multiples of 32, got {(hs, ws)}")
        dev = im1.device
        st = {}
        pyr = self._encode(P, self._images(dt, im1, im2, hs, ws))
        for sc in (1, 2, 4, 8):
            st[f"lo{sc}"] = pyr[sc]
        for s in ("32", "16"):
            feat = pyr[int(s)]
            nb, h, w, _ = feat.shape
            n = h * w
            a32 = torch.zeros(nb * n + 64, 512, dtype=torch.float32, device=dev)
            ops.linear(feat.view(nb * n, feat.shape[3]), P["proj" + s], a32)
            if dt == GIM_F32:
                a = a32[:nb * n].view(nb, h, w, 512)
            else:
                a = torch.empty(nb, h, w, 512, dtype=tdt, device=dev)
                ops.cast_rows(a32[:nb * n], a.view(nb * n, 512))
            fin = torch.empty(nb * n, FEAT_DIM, dtype=tdt, device=dev)
            ops.linear(a.view(nb * n, 512), P["fin" + s], fin)
            st["a32_" + s], st["a32_" + s + ".rows"] = a32[:nb * n].view(nb, n, 512), a32
            st["fin" + s] = fin.view(nb, h, w, FEAT_DIM)
            if s == "16":
                st["a16"] = a
        if after_low is not None:
            after_low(st)
        if self.upsample_preds:
            hi = self._encode(P, self._images(dt, im1, im2, *self.upsample_res), top=8)
            for sc in (1, 2, 4, 8):
                st[f"hi{sc}"] = hi[sc]
        st["black"] = self._black([im1] if im2 is None else [im1, im2], *self._out_size())
        return st

    def _gp_pair(self, P, dt, q, s):
        """GP + DFN input of scale s for the stacked pair batch q: everything of that scale that needs both images and not the coarser
        scales' flow (GP.forward ignores `dense_flow`, dkm.py:340) -> emb_in = [feats | mu]"""
        tdt = torch_dtype(dt)
        nb, h, w, _ = q["fin" + s].shape
        n = h * w
        emb_in = torch.empty(nb * n, FEAT_DIM + GP_DIM, dtype=tdt, device=q["fin" + s].device)
        emb_in[:, :FEAT_DIM].copy_(q["fin" + s].view(nb * n, FEAT_DIM))
        self._gp(P, s, q["a32_" + s + ".rows"], nb, h, w, tdt, emb_in[:, FEAT_DIM:])
        return emb_in

    def _begin(self, P, dt, q, B):
        """The GP of both coarse scales (a latency-bound chain of ~150 small launches) needs the low-resolution state only: with the
        upsampling pass it runs on a side stream while the main stream encodes (match_batch) or gathers (match_features) the rest."""
        if not (self.upsample_preds and self.overlap_gp):
            return {s: self._gp_pair(P, dt, q, s) for s in ("32", "16")}, None
        main = torch.cuda.current_stream()
        side = self._side_stream(q["fin16"].device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            gp = {s: self._gp_pair(P, dt, q, s) for s in ("32", "16")}
        for s in ("32", "16"):
            q["a32_" + s + ".rows"].record_stream(side)
            q["fin" + s].record_stream(side)
            gp[s].record_stream(main)
        return gp, side

    def _match_state(self, P, dt, q, sup, B, pending):
        gp, side = pending if pending is not None else self._begin(P, dt, q, B)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        hs, ws = self.h_resized, self.w_resized
        f1 = {1: q["lo1"], 2: q["lo2"], 4: q["lo4"], 8: q["lo8"], 16: q["a16"], 32: q["fin32"]}
        y1 = None if sup is None else {1: sup["lo1"], 2: sup["lo2"], 4: sup["lo4"], 8: sup["lo8"], 16: sup["a16"]}
        cor = self._decode(P, dt, f1, gp=gp, sup=y1)
        if self.upsample_preds:
            hs, ws = self.upsample_res
        low = ops.resize_bilinear(cor[16][1], (hs, ws))
        if self.upsample_preds:
            f1 = {sc: q[f"hi{sc}"] for sc in (1, 2, 4, 8)}
            y1 = None if sup is None else {sc: sup[f"hi{sc}"] for sc in (1, 2, 4, 8)}
            cor = self._decode(P, dt, f1, upsample=True, dense_flow=cor[1][0], dense_certainty=cor[1][1], sup=y1)
        flow, cert = cor[1]
        warp, certainty = self._finish_state(q["black"], flow, cert, low, hs, ws)
        self._debug = {"corresps": cor}
        return warp, certainty

    def _decode(self, P, dt, f1, upsample=False, dense_flow=None, dense_certainty=None, gp=None, sup=None):
        """Decoder.forward on the symmetric pair (f2 = f1 with the two images swapped) -> {scale: (flow, certainty)}.  f1: per scale the
        tensor the refiner reads (16: the projection; 32: anything of that size), gp: {scale: emb_in} of `_gp_pair`, sup: f1 in support
        order (match_features gathers it; None: the two halves of f1 are swapped with a copy)"""
        tdt = torch_dtype(dt)
        scales = ["8", "4", "2", "1"] if upsample else ["32", "16", "8", "4", "2", "1"]
        sizes = {s: tuple(f1[s].shape[1:3]) for s in f1}
        full = sizes[1]
        dev = f1[1].device
        nb = f1[1].shape[0]
        half = nb // 2
        coarsest = int(scales[0])
        if not upsample:
            flow = ops.dkm_grid_coords(nb, *sizes[coarsest], dev)
            cert = torch.zeros(nb, *sizes[coarsest], 1, dtype=torch.float32, device=dev)
        else:
            flow = ops.resize_bilinear(dense_flow, sizes[coarsest])
            cert = ops.resize_bilinear(dense_certainty, sizes[coarsest])
        old = None
        out = {}
        for s in scales:
            ins = int(s)
            h, w = sizes[ins]
            n = h * w
            a = f1[ins]
            if s in ("32", "16"):
                emb_in = gp[s]
                emb = self._rrb(P, "rd" + s, emb_in.view(nb, h, w, FEAT_DIM + GP_DIM))
                if old is not None:
                    old = ops.resize_bilinear(old, (h, w))
                # CAB (dkm.py:160-168): global average of cat[context, emb] -> 1x1 -> relu -> 1x1 -> sigmoid gate
                pooled = torch.zeros(nb, 2 * DFN_DIM, dtype=torch.float32, device=dev)
                if old is not None:
                    ops.global_avgpool(old, pooled, 0)
                ops.global_avgpool(emb, pooled, DFN_DIM)
                g1 = torch.empty(nb, DFN_DIM, dtype=torch.float32, device=dev)
                ops.linear(pooled, P["cab" + s + ".c1"], g1, ACT_RELU)
                g2 = torch.empty(nb, DFN_DIM, dtype=torch.float32, device=dev)
                ops.linear(g1, P["cab" + s + ".c2"], g2)
                ctx = ops.cab_scale_add(g2, old, emb)
                old = self._rrb(P, "ru" + s, ctx)
                preds = torch.empty(nb * n, P["term" + s].n_store, dtype=torch.float32, device=dev)
                ops.linear(old.view(nb * n, DFN_DIM), P["term" + s], preds)
                flow = torch.zeros(nb, h, w, 2, dtype=torch.float32, device=dev)
                cert = torch.empty(nb, h, w, 1, dtype=torch.float32, device=dev)
                ops.dkm_flow_update(flow, cert, preds, 1.0, 1.0, cert_init=True)       # flow, certainty = preds
            if s in REFINER:
                y = sup[ins] if sup is not None else torch.cat((a[half:], a[:half]))    # support = the other image of each pair
                self._refine(P, s, dt, a, y, flow, cert, ins, full)
            out[ins] = (flow, cert)
            if s != "1":
                flow = ops.resize_bilinear(flow, sizes[ins // 2])
                cert = ops.resize_bilinear(cert, sizes[ins // 2])
        return out

    def _side_stream(self, dev):
        if getattr(self, "_side", None) is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        return self._side


def DKMv3(weights, h, w, symmetric=True, sample_mode="threshold_balanced", **kwargs):
    """`networks/dkm/models/model_zoo/DKMv3.py:5-145`; `weights` is ignored like in the reference (load_state_dict is
    the caller's job, `demo.py:364-376`)."""
    kwargs.pop("device", None)
    return RegressionMatcher(h=h, w=w, name="DKMv3", sample_mode=sample_mode, symmetric=symmetric, **kwargs)
