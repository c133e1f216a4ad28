"""CPU restatement (torch fp32, functional) of the ADE20K segmenter gim runs before matching: ResnetDilated(resnet50, dilate_scale=8)
+ PPMDeepsup inference + hloc's `segment` arg-max (networks/mit_semseg/models/models.py:21-47, 208-268, 438-495; resnet.py:95-135;
hloc/utils/__init__.py:42-49).  Written from those semantics: deep stem (3 x conv3x3 + BN + ReLU, the first with stride 2), maxpool
3/2/1, bottleneck layers 3-4-6-3 whose stride-2 3x3 / downsample convolutions in layers 3 and 4 become stride 1 and whose 3x3s dilate
(layer 3: 1 then 2, layer 4: 2 then 4, padding = dilation), pyramid pooling at 1, 2, 3, 6 (adaptive average pool, 1x1 conv + BN +
ReLU, bilinear back), conv_last, bilinear upsampling of the logits, softmax, arg-max.

make_state_dict(seed) -> (encoder state dict, decoder state dict) in the reference's key layout (both halves of the two-file
checkpoint format), with values that keep the un-normalised residual streams in a trained network's range."""
import torch
import torch.nn.functional as F

LAYERS = ((64, 3), (128, 4), (256, 6), (512, 3))
SCALES = (1, 2, 3, 6)
NUM_CLASS = 150


def _conv_keys(sd, name, co, ci, k, g, bias=False, std=None):
    std = (2.0 / (ci * k * k)) ** 0.5 if std is None else std
    sd[name + ".weight"] = torch.randn(co, ci, k, k, generator=g) * std
    if bias:
        sd[name + ".bias"] = torch.randn(co, generator=g) * 0.1


def _bn_keys(sd, name, c, g, gain=1.0):
    sd[name + ".weight"] = (0.8 + 0.4 * torch.rand(c, generator=g)) * gain
    sd[name + ".bias"] = torch.randn(c, generator=g) * 0.1 * gain
    sd[name + ".running_mean"] = torch.randn(c, generator=g) * 0.1
    sd[name + ".running_var"] = 0.5 + torch.rand(c, generator=g)
    sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)


def block_geometry(li, bi):
    """(stride, dilation) of the 3x3 of block bi in layer li, and the downsample stride of the layer's first block"""
    st, d = 1, 1
    if li == 2 and bi == 0:
        st = 2
    elif li == 3:
        d = 1 if bi == 0 else 2
    elif li == 4:
        d = 2 if bi == 0 else 4
    return st, d, (2 if li == 2 else 1)


def make_state_dict(seed=0):
    g = torch.Generator().manual_seed(seed)
    enc = {}
    for i, (ci, co) in enumerate(((3, 64), (64, 64), (64, 128)), start=1):
        _conv_keys(enc, f"conv{i}", co, ci, 3, g)
        _bn_keys(enc, f"bn{i}", co, g)
    inpl = 128
    for li, (planes, nblk) in enumerate(LAYERS, start=1):
        for bi in range(nblk):
            p = f"layer{li}.{bi}."
            _conv_keys(enc, p + "conv1", planes, inpl, 1, g)
            _bn_keys(enc, p + "bn1", planes, g)
            _conv_keys(enc, p + "conv2", planes, planes, 3, g)
            _bn_keys(enc, p + "bn2", planes, g)
            _conv_keys(enc, p + "conv3", planes * 4, planes, 1, g)
            _bn_keys(enc, p + "bn3", planes * 4, g, gain=0.3)      # residual branches small against the identity, as in a trained net
            if bi == 0:
                _conv_keys(enc, p + "downsample.0", planes * 4, inpl, 1, g)
                _bn_keys(enc, p + "downsample.1", planes * 4, g)
            inpl = planes * 4
    dec = {}
    for i in range(len(SCALES)):
        _conv_keys(dec, f"ppm.{i}.1", 512, 2048, 1, g)
        _bn_keys(dec, f"ppm.{i}.2", 512, g)
    _conv_keys(dec, "cbr_deepsup.0", 512, 1024, 3, g)
    _bn_keys(dec, "cbr_deepsup.1", 512, g)
    _conv_keys(dec, "conv_last.0", 512, 4096, 3, g)
    _bn_keys(dec, "conv_last.1", 512, g)
    _conv_keys(dec, "conv_last.4", NUM_CLASS, 512, 1, g, bias=True, std=0.1)
    _conv_keys(dec, "conv_last_deepsup", NUM_CLASS, 512, 1, g, bias=True, std=0.1)
    return enc, dec


def _cbr(sd, conv, bn, x, stride=1, pad=0, dil=1, relu=True):
    y = F.conv2d(x, sd[conv + ".weight"], sd.get(conv + ".bias"), stride, pad, dil)
    if bn is not None:
        y = F.batch_norm(y, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, 1e-5)
    return F.relu(y) if relu else y


def encode(enc, img):
    """img [B,3,H,W] normalised -> conv5 [B,2048,h8,w8]"""
    x = _cbr(enc, "conv1", "bn1", img, 2, 1)
    x = _cbr(enc, "conv2", "bn2", x, 1, 1)
    x = _cbr(enc, "conv3", "bn3", x, 1, 1)
    x = F.max_pool2d(x, 3, 2, 1)
    for li, (_, nblk) in enumerate(LAYERS, start=1):
        for bi in range(nblk):
            p = f"layer{li}.{bi}."
            st, d, dst = block_geometry(li, bi)
            o = _cbr(enc, p + "conv1", p + "bn1", x)
            o = _cbr(enc, p + "conv2", p + "bn2", o, st, d, d)
            o = _cbr(enc, p + "conv3", p + "bn3", o, relu=False)
            idn = _cbr(enc, p + "downsample.0", p + "downsample.1", x, dst, relu=False) if bi == 0 else x
            x = F.relu(o + idn)
    return x


def ppm_pool(conv5):
    """-> [B, 50, C]: the adaptive average pools at 1, 2, 3, 6, bins row-major, scales concatenated"""
    return torch.cat([F.adaptive_avg_pool2d(conv5, s).flatten(2) for s in SCALES], 2).transpose(1, 2)


def ppm_head(dec, conv5):
    """-> (pooled [B,50,2048], logits [B,150,h8,w8]) of PPMDeepsup's inference branch before its upsampling"""
    h8, w8 = conv5.shape[-2:]
    outs = [conv5]
    for i, s in enumerate(SCALES):
        y = _cbr(dec, f"ppm.{i}.1", f"ppm.{i}.2", F.adaptive_avg_pool2d(conv5, s))
        outs.append(F.interpolate(y, (h8, w8), mode="bilinear", align_corners=False))
    x = _cbr(dec, "conv_last.0", "conv_last.1", torch.cat(outs, 1), 1, 1)
    return ppm_pool(conv5), _cbr(dec, "conv_last.4", None, x, relu=False)


def head(logits, seg_size):
    """logits [B,150,h,w] -> (class map int64 [B,H,W], top-2 margin of the interpolated logits, max softmax probability)"""
    x = F.interpolate(logits, size=tuple(seg_size), mode="bilinear", align_corners=False)
    top = x.topk(2, dim=1).values
    prob, cls = F.softmax(x, dim=1).max(dim=1)
    return cls, top[:, 0] - top[:, 1], prob


def segment(enc, dec, img, seg_size=None):
    """-> dict(conv5, pooled, logits, cls, margin, prob)"""
    seg_size = tuple(img.shape[-2:]) if seg_size is None else seg_size
    conv5 = encode(enc, img)
    pooled, logits = ppm_head(dec, conv5)
    cls, margin, prob = head(logits, seg_size)
    return {"conv5": conv5, "pooled": pooled, "logits": logits, "cls": cls, "margin": margin, "prob": prob}


def seeded_image(h, w, seed):
    """a normalised [1,3,h,w] image with smooth structure (a few blurred blobs + texture), so that class maps have regions"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 3, max(2, h // 16), max(2, w // 16), generator=g)
    img = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False) + 0.15 * torch.rand(1, 3, h, w, generator=g)
    img = img.clamp(0, 1)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (img - mean) / std
