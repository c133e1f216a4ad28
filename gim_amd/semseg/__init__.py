"""gim_semseg: the ADE20K-150 segmenter (ResNet50-dilated + PPM-deepsup) of gim's SfM / video paths on libgimhip.

    from gim_amd.semseg import ModelBuilder, SegmentationModule, segment
    enc = ModelBuilder.build_encoder(arch='resnet50dilated', fc_dim=2048, weights='weights/encoder_epoch_20.pth')
    dec = ModelBuilder.build_decoder(arch='ppm_deepsup', fc_dim=2048, num_class=150, weights='weights/decoder_epoch_20.pth',
                                     use_softmax=True)
    module = SegmentationModule(enc, dec, torch.nn.NLLLoss(ignore_index=-1)).to('cuda').eval()
    mask = segment(rgb, 1920, 'cuda', module)          # numpy uint8 [H', W'] -- hloc/utils/__init__.py:42-49

`python -m gim_amd.semseg IMAGES OUT_DIR [--size 1920]` writes OUT_DIR/<name>.npy as reconstruction.py:26-53 does.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .model import ModelBuilder, PPMDeepsup, ResnetDilated, SegmentationModule  # noqa: F401

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def resize_long_side(img, size):
    """read_deeplab_image's resize (hloc/utils/__init__.py:19-31): long side to `size` when larger, cv2 INTER_AREA when cv2 imports,
    otherwise area averaging (adaptive average pooling: INTER_AREA for integer factors, gim_amd/demo.py documents the difference).
    img: numpy [H, W, 3] -> numpy float32 [H', W', 3]"""
    height, width = img.shape[:2]
    if max(width, height) <= size:
        return img.astype(np.float32)
    if width > height:
        nw, nh = size, int(size * height / width)
    else:
        nw, nh = int(size * width / height), size
    try:
        import cv2
        return cv2.resize(img, (nw, nh), interpolation=cv2.INTER_AREA).astype(np.float32)
    except ImportError:
        t = torch.from_numpy(np.ascontiguousarray(img)).float().permute(2, 0, 1)[None]
        return F.interpolate(t, size=(nh, nw), mode="area")[0].permute(1, 2, 0).numpy()


def read_segmentation_image(img, size):
    """hloc/utils/__init__.py:34-39: [3, H', W'] fp32, ImageNet-normalised"""
    t = torch.from_numpy(np.ascontiguousarray(resize_long_side(img, size))).float().div(255).permute(2, 0, 1)
    return (t - torch.tensor(MEAN).view(-1, 1, 1)) / torch.tensor(STD).view(-1, 1, 1)


def segment(rgb, size, device, segmentation_module):
    """hloc.utils.segment: rgb numpy [H, W, 3] -> numpy uint8 [H', W'] class map at the resized resolution (fast path: no
    full-resolution score tensor)"""
    img = read_segmentation_image(rgb, size)
    out = segmentation_module.segment(img[None].to(device), tuple(img.shape[1:]))
    return out[0].cpu().numpy().astype(np.uint8)


def resized_wh(width, height, size):
    """read_deeplab_image's target (hloc/utils/__init__.py:19-31): the long side brought down to `size`, or the frame's own size"""
    if max(width, height) <= size:
        return width, height
    if width > height:
        return size, int(size * height / width)
    return int(size * width / height), size


@torch.no_grad()
def segment_device(frames_u8, size, segmentation_module):
    """`segment` without a host pass: frames_u8 uint8 [S, H, W, 3] (or [H, W, 3]) on the device -> uint8 [S, H', W'] class maps on the
    device at the long-side-`size` resolution.  The input of the module is ops.frame_prep's `norm` output (gim_amd/frame_prep.py: the
    written area-resize contract, then (x / 255 - mean) / std), one launch for all frames, then `segmentation_module.segment` per
    frame.  Where the frame is not resized this is `segment`'s input bit for bit; where it is, `segment` resizes with OpenCV or
    average pooling and the inputs differ as those resizes differ from the contract."""
    from .. import frame_prep as fp
    from .. import ops
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8[None]
    S, H, W = frames_u8.shape[:3]
    wn, hn = resized_wh(W, H, size)
    r = ops.frame_prep(frames_u8.contiguous(), None, None, [(s, None, (wn, hn), fp.OUT_NORM) for s in range(S)], kept=False)
    out = torch.empty(S, hn, wn, dtype=torch.uint8, device=frames_u8.device)
    for s in range(S):
        out[s] = segmentation_module.segment(r.get(s, "norm")[None], (hn, wn))[0].to(torch.uint8)
    return out
