"""The Bottleneck stages of the two ResNet-50 encoders that run block by block on the implicit GEMM: gim_dkm's torchvision
resnet50 (`networks/dkm/models/encoders.py:30-62`) and the segmenter's dilated one (`networks/mit_semseg/models/models.py:208-268`).
They differ in the stem and in the (stride, dilation) schedule of the blocks, which the caller passes in.
"""
import torch.nn as nn

from . import ops
from ._lib import ACT_NONE, ACT_RELU
from .packing import bn_params as _bn, pack_conv

LAYERS = ((64, 3), (128, 4), (256, 6), (512, 3))      # (planes, blocks) of layer1..4


class Bottleneck(nn.Module):
    def __init__(self, inpl, planes, stride, dilation=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inpl, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride


def add_layers(net, inpl, schedule):
    """net.layer1..4 = the Bottleneck stacks of LAYERS; schedule(li, bi) -> (stride, dilation, downsample stride) of block bi of layer li"""
    for li, (planes, nblk) in enumerate(LAYERS, start=1):
        blocks = []
        for bi in range(nblk):
            stride, dilation, ds_stride = schedule(li, bi)
            ds = None
            if bi == 0:
                ds = nn.Sequential(nn.Conv2d(inpl, planes * 4, 1, ds_stride, bias=False), nn.BatchNorm2d(planes * 4))
            blocks.append(Bottleneck(inpl, planes, stride, dilation, ds))
            inpl = planes * 4
        setattr(net, f"layer{li}", nn.Sequential(*blocks))


def pack_bottlenecks(P, net, layers, dt, device, schedule):
    """P[l{li}.{bi}.c1 / .c2 / .c3 / .ds] of net.layer1..4 (BatchNorm folded); layers, schedule: as in add_layers"""
    for li, (_, nblk) in enumerate(layers, start=1):
        for bi in range(nblk):
            blk = getattr(net, f"layer{li}")[bi]
            p = f"l{li}.{bi}."
            stride, dilation, ds_stride = schedule(li, bi)
            P[p + "c1"] = pack_conv(blk.conv1.weight, _bn(blk.bn1), dt, device)
            P[p + "c2"] = pack_conv(blk.conv2.weight, _bn(blk.bn2), dt, device, stride=stride, pad=dilation, dilation=dilation)
            P[p + "c3"] = pack_conv(blk.conv3.weight, _bn(blk.bn3), dt, device)
            if blk.downsample is not None:
                P[p + "ds"] = pack_conv(blk.downsample[0].weight, _bn(blk.downsample[1]), dt, device, stride=ds_stride)


def bottleneck(x, P, p, health=None):
    """one block, packed under the prefix p: relu(conv3(relu(conv2(relu(conv1(x))))) + identity or downsample(x)), BatchNorm folded.
    health: the int32 word the residual store reports a left 16-bit range into (ops.conv_rows), or None"""
    o = ops.conv2d(x, P[p + "c1"], ACT_RELU)
    o = ops.conv2d(o, P[p + "c2"], ACT_RELU)
    idn = ops.conv2d(x, P[p + "ds"], ACT_NONE) if (p + "ds") in P else x
    return ops.conv2d(o, P[p + "c3"], ACT_RELU, res=idn, health=health)
