"""The fp32 mode's split products (gim_conv_args.split16) have a weight-side range: every fp32 weight is scaled by 4096 before its IEEE-fp16
hi / lo split, so a BatchNorm-folded filter of 16 or more splits into infinities.  A channel whose running_var is 0 (common in trained ResNets:
dead channels) folds gamma / sqrt(eps) ~ 316 gamma into its filter.  `split16_weight_overflow` is the pack-time decision; LoFTR._prepack acts on it
(warns, turns fp32_split off) before the first launch.  Both run on the CPU: the packs are plain torch tensors."""
import warnings

import pytest
import torch

from tools import synth_loftr as S

DEAD = "backbone.encode.layer2.0.bn2"   # the 3 x 3 conv of layer 2's first block -> pack "l2.0.c2"


def _packs(sd, precision="fp32"):
    model, _ = S.synthetic_model(precision)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        P = model._prepack(torch.device("cpu"))
    return model, P, [str(w.message) for w in rec]


def _dead_channels(sd, n=3):
    sd = {k: v.clone() for k, v in sd.items()}
    sd[DEAD + ".running_var"][:n] = 0.0
    return sd


def test_folded_weight_reference():
    """the premise, computed from the state dict alone: zero running_var lifts the folded filter past 65504 / 4096"""
    from gim_amd.packing import fold_bn
    _, sd = S.synthetic_model("fp32")
    bad = _dead_channels(sd)
    bn = lambda d: tuple(d[f"{DEAD}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")) + (1e-5,)  # noqa: E731
    w = sd["backbone.encode.layer2.0.conv2.weight"]
    ok_max = fold_bn(w, bn(sd))[0].abs().max().item()
    bad_max = fold_bn(w, bn(bad))[0].abs().max().item()
    print(f"layer2.0.conv2 folded max |w|: {ok_max:.3f} healthy, {bad_max:.3f} with 3 dead channels")
    assert ok_max * 4096 < 65504 <= bad_max * 4096


def test_split16_weight_overflow_names_the_dead_channels_pack():
    from gim_amd.loftr.loftr import split16_weight_overflow
    _, sd = S.synthetic_model("fp32")
    _, P, _ = _packs(sd)
    assert split16_weight_overflow(P) == []
    _, Pb, _ = _packs(_dead_channels(sd))
    assert split16_weight_overflow(Pb) == ["l2.0.c2"]


def test_split16_weight_overflow_threshold():
    """exactly at the boundary: 65503.99 / 4096 is in range, 65504 / 4096 is not (a finite hi needs rn16(4096 |w|) <= 65504; the check is
    the conservative side of 65520), and a non-fp32 pack is not looked at"""
    from types import SimpleNamespace as NS
    from gim_amd.loftr.loftr import split16_weight_overflow
    inside = torch.tensor([15.99, -1.0])
    edge = torch.tensor([0.5, -65504.0 / 4096])
    P = {"a": NS(w=inside), "b": NS(w=edge), "c": NS(w=edge.half()), "ln": (torch.ones(3), torch.zeros(3), 1e-5), "e": NS(w=torch.empty(0))}
    assert split16_weight_overflow(P) == ["b"]


def test_prepack_falls_back_to_exact_products():
    _, sd = S.synthetic_model("fp32")
    model, _, msgs = _packs(sd)
    assert model.fp32_split and not model.split_overflowed and not msgs, msgs
    model, _, msgs = _packs(_dead_channels(sd))
    assert not model.fp32_split and model.split_overflowed
    assert any("l2.0.c2" in m and "exact fp32 products" in m for m in msgs), msgs


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_prepack_split_check_is_the_fp32_modes_only(precision):
    """the 16-bit modes never multiply split products: their packs are not judged by the split range (fp16 has its own check)"""
    _, sd = S.synthetic_model(precision)
    model, _, _ = _packs(_dead_channels(sd), precision)
    assert model.fp32_split and not model.split_overflowed
