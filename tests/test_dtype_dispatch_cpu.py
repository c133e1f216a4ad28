"""The one dtype convention of the C ABI (include/gim_hip.h, csrc/gim_common.h: GIM_TWIN / GIM_TO_F16 / GIM_ROUTE_H16 / GIM_ROUTE_ANY),
without a GPU: the header and the ctypes mirror declare no `*_f16` twin, every fused entry point carries an `int dtype` tag where the header
says it sits, and a tag that names no 16-bit kind is refused before a pointer is read or the HIP runtime is called -- which is why these
calls are safe on a machine without a device: the pointers are addresses of small host buffers.  The entry points that accept fp32 too
(every other prototype of the header with an `int` tag) refuse a tag that names no kind and a pair of tags that names both 16-bit kinds in
the same way: in either flavour `tag == GIM_H16` decides the element width, so such a call would run with 4-byte accesses to 2-byte
buffers."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gim_hip.h")).read(), flags=re.S)

# the fused entry points -> the parameter their tag stands in front of
FUSED = {
    "gim_bneck64_fused": "health", "gim_bneck64_fused_ds": "health",
    "gim_bneck_tail128": "health", "gim_bneck_tail128_ds": "health", "gim_bneck_tail256": "health",
    "gim_token_mlp": "stream", "gim_token_mlp_emit": "emit",
    "gim_fine_fused": "stream", "gim_fine_fused_dev": "stream",
}
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "gim_stream_t": ctypes.c_void_p}
# plausible sizes by parameter name: one 8 x 32 image tile / 256 pixel rows / 64 token rows / 8 fine matches
_INTS = {"B": 1, "H": 8, "W": 32, "Ho": 8, "Wo": 32, "Hin": 16, "Win": 64, "M": 256, "M_cap": 8, "n_next": 128, "act_next": 1,
         "R": 64, "C": 256, "L": 64, "S": 64, "ldm": 256, "ldxb": 256, "ldx32": 256,
         "hf0": 16, "wf0": 16, "hf1": 16, "wf1": 16, "ldf": 128, "w0c": 4, "w1c": 4, "stride": 4, "has_scale0": 0}
_INTS_OF = {"gim_bneck64_fused": {"n_next": 64}, "gim_fine_fused": {"M": 8, "C": 128, "W": 5}, "gim_fine_fused_dev": {"C": 128, "W": 5}}


def _params(name):
    """[(C type with the pointer levels collapsed to '*', parameter name)] of the header's prototype"""
    m = re.search(r"^\s*int\s+%s\s*\((.*?)\)\s*;" % name, HEADER, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    out = []
    for a in m.group(1).split(","):
        a = a.strip()
        out.append(("*" if "*" in a else a.replace("const", "").split()[0], re.search(r"(\w+)$", a).group(1)))
    return out


def test_no_twin_in_the_declared_abi():
    from gim_amd import _lib
    declared = set(re.findall(r"\b(gim_[a-z0-9_]+)\s*\(", HEADER))
    assert len(declared) > 50, "no declarations parsed"
    assert not [n for n in declared if n.endswith("_f16")]
    assert not [n for n in _lib.PROTOTYPES if n.endswith("_f16")]


@pytest.mark.parametrize("name", sorted(FUSED))
def test_every_fused_entry_point_carries_a_tag(name):
    from gim_amd import _lib
    ps = _params(name)
    names = [n for _, n in ps]
    assert ("int", "dtype") in ps and names.count("dtype") == 1
    assert names[names.index("dtype") + 1] == FUSED[name], names     # in front of health, else of stream (gim_token_mlp_emit: of emit)
    assert names[-1] == "stream"
    args = [ctypes.c_void_p if t == "*" else _CTYPE[t] for t, _ in ps]
    assert (ctypes.c_int, args) == _lib.PROTOTYPES[name], (name, args, _lib.PROTOTYPES[name])


@pytest.mark.parametrize("tag", ["GIM_F32", 7])
@pytest.mark.parametrize("name", sorted(FUSED))
def test_a_wrong_tag_is_rejected_before_the_device_is_touched(name, tag):
    from gim_amd import _lib
    invalid = int(re.search(r"\bGIM_ERR_INVALID\s*=\s*(-?\d+)", HEADER).group(1))
    tag = _lib.GIM_F32 if tag == "GIM_F32" else tag
    assert tag not in (_lib.GIM_BF16, _lib.GIM_F16)
    keep, args = [], []
    for t, n in _params(name):
        if n == "stream":
            args.append(None)                                        # the null stream
        elif n == "emit":
            keep.append(_lib.TokenEmit())                            # zeroed
            args.append(ctypes.addressof(keep[-1]))
        elif t == "*":
            keep.append(ctypes.create_string_buffer(64))             # non-null, never read: the tag check comes first
            args.append(ctypes.addressof(keep[-1]))
        elif n == "dtype":
            args.append(tag)
        elif t == "float":
            args.append(1e-5 if n == "ln_eps" else 4.0)
        else:
            args.append(_INTS_OF.get(name, {}).get(n, _INTS[n]))
    assert getattr(_lib.lib, name)(*args) == invalid
    msg = _lib.lib.gim_last_error().decode()
    assert msg.startswith(name + ":") and f"dtype tag {tag}" in msg, msg


# ---- the entry points that take fp32 too (GIM_ROUTE_ANY / GIM_ROUTE_ANY2 / GIM_TAG_ANY): the list comes from the header ---------------------
TAGS = ("dtype", "out_dtype", "x_dtype")
TAGGED = sorted(m.group(1) for m in re.finditer(r"^\s*int\s+(gim_\w+)\s*\(([^;]*?)\)\s*;", HEADER, re.S | re.M)
                if re.search(r"\bint\s+(%s)\s*(,|$)" % "|".join(TAGS), m.group(2)))
ANY = [n for n in TAGGED if n not in FUSED]
# gim_stem7x7 alone takes the two 16-bit kinds side by side (the bf16 mode reads an fp16 image and writes bf16: `out_dtype` picks the
# conversion, `dtype` the flavour); what it refuses is fp32 -- or no kind -- in either position
MIXED_16_IS_LEGAL = {"gim_stem7x7"}
_INTS_ANY = {"storage": 0, "act": 0, "split": 1, "cert_init": 0, "kv_shift": 0, "b_off": 0, "c_off": 0, "D": 64, "K": 8, "nb": 1, "r": 2,
             "cell": 8, "hw": 64, "rows": 64, "E": 32, "n_slots": 2}


def _tag_positions(name):
    return [i for i, (t, n) in enumerate(_params(name)) if t == "int" and n in TAGS]


def _bad_tag_cases():
    """(entry point, {parameter index: tag}) -- every combination here is one the library must refuse: NEVER a valid one, the buffers
    are 64 host bytes"""
    F32, BF16, F16 = 0, 1, 2
    cases = []
    for name in ANY:
        pos = _tag_positions(name)
        fill = BF16 if name in MIXED_16_IS_LEGAL else F32
        for p in pos:                                                   # a tag that names no kind, in each position in turn
            cases.append((name, {q: (7 if q == p else fill) for q in pos}))
        if len(pos) == 2:
            pairs = [(F32, BF16), (F16, F32)] if name in MIXED_16_IS_LEGAL else [(BF16, F16), (F16, BF16)]
            cases += [(name, dict(zip(pos, pr))) for pr in pairs]
    return cases


def test_the_header_lists_the_tagged_entry_points():
    from gim_amd import _lib
    assert (_lib.GIM_F32, _lib.GIM_BF16, _lib.GIM_F16) == (0, 1, 2)
    assert len(TAGGED) >= 40, TAGGED                                   # 43 today: 9 fused + 34 that take fp32 too
    assert set(FUSED) <= set(TAGGED) and len(ANY) >= 34, ANY
    assert {"gim_sdpa", "gim_lg_rotary", "gim_layernorm_act", "gim_resize_image", "gim_layernorm_residual", "gim_stem7x7",
            "gim_lg_gather_pairs", "gim_dkm_flow_update"} <= set(ANY)
    two = sorted(n for n in ANY if len(_tag_positions(n)) == 2)
    assert two == ["gim_layernorm_residual", "gim_linear_attention_apply", "gim_linear_attention_short", "gim_local_corr",
                   "gim_resize_bilinear", "gim_sdpa", "gim_stem7x7"], two
    assert all(1 <= len(_tag_positions(n)) <= 2 for n in ANY)


@pytest.mark.parametrize("name,tags", _bad_tag_cases(), ids=lambda v: v if isinstance(v, str) else "-".join(str(t) for t in v.values()))
def test_an_unknown_or_mixed_tag_is_rejected_before_the_device_is_touched(name, tags):
    from gim_amd import _lib
    invalid = int(re.search(r"\bGIM_ERR_INVALID\s*=\s*(-?\d+)", HEADER).group(1))
    known = (_lib.GIM_F32, _lib.GIM_BF16, _lib.GIM_F16)
    vals = list(tags.values())
    assert any(t not in known for t in vals) or (name in MIXED_16_IS_LEGAL and _lib.GIM_F32 in vals) or \
        (name not in MIXED_16_IS_LEGAL and set(vals) == {_lib.GIM_BF16, _lib.GIM_F16}), "this test never passes a valid combination"
    keep, args = [], []
    for i, (t, n) in enumerate(_params(name)):
        if n == "stream":
            args.append(None)
        elif t == "*":
            keep.append(ctypes.create_string_buffer(64))                 # non-null, never read: the tag check comes first
            args.append(ctypes.addressof(keep[-1]))
        elif i in tags:
            args.append(tags[i])
        elif t == "float":
            args.append(1e-5 if "eps" in n else 0.5)
        else:
            args.append(_INTS_ANY.get(n, _INTS.get(n, 256 if n.startswith("ld") else 8)))
    assert getattr(_lib.lib, name)(*args) == invalid
    msg = _lib.lib.gim_last_error().decode()
    said = f"dtype tag {vals[0]}" if len(vals) == 1 else f"dtype tags {vals[0]}, {vals[1]}"
    assert msg.startswith(name + ":") and said in msg, msg
