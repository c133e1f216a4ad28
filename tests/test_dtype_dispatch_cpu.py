"""The one dtype convention of the C ABI (include/gim_hip.h, csrc/gim_common.h: GIM_TWIN / GIM_TO_F16 / GIM_ROUTE_H16), without a GPU: the
header and the ctypes mirror declare no `*_f16` twin, every fused entry point carries an `int dtype` tag where the header says it sits,
and a tag that names no 16-bit kind is refused before a pointer is read or the HIP runtime is called -- which is why these calls are safe on
a machine without a device: the pointers are addresses of small host buffers."""
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
