"""The gim_lightglue pair-list path without a GPU: the keypoint bank's bookkeeping (slots, LRU eviction, stale encodings), the pair
batching, the three new exports (header prototype == ctypes binding, ABI revision unchanged, host-side argument checks), the hloc
plugin classes against tests/hloc_stub, the extractor's size error, and the resources of the two bank kernels (read from the AMDGPU
metadata notes like tests/test_feature_bank_resources_cpu.py)."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
_kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kr)

NEW = ("gim_lg_bank_put", "gim_lg_gather_pairs", "gim_lg_emit_hloc")
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_slot_table_and_lru():
    from gim_amd._lib import GimHipError
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(4, 8, storage="fp16", device="cpu")   # bookkeeping only: no kernel is launched here
    assert bank.desc.dtype == torch.float16 and bank.kpts.dtype == torch.float32 and bank.enc.shape == (4, 8, 64)
    assert KeypointBank(2, 8, storage="fp32", device="cpu").desc.dtype == torch.float32
    s = bank.reserve(["a", "b", "c"])
    assert sorted(s) == [0, 1, 2] and len(bank) == 3 and "a" in bank and "d" not in bank
    assert bank.slots(["c", "a", "c"]) == [s[2], s[0], s[2]]              # duplicates share a slot; "b" is now the least recently used
    sd = bank.reserve(["d"])
    assert sd == [3] and bank.stats.evictions == 0
    se = bank.reserve(["e"])                                             # full: evicts "b" and takes its slot
    assert se == [s[1]] and "b" not in bank and bank.stats.evictions == 1
    assert bank.reserve(["a"]) == [s[0]]                                 # a resident key keeps its slot (it is overwritten)
    with pytest.raises(GimHipError, match="not resident"):
        bank.slots(["a", "b"])
    with pytest.raises(GimHipError, match="not resident"):
        bank.slots(["never"])
    assert bank.slots(["e", "d", "c", "a", "e", "d", "c", "a"]) == [se[0], 3, s[2], s[0]] * 2   # more names than slots, all resident
    with pytest.raises(ValueError):
        bank.reserve(["x", "x"])
    with pytest.raises(GimHipError):
        bank.reserve(list("vwxyz"))                                      # more images in one insertion than slots
    with pytest.raises(ValueError):
        KeypointBank(4, 8, storage="bf16", device="cpu")
    with pytest.raises(GimHipError, match="outside"):
        bank.slot_tensor([0, 4])
    with pytest.raises(GimHipError, match="int32"):
        bank.slot_tensor(torch.zeros(2, dtype=torch.int64))
    assert bank.slot_tensor([3, 0]).dtype == torch.int32
    # there is no CPU path: an insertion of host tensors is refused, and the refused image is not reported resident with stale data
    with pytest.raises(GimHipError, match="device"):
        bank.put("cpu", torch.zeros(8, 2), torch.zeros(8, 256), torch.tensor([64.0, 48.0]))
    with pytest.raises(GimHipError, match="keypoints"):
        bank.put("short", torch.zeros(7, 2), torch.zeros(7, 256), torch.tensor([64.0, 48.0]))
    assert "cpu" not in bank and "short" not in bank


def test_bank_uses_the_loftr_slot_table_unchanged():
    from gim_amd.lightglue import bank as kb
    from gim_amd.loftr.bank import SlotTable
    assert kb.SlotTable is SlotTable and isinstance(kb.KeypointBank(1, 1, device="cpu").table, SlotTable)


def test_pair_batching():
    from gim_amd.lightglue.pairs import pair_batches
    pairs = [(0, 1), (0, 2), (1, 2), (2, 0), (1, 1)]
    assert pair_batches(pairs, 4) == [pairs[:4], pairs[4:]]               # a full batch and a tail of one
    assert pair_batches(pairs, 8) == [pairs] and pair_batches(pairs, 1) == [[p] for p in pairs]
    assert pair_batches(pairs, 5) == [pairs] and pair_batches([], 8) == []
    assert pair_batches(pairs + pairs, 5) == [pairs, pairs]               # nothing reordered, nothing deduplicated
    with pytest.raises(ValueError):
        pair_batches(pairs, 0)


def test_match_pair_list_of_nothing_touches_nothing():
    from gim_amd.lightglue import match_pair_list
    assert match_pair_list(None, None, [], batch_pairs=8, writer=None) == []


def test_repack_moves_the_epoch_a_bank_watches():
    from gim_amd.lightglue import LightGlue
    lg = LightGlue({"filter_threshold": 0.1})
    e0 = lg._pack_epoch
    lg.load_state_dict(lg.state_dict())
    e1 = lg._pack_epoch
    lg.float()
    assert e0 < e1 < lg._pack_epoch and lg._packed is None and lg.input_hook is None
    assert callable(lg.match_pairs)


# ------------------------------------------------------------------------------------------------ exports
@pytest.mark.parametrize("name", NEW)
def test_new_exports_have_the_headers_signature(name):
    from gim_amd import _lib
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib, name)                     # AttributeError: the symbol is missing from the library
    res, args = _header_prototype(name)
    assert (res, args) == _lib.PROTOTYPES[name], (res, args, _lib.PROTOTYPES[name])
    assert fn.restype is res and list(fn.argtypes) == args


def test_abi_revision_is_still_115():
    from gim_amd import _lib
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115      # added exports move no revision
    assert re.findall(r"^ \* (\d{3})\b", open(HEADER).read(), re.M)[-1] == "115"


def test_host_argument_checks_need_no_gpu():
    """the entry points refuse malformed arguments before they touch the device"""
    from gim_amd import _lib
    from gim_amd._lib import GIM_BF16, GIM_F16, GIM_F32
    L = _lib.lib
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    assert L.gim_lg_emit_hloc(p, p, p, p, 0, 2048, None) == 0                       # nothing to do
    assert L.gim_lg_emit_hloc(p, p, p, p, 1, 32768, None) != 0                      # does not fit int16
    assert b"32767" in L.gim_last_error()
    assert L.gim_lg_emit_hloc(p, p, odd, p, 1, 8, None) != 0                        # misaligned output
    assert L.gim_lg_bank_put(p, p, p, p, p, p, p, p, 0, 8, 4, GIM_F16, None) == 0   # n = 0
    assert L.gim_lg_bank_put(p, p, p, p, p, p, p, p, 1, 8, 4, GIM_BF16, None) != 0  # the bank stores fp32 or IEEE fp16
    assert b"storage" in L.gim_last_error()
    assert L.gim_lg_bank_put(p, p, None, p, p, p, p, p, 1, 8, 4, GIM_F16, None) != 0   # Wr without image sizes
    assert L.gim_lg_gather_pairs(p, p, p, p, p, p, p, 0, 8, 4, GIM_F16, GIM_BF16, 256, 512, None) == 0   # B = 0
    assert L.gim_lg_gather_pairs(p, p, p, p, p, p, p, 1, 8, 4, GIM_F16, GIM_F32, 512, 512, None) != 0    # fp32 mode writes once: cat must be NULL
    assert b"cat" in L.gim_last_error()
    assert L.gim_lg_gather_pairs(p, p, p, p, p, None, p, 1, 8, 4, GIM_F16, GIM_BF16, 256, 512, None) != 0
    assert L.gim_lg_gather_pairs(p, p, p, p, p, p, p, 1, 8, 4, GIM_F16, GIM_BF16, 250, 512, None) != 0   # rows must stay 16-byte aligned
    assert L.gim_lg_gather_pairs(p, p, p, p, odd, p, p, 1, 8, 4, GIM_F16, GIM_BF16, 256, 512, None) != 0


def test_emit_hloc_wrapper_rejects_wide_images_on_the_host():
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    r = ops.AssignResult()
    r.matches0, r.mscores0 = torch.zeros(1, 32768, dtype=torch.int64), torch.zeros(1, 32768)
    with pytest.raises(GimHipError, match="32767"):
        ops.lg_emit_hloc(r)


# ------------------------------------------------------------------------------------------------ hloc plugins
def test_hloc_plugins_are_found():
    from hloc.utils.base_model import BaseModel, dynamic_load

    import gim_amd.hloc_extractors as extractors
    import gim_amd.hloc_matchers as matchers
    Matcher = dynamic_load(matchers, "gim_lightglue_hip")
    assert issubclass(Matcher, BaseModel) and set(Matcher.required_inputs) >= {"keypoints0", "descriptors1", "image_size0"}
    m = Matcher({})
    assert m.conf["filter_threshold"] == 0.1 and m.conf["batch_pairs"] == 8 and m.net.conf["filter_threshold"] == 0.1
    assert callable(m.match_pairs_from_features) and m.match_pairs_from_features({}, [], {}) == []
    Extractor = dynamic_load(extractors, "gim_superpoint_hip")
    assert issubclass(Extractor, BaseModel) and Extractor.required_inputs == ["image"]
    e = Extractor({})
    assert e.net.conf["max_num_keypoints"] == 2048 and e.net.conf["force_num_keypoints"] and e.net.conf["nms_radius"] == 3


def test_extractor_names_a_size_that_is_no_multiple_of_8():
    from gim_amd._lib import GimHipError
    from gim_amd.hloc_extractors.gim_superpoint_hip import GimSuperPointHip
    e = GimSuperPointHip({"max_keypoints": 64})
    with pytest.raises(GimHipError, match="100x100"):      # a host tensor: the size is refused before any device work
        e({"image": torch.zeros(1, 1, 100, 100)})
    with pytest.raises(GimHipError, match="104x100"):
        e({"image": torch.zeros(1, 1, 100, 104)})


# ------------------------------------------------------------------------------------------------ kernel resources
@pytest.mark.parametrize("kernel,max_regs", [("lg_bank_put_kernel<", 64), ("lg_gather_pairs_kernel<", 48), ("lg_emit_hloc_kernel(", 48)])
def test_bank_kernels_target_gfx950_without_scratch(kernel, max_regs):
    """copy / convert kernels: 16 bytes x a few in flight per lane plus addresses -- and, for the insertion, sinf / cosf's range
    reduction.  No scratch, no spilled register, in every storage variant."""
    ks = _kr._kernels()          # asserts the gfx950 target of every code object it parses
    hit = [(n, v) for n, v in ks.items() if kernel in n]
    assert len(hit) == (1 if kernel.endswith("(") else 2), f"{kernel}: found {[n for n, _ in hit]}"
    for n, (regs, scratch, spills) in hit:
        assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
        assert regs <= max_regs, f"{n}: {regs} VGPRs"
