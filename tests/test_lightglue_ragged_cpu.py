"""Ragged keypoint counts of the gim_lightglue pair-list path without a GPU: the keypoint bank's count bookkeeping (capacity, LRU
eviction, re-insertion, n = 0), the pair-list driver's trimming to image 0's count, the four new exports (header prototype == ctypes
binding, exported by the built library, ABI revision unchanged, host-side argument checks) and the resources of the kernels that took
length tables (read from the AMDGPU metadata notes like tests/test_lightglue_pairs_cpu.py reads the bank kernels')."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_spec = importlib.util.spec_from_file_location("_kernel_resources_ragged", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
_kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kr)

NEW = ("gim_sdpa_varlen", "gim_lg_transpose_varlen", "gim_lg_assign_ragged", "gim_lg_gather_pairs_ragged")
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_counts_follow_the_slots_through_eviction_and_reinsertion():
    from gim_amd._lib import GimHipError
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(3, 8, device="cpu")                   # bookkeeping only: no kernel is launched here
    assert bank.counts == [0, 0, 0] and bank.n.dtype == torch.int32 and bank.n.shape == (3,)
    s = bank._admit(["a", "b", "c"], [8, 5, 0])               # a full image, a short one, one without keypoints
    assert bank.slot_counts(s) == [8, 5, 0] and bank.slot_counts(bank.slots(["c", "b", "a", "b"])) == [0, 5, 8, 5]
    bank.slots(["a", "c"])                                    # "b" is now the least recently used
    sd = bank._admit(["d"], [3])                              # evicts "b" and takes its slot -- with its own count
    assert sd == [s[1]] and "b" not in bank and bank.slot_counts(sd) == [3] and bank.stats.evictions == 1
    assert bank.slot_counts(bank.slots(["a", "c", "d"])) == [8, 0, 3]
    sb = bank._admit(["b"], [7])                              # re-inserted with another count; "a" goes
    assert sb == [s[0]] and "a" not in bank and bank.slot_counts(bank.slots(["b", "c", "d"])) == [7, 0, 3]
    assert bank._admit(["c"], [2]) == [s[2]] and bank.counts[s[2]] == 2       # a resident key keeps its slot, the count is overwritten
    before = (list(bank.counts), bank.table.keys())
    for bad in (9, -1):
        with pytest.raises(GimHipError, match="holds 8"):
            bank._admit(["x", "y"], [1, bad])                 # refused as a whole: nothing reserved, nothing recorded
    assert (list(bank.counts), bank.table.keys()) == before and "x" not in bank


def test_put_accepts_fewer_keypoints_than_the_capacity():
    """host tensors reach the device check whatever their count (the parent refused any count but the capacity first: 'ragged counts
    are not built'); a malformed image is still named as such"""
    from gim_amd._lib import GimHipError
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(2, 8, device="cpu")
    for n in (0, 1, 7, 8):
        with pytest.raises(GimHipError, match="device") as e:
            bank.put("img", torch.zeros(n, 2), torch.zeros(n, 256), torch.tensor([64.0, 48.0]))
        assert "ragged" not in str(e.value)
    with pytest.raises(GimHipError, match="device"):
        bank.put_many(["p", "q"], [torch.zeros(3, 2), torch.zeros(8, 2)], [torch.zeros(3, 256), torch.zeros(8, 256)], torch.ones(2, 2))
    with pytest.raises(GimHipError, match=r"descriptors \[k, 256\]"):
        bank.put("img", torch.zeros(5, 2), torch.zeros(4, 256), torch.tensor([64.0, 48.0]))
    assert len(bank) == 0


class _Group(dict):
    def create_group(self, name):
        self[name] = g = _Group()
        return g

    def create_dataset(self, name, data):
        self[name] = np.asarray(data)


def test_sparse_pair_list_trims_to_image0():
    from gim_amd import hloc_formats
    from gim_amd.bank import sparse_pair_list
    from gim_amd.lightglue import KeypointBank
    K = 6
    bank = KeypointBank(3, K, device="cpu")
    bank._admit(["a", "b", "c"], [6, 4, 0])
    seen = []

    def stub(s0, s1):   # rows padded to the capacity, as LightGlue.match_pairs returns them
        seen.append((s0, s1))
        m = np.full((len(s0), K), -1, dtype=np.int16)
        s = np.zeros((len(s0), K), dtype=np.float16)
        for r, (a, b) in enumerate(zip(s0, s1)):
            n = min(bank.counts[a], bank.counts[b])
            m[r, :n] = np.arange(n)
            s[r, :n] = 0.5
        return zip(m, s)

    pairs = [("a", "b"), ("b", "a"), ("c", "a"), ("a", "c"), ("b", "b")]
    w = _Group()
    out = sparse_pair_list(bank, pairs, 2, stub, w, None, counts0=bank.slot_counts)
    assert [len(s0) for s0, _ in seen] == [2, 2, 1]
    assert [(a, b) for a, b, _, _ in out] == pairs
    assert [len(m) for _, _, m, _ in out] == [6, 4, 0, 6, 4] == [len(s) for _, _, _, s in out]
    assert out[0][2].tolist() == [0, 1, 2, 3, -1, -1] and out[1][2].tolist() == [0, 1, 2, 3] and out[3][2].tolist() == [-1] * 6
    for (a, b), (_, _, m, s) in zip(pairs, out):
        g = w[hloc_formats.pair_key(a, b)]
        assert g["matches0"].dtype == np.int16 and g["matching_scores0"].dtype == np.float16
        assert np.array_equal(g["matches0"], m) and np.array_equal(g["matching_scores0"], s)
    # without counts nothing is cut (the other sparse matchers' call)
    assert [len(m) for _, _, m, _ in sparse_pair_list(bank, pairs, 8, stub)] == [K] * 5


def test_plugin_refuses_an_image_above_the_cap_before_any_device_work():
    from gim_amd._lib import GimHipError
    from gim_amd.hloc_matchers.gim_lightglue_hip import GimLightGlueHip
    m = GimLightGlueHip({"max_keypoints": 4})
    feats = {n: {"keypoints": np.zeros((k, 2), np.float16), "descriptors": np.zeros((256, k), np.float16), "image_size": np.array([64, 48])}
             for n, k in (("a", 3), ("b", 5))}
    with pytest.raises(GimHipError, match="'b' has 5 keypoints"):
        m.match_pairs_from_features(feats, [("a", "b")], {}, device="cpu")


# ------------------------------------------------------------------------------------------------ exports
@pytest.mark.parametrize("name", NEW)
def test_new_exports_have_the_headers_signature(name):
    from gim_amd import _lib
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib, name)                     # AttributeError: the symbol is missing from the library
    res, args = _header_prototype(name)
    want = (_lib.PROTOTYPES[name][0], [ctypes.c_void_p if isinstance(a, type) and issubclass(a, ctypes._Pointer) else a
                                       for a in _lib.PROTOTYPES[name][1]])
    assert (res, args) == want, (res, args, want)
    assert fn.restype is res and len(fn.argtypes) == len(args)


def test_abi_revision_and_old_signatures_stay():
    from gim_amd import _lib
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    assert re.findall(r"^ \* (\d{3})\b", open(HEADER).read(), re.M)[-1] == "115"
    assert _header_prototype("gim_sdpa")[1] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 12 + [ctypes.c_void_p]
    assert _header_prototype("gim_lg_transpose")[1] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    assert _header_prototype("gim_lg_gather_pairs")[1] == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    assert ctypes.sizeof(_lib.LgAssignArgs) == 13 * 8 + 6 * 4


def test_host_argument_checks_need_no_gpu():
    from gim_amd import _lib
    from gim_amd._lib import GIM_BF16, GIM_F16, GIM_F32
    L = _lib.lib
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert L.gim_sdpa_varlen(p, p, p, p, None, p, 2, 4, 8, 8, 64, 64, 256, 256, 256, 0, GIM_F32, GIM_F32, None) != 0
    assert b"length table" in L.gim_last_error()
    assert L.gim_sdpa_varlen(p, p, p, p, p, p, 2, 4, 8, 8, 64, 96, 256, 256, 256, 0, GIM_F32, GIM_F32, None) != 0     # head dim
    for tags in ((GIM_BF16, GIM_F16), (GIM_F16, GIM_BF16), (7, GIM_F32), (GIM_F32, 7)):      # two 16-bit kinds / a tag that names no kind
        assert L.gim_sdpa_varlen(p, p, p, p, p, p, 2, 4, 8, 8, 64, 64, 256, 256, 256, 0, tags[0], tags[1], None) != 0
        msg = L.gim_last_error().decode()
        assert msg.startswith("gim_sdpa_varlen:") and f"dtype tags {tags[0]}, {tags[1]}" in msg, msg
    assert L.gim_lg_transpose_varlen(p, p, p, 2, 8, 64, 256, 256, 7, None) != 0 and b"dtype tag 7" in L.gim_last_error()
    assert L.gim_lg_transpose_varlen(p, p, None, 2, 8, 64, 256, 256, GIM_F32, None) != 0
    assert L.gim_lg_transpose_varlen(p, p, p, 2, 8, 60, 256, 256, GIM_F32, None) != 0                                # Sp no multiple of 64
    a = _lib.LgAssignArgs()
    assert L.gim_lg_assign_ragged(ctypes.byref(a), None, p, None) != 0
    assert L.gim_lg_gather_pairs_ragged(p, p, p, p, None, p, p, p, p, p, 0, 8, 4, GIM_F16, GIM_BF16, 256, 512, None) == 0   # B = 0
    assert L.gim_lg_gather_pairs_ragged(p, p, p, p, None, p, p, p, p, p, 1, 8, 4, GIM_F16, GIM_BF16, 256, 512, None) != 0
    assert b"count" in L.gim_last_error()
    assert L.gim_lg_gather_pairs_ragged(p, p, p, p, p, p, p, p, p, p, 1, 8, 4, GIM_F16, GIM_F32, 512, 512, None) != 0       # cat in fp32 mode


# ------------------------------------------------------------------------------------------------ kernel resources
def _register_file_use():
    """kernel name -> registers of the unified file a lane occupies.  gfx950's `.vgpr_count` is that total already (the accumulation
    registers `.agpr_count` counts sit inside it, behind `accum_offset`), so it is read alone here -- _kr._kernels() adds the two,
    which counts a kernel's AGPRs twice."""
    import glob
    import struct
    import subprocess
    import tempfile
    yaml = pytest.importorskip("yaml")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([os.path.join(_kr.LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", _kr.LIB, fat], check=True)
        data = open(fat, "rb").read()
        pos, n = data.find(b"\x7fELF"), 0
        while pos >= 0:
            e_shoff = struct.unpack_from("<Q", data, pos + 0x28)[0]
            e_shentsize, e_shnum = struct.unpack_from("<HH", data, pos + 0x3A)
            size = e_shoff + e_shentsize * e_shnum
            open(os.path.join(td, f"co_{n}.elf"), "wb").write(data[pos:pos + size])
            n += 1
            pos = data.find(b"\x7fELF", pos + max(size, 4))
        for elf in sorted(glob.glob(os.path.join(td, "co_*.elf"))):
            txt = subprocess.run([os.path.join(_kr.LLVM, "llvm-readelf"), "--notes", elf], capture_output=True, text=True).stdout
            if "sdpa_kernel" not in txt:
                continue
            for k in yaml.safe_load(txt[txt.index("---"):txt.rindex("...")]).get("amdhsa.kernels", []):
                out[k[".name"]] = max(out.get(k[".name"], 0), k[".vgpr_count"])
    return out


@pytest.mark.parametrize("kernel,variants,max_regs", [
    ("sdpa_kernel<true, ", 8, 256),       # 16-bit operands: 4 output / head-dim variants x {uniform, varlen}; two workgroups of 4 waves per CU
    ("sdpa_kernel<false, ", 8, 256),      # fp32 operands (parity mode); at head dim 128 the budget is 512, see below
    ("lg_transpose_kernel<", 2, 64),
    ("lga_stats_kernel(", 1, 256),
    ("lga_best_kernel<", 2, 256),
    ("lga_combine_kernel(", 1, 64),
    ("lga_filter_kernel(", 1, 64),
    ("lg_gather_pairs_kernel<", 2, 48),
])
def test_kernels_with_length_tables_use_no_scratch(kernel, variants, max_regs):
    """No scratch and no spilled register in any kernel that took a length table, uniform and varlen instantiations alike.
    Register budget: 256 at two workgroups of 4 waves per CU.  The fp32-operand sdpa_kernel at head dim 128 stages 128 KiB of LDS
    tiles, so one workgroup per CU is all that fits the CU's 160 KiB: one wave per SIMD, 512 registers of the unified file."""
    ks = _kr._kernels()          # asserts the gfx950 target of every code object it parses
    hit = [(n, v) for n, v in ks.items() if kernel in n]
    assert len(hit) == variants, f"{kernel}: found {[n for n, _ in hit]}"
    wide = kernel == "sdpa_kernel<false, "
    for n, (regs, scratch, spills) in hit:
        assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
        if not (wide and ", 128, " in n):
            assert regs <= max_regs, f"{n}: {regs} VGPRs"
    if wide:
        use = {n: v for n, v in _register_file_use().items() if "sdpa_kernelILb0E" in n and "Li128E" in n}
        assert len(use) == 4 and all(256 < v <= 512 for v in use.values()), use   # above 256: the one-workgroup budget is what holds them
