"""gim_slot_copy (csrc/feature_bank.hip) in the built libgimhip.so, without a GPU: the symbol is exported and bound, its ctypes
signature is the header's prototype, it moved no ABI revision (the library is at 115), and the kernel is a gfx950 code object with no scratch and no
spills (read from the AMDGPU metadata notes like tests/test_semseg_resources_cpu.py)."""
import ctypes
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
_kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kr)

# C parameter type (pointer levels collapsed) -> the ctypes type gim_amd/_lib.py uses for it
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if "*" in a:
            args.append(ctypes.c_void_p)
        else:
            args.append(_CTYPE[a.replace("const", "").split()[0]])
    return _CTYPE[m.group(1)], args


def test_slot_copy_is_exported_with_the_headers_signature():
    from gim_amd import _lib
    assert "gim_slot_copy" in _lib.PROTOTYPES
    fn = _lib.lib.gim_slot_copy                      # AttributeError: the symbol is missing from the library
    res, args = _header_prototype("gim_slot_copy")
    assert (res, args) == _lib.PROTOTYPES["gim_slot_copy"], (res, args, _lib.PROTOTYPES["gim_slot_copy"])
    assert fn.restype is res and list(fn.argtypes) == args
    assert len(args) == 9 and args[5] is ctypes.c_int64   # block_bytes is 64-bit: a 640x480 fp32 fine map alone is 39 MB, slabs go past 2 GiB


def test_abi_revision_is_still_114():
    """(named after the revision this export arrived in; 115 gave the fused kernels their dtype tag)"""
    from gim_amd import _lib
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    src = open(HEADER).read()
    assert re.findall(r"^ \* (\d{3})\b", src, re.M)[-1] == "115"


def test_host_argument_checks_need_no_gpu():
    """the entry point refuses malformed arguments before it touches the device"""
    from gim_amd import _lib
    f = _lib.lib.gim_slot_copy
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert f(p, p, None, None, 0, 16, 0, 0, None) == 0                 # n = 0: nothing to do
    assert f(p, p, None, None, 1, 24, 1, 1, None) != 0                 # block_bytes not a multiple of 16
    assert b"multiple of 16" in _lib.lib.gim_last_error()
    assert f(p, p, None, None, 3, 16, 2, 4, None) != 0                 # identity source over more blocks than slots
    assert f(ctypes.c_void_p(p.value + 4), p, None, None, 1, 16, 1, 1, None) != 0   # misaligned slab
    assert f(p, p, None, None, -1, 16, 1, 1, None) != 0


def test_slot_copy_kernel_targets_gfx950_without_scratch():
    ks = _kr._kernels()          # asserts the gfx950 target of every code object it parses
    hit = [(n, v) for n, v in ks.items() if "slot_copy_kernel(" in n]
    assert hit, "slot_copy_kernel not found in the library"
    for n, (regs, scratch, spills) in hit:
        assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
        assert regs <= 64, f"{n}: {regs} VGPRs"     # a copy kernel: four 16-byte registers quadruples in flight plus addresses
