"""gim_conv2d_ups_tiles / gim_conv_ups_tiles_supported / gim_fine_tile_lists in the built libgimhip.so, without a GPU: the symbols are
exported and bound with the header's signatures, they moved no ABI revision, the entry refuses malformed arguments on the host, and the
list-walking instantiation of the upsample-carrying tile stays inside the register / scratch budget of the dense one (read from the
AMDGPU metadata notes like tests/test_kernel_resources_cpu.py, whose table keeps the dense instantiations)."""
import ctypes
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
_kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kr)

_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    """(restype, argtypes) of `name` as include/gim_hip.h declares it; a gim_conv_args pointer is the ctypes mirror's pointer type"""
    from gim_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if "gim_conv_args" in a:
            args.append(ctypes.POINTER(_lib.ConvArgs))
        elif "*" in a:
            args.append(ctypes.c_void_p)
        else:
            args.append(_CTYPE[a.replace("const", "").split()[0]])
    return _CTYPE[m.group(1)], args


@pytest.mark.parametrize("name,nargs", [("gim_conv2d_ups_tiles", 5), ("gim_conv_ups_tiles_supported", 1), ("gim_fine_tile_lists", 17)])
def test_exported_with_the_headers_signature(name, nargs):
    from gim_amd import _lib
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib, name)                      # AttributeError: the symbol is missing from the library
    res, args = _header_prototype(name)
    assert (res, args) == _lib.PROTOTYPES[name], (res, args, _lib.PROTOTYPES[name])
    assert fn.restype is res and list(fn.argtypes) == args and len(args) == nargs


def test_the_list_entries_take_the_arguments_of_their_dense_twins():
    from gim_amd import _lib
    P = _lib.PROTOTYPES
    assert P["gim_conv2d_ups_tiles"] == P["gim_conv3x3_halo_tiles"]
    assert P["gim_conv_ups_tiles_supported"] == P["gim_conv_ups_supported"]
    old, new = P["gim_fine_tile_list"][1], P["gim_fine_tile_lists"][1]
    assert new == old[:13] + [ctypes.c_void_p, ctypes.c_void_p] + old[13:]     # tiles4 / n_tiles4 in front of tiles_cap


def test_abi_revision_and_the_answer_to_an_older_library():
    """the entries arrived within the current revision (no structure or prototype changed: the header, the mirror and the library agree on it);
    a library of the same revision built before them is refused at load with the rebuild message, not later with a missing symbol"""
    from gim_amd import _lib
    assert _lib.ABI_VERSION == _lib.lib.gim_version()
    assert re.findall(r"^ \* (\d{3})\b", open(HEADER).read(), re.M)[-1] == str(_lib.ABI_VERSION)
    saved = dict(_lib.PROTOTYPES)
    _lib.PROTOTYPES["gim_entry_of_a_newer_tree"] = (ctypes.c_int, [])
    try:
        with pytest.raises(ImportError, match="older tree, rebuild"):
            _lib._load()
    finally:
        _lib.PROTOTYPES.clear()
        _lib.PROTOTYPES.update(saved)


def test_host_argument_checks_need_no_gpu():
    from gim_amd import _lib
    a = _lib.ConvArgs()
    assert _lib.lib.gim_conv_ups_tiles_supported(None) == 0 and _lib.lib.gim_conv_ups_tiles_supported(ctypes.byref(a)) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert _lib.lib.gim_conv2d_ups_tiles(None, p, p, 4, None) != 0
    assert _lib.lib.gim_conv2d_ups_tiles(ctypes.byref(a), None, p, 4, None) != 0
    assert _lib.lib.gim_conv2d_ups_tiles(ctypes.byref(a), p, p, -1, None) != 0
    a.dtype = a.out_dtype = _lib.GIM_BF16
    assert _lib.lib.gim_conv2d_ups_tiles(ctypes.byref(a), p, p, 4, None) != 0          # no `ups`, no geometry
    assert b"gim_conv_ups_tiles_supported" in _lib.lib.gim_last_error()
    assert _lib.lib.gim_fine_tile_lists(p, p, p, p, 1, 1, 8, 8, 4, 32, 32, p, p, None, p, 8, None) != 0   # tiles4 missing


# kernel (substring of the demangled name) -> (max VGPRs incl. AGPRs, max scratch bytes per lane).  Values of the tree that produced
# profiles/lateral_sparse_ab.txt, a few bytes of slack on the known spill (the convention of tests/test_kernel_resources_cpu.py, whose
# table keeps the dense instantiations: 24 B / 52 B there):
#   igemm_persistent_tiles_kernel<.., true>   256 registers,  0 B scratch, 0 spilled   (N = 196, fragment skip: the forward's lateral)
#   igemm_persistent_tiles_kernel<.., false>  256 registers, 36 B scratch, 8 spilled
#   fine_tile_list_kernel<false> / <true>      26 / 45 registers, no scratch
HOT = {
    "igemm_persistent_tiles_kernel<256, 256, 4, 2, true>": (256, 0),
    "igemm_persistent_tiles_kernel<256, 256, 4, 2, false>": (256, 40),
    "fine_tile_list_kernel<true>": (64, 0),
    "fine_tile_list_kernel<false>": (32, 0),
}


def test_list_walking_kernels_stay_inside_the_budget():
    ks = _kr._kernels()
    for key, (max_regs, max_scratch) in HOT.items():
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert hit, f"{key} not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert regs <= max_regs and scratch <= max_scratch, f"{n[:110]}: {regs} registers, {scratch} B scratch, {spills} spilled registers"
