"""gim_balanced_sample_pairs (csrc/sample_pairs.hip) in the built libgimhip.so, without a GPU: both symbols are exported and bound
with the header's prototypes, they moved no ABI revision, the argument checks return before a launch, the workspace size grows with
every argument and ends where the documented layout ends, and the kernels are gfx950 wave64 code objects without scratch (read from
the AMDGPU metadata notes like tests/test_feature_bank_resources_cpu.py)."""
import ctypes
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_feature_bank_resources", os.path.join(ROOT, "tests", "test_feature_bank_resources_cpu.py"))
_fb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_fb)

NEW = ("gim_balanced_sample_pairs_ws_bytes", "gim_balanced_sample_pairs")
_fb._CTYPE.setdefault("uint32_t", ctypes.c_uint32)
# the nine kernels of the launch sequence, as the demangled names spell them (all take the by-value argument struct)
KERNELS = ("sp_keys_kernel<false>(SpArgs", "sp_keys_kernel<true>(SpArgs", "sp_pick_kernel<0>(SpArgs", "sp_pick_kernel<1>(SpArgs",
           "sp_hist_kernel<0>(SpArgs", "sp_hist_kernel<1>(SpArgs", "sp_count_kernel<0>(SpArgs", "sp_count_kernel<1>(SpArgs",
           "sp_scan_kernel<0>(SpArgs", "sp_scan_kernel<1>(SpArgs", "sp_emit_kernel<0>(SpArgs", "sp_emit_kernel<1>(SpArgs",
           "sp_kde_kernel(SpArgs")


def test_symbols_are_exported_with_the_headers_prototypes():
    from gim_amd import _lib
    for name in NEW:
        assert name in _lib.PROTOTYPES
        fn = getattr(_lib.lib, name)                   # AttributeError: the symbol is missing from the library
        res, args = _fb._header_prototype(name)
        assert (res, args) == _lib.PROTOTYPES[name], (name, res, args, _lib.PROTOTYPES[name])
        assert fn.restype is res and list(fn.argtypes) == args
    assert len(_lib.PROTOTYPES["gim_balanced_sample_pairs"][1]) == 13
    assert "sample_pairs.hip" in __import__("gim_amd.build", fromlist=["SOURCES"]).SOURCES


def test_abi_revision_is_still_115():
    from gim_amd import _lib, ops
    assert _lib.lib.gim_version() == _lib.ABI_VERSION == 115          # added exports: they moved no ABI revision
    src = open(_fb.HEADER).read()
    assert re.findall(r"^ \* (\d{3})\b", src, re.M)[-1] == "115"
    assert "#define GIM_SAMPLE_MAX_PAIRS 16" in src and ops.SAMPLE_MAX_PAIRS == 16


def test_argument_checks_return_before_a_launch():
    from gim_amd import _lib
    L = _lib.lib
    f = L.gim_balanced_sample_pairs
    buf = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256     # host memory: a call that passed the checks would hand it to a kernel
    inv = -1                                            # GIM_ERR_INVALID
    assert "GIM_ERR_INVALID = -1" in open(_fb.HEADER).read()
    good = [p, p, p, p, p, p, p, 2, 960, 50, 0.05, 0, None]
    for i in range(7):                                  # every pointer in turn
        a = list(good)
        a[i] = None
        assert f(*a) == inv, i
        assert b"NULL" in L.gim_last_error()
    for pos, bad in ((7, 0), (7, 17), (7, -1), (8, 0), (8, -5), (9, 0), (9, -1)):      # B = 0, B = 17, n = 0, num = 0
        a = list(good)
        a[pos] = bad
        assert f(*a) == inv, (pos, bad)
        assert b"balanced_sample_pairs" in L.gim_last_error()
    a = list(good)
    a[3] = p + 4                                        # sparse rows are written 16 bytes at a time
    assert f(*a) == inv and b"aligned" in L.gim_last_error()
    for B, n, num in ((0, 960, 50), (2, 0, 50), (2, 960, 0)):
        assert L.gim_balanced_sample_pairs_ws_bytes(B, n, num) == 0


def test_ws_bytes_grows_with_every_argument_and_matches_the_layout():
    from gim_amd import _lib, ops
    wb = _lib.lib.gim_balanced_sample_pairs_ws_bytes
    Bs, ns, nums = (1, 2, 3, 4, 8, 15, 16), (1, 7, 960, 961, 2048, 2049, 300_000, 1152 * 3072), (1, 50, 51, 512, 513, 5000, 8192, 10000)
    for B in Bs:
        for n in ns:
            for num in nums:
                got = wb(B, n, num)
                assert got == ops.balanced_sample_pairs_layout(B, n, num)["bytes"] and got > 0 and got % 256 == 0, (B, n, num)
    for n in ns:
        for num in nums:
            v = [wb(B, n, num) for B in Bs]
            assert v == sorted(v) and v[-1] > v[0]
    for B in Bs:
        for num in nums:
            v = [wb(B, n, num) for n in ns]
            assert v == sorted(v) and v[-1] > v[0]
        for n in ns:
            v = [wb(B, n, num) for num in nums]
            assert v == sorted(v)                       # K1 = min(4 * num, n): flat once 4 * num passes n
            if n >= 4 * nums[-1]:
                assert len(set(v)) > 4
    # the full hloc size: 16 pairs of 1152 x 3072 certainties, 8192 samples -- the key words alone pass 2^27 bytes
    lay = ops.balanced_sample_pairs_layout(16, 1152 * 3072, 8192)
    assert lay["rows"][0] == 16 * 1152 * 3072 * 4 and lay["rows"][2] == (16, 32768, 4)


def test_python_wrappers_refuse_what_the_library_would_misread():
    torch = pytest.importorskip("torch")
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    with pytest.raises(GimHipError, match="device"):
        ops.balanced_sample_pairs(torch.zeros(1, 8, 4), torch.zeros(1, 8), [(1, 2)], 4, 0.05, False)     # no CPU fallback


def test_kernels_target_gfx950_without_scratch():
    ks = _fb._kr._kernels()      # asserts the gfx950 target of every code object it parses
    for key in KERNELS:
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert hit, f"{key}...) not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
            assert regs <= 64, f"{n}: {regs} VGPRs"     # the KDE body holds 54 (as kde_kernel does); 4 workgroups of 256 per CU need <= 128
    # the per-pair kernels kept their place: the shared helpers moved, not the kernels
    assert any(n.startswith("kde_kernel(") for n in ks) and any(n.startswith("ws_keys_kernel(") for n in ks)
