"""gim_conv2d_tiles / gim_conv2d_tiles_supported / gim_conv2d_big_tile / gim_fine_tile_lists4 in the built libgimhip.so, without a GPU: the
symbols are exported and bound with the header's signatures, they moved no ABI revision, the entries refuse malformed arguments on the
host, the predicate answers the cases the module asks it about, and -- from the AMDGPU metadata notes, like
tests/test_kernel_resources_cpu.py -- every instantiation that shares the included body (igemm_persistent_body.h) or the list kernel's
body kept the registers, scratch and spills it had before the 3 x 3 list walk and the quarter-level mode arrived."""
import ctypes
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_ups_tiles_cpu", os.path.join(ROOT, "tests", "test_ups_tiles_cpu.py"))
_ut = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ut)


@pytest.mark.parametrize("name,nargs", [("gim_conv2d_tiles", 5), ("gim_conv2d_tiles_supported", 1), ("gim_conv2d_big_tile", 1), ("gim_fine_tile_lists4", 20)])
def test_exported_with_the_headers_signature(name, nargs):
    from gim_amd import _lib
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib, name)                      # AttributeError: the symbol is missing from the library
    res, args = _ut._header_prototype(name)
    assert (res, args) == _lib.PROTOTYPES[name], (res, args, _lib.PROTOTYPES[name])
    assert fn.restype is res and list(fn.argtypes) == args and len(args) == nargs


def test_the_list_entries_take_the_arguments_of_their_twins():
    from gim_amd import _lib
    P = _lib.PROTOTYPES
    assert P["gim_conv2d_tiles"] == P["gim_conv2d_ups_tiles"] == P["gim_conv3x3_halo_tiles"]
    assert P["gim_conv2d_tiles_supported"] == P["gim_conv2d_big_tile"] == P["gim_conv_ups_tiles_supported"]
    old, new = P["gim_fine_tile_lists"][1], P["gim_fine_tile_lists4"][1]
    assert new == old[:16] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + old[16:]     # tilesq / n_tilesq / tilesq_cap in front of the stream
    assert _lib.ABI_VERSION == _lib.lib.gim_version() == 115                                  # added within the revision


def _args(_lib, B=2, H=16, W=64, npad=256, N=256, kpad=9 * 256, lds=1):
    a = _lib.ConvArgs()
    a.dtype = a.out_dtype = _lib.GIM_F16
    a.B, a.H, a.W, a.Ho, a.Wo = B, H, W, H, W
    a.stride, a.pad = 1, 1
    a.ldx, a.ldy = 256, N
    a.N, a.npad, a.kpad = N, npad, kpad
    a.x_bytes = B * H * W * 256 * 2
    a.use_lds_dma = lds
    return a


def test_predicates_need_no_gpu():
    from gim_amd import _lib
    sup = lambda a: _lib.lib.gim_conv2d_tiles_supported(ctypes.byref(a))
    big = lambda a: _lib.lib.gim_conv2d_big_tile(ctypes.byref(a))
    assert _lib.lib.gim_conv2d_tiles_supported(None) == 0 and _lib.lib.gim_conv2d_big_tile(None) == 0
    assert sup(_lib.ConvArgs()) == 0
    for dt in (_lib.GIM_F16, _lib.GIM_BF16):
        a = _args(_lib)
        a.dtype = a.out_dtype = dt
        assert sup(a) == 1
    assert sup(_args(_lib, N=200)) == 1
    bad = []
    for field, value in (("stride", 2), ("pad", 0), ("H", 12), ("W", 48), ("npad", 128), ("split16", 1), ("act_cols", 128), ("use_lds_dma", 0),
                         ("use_lds_dma", 2), ("dtype", _lib.GIM_F32), ("out_dtype", _lib.GIM_F32), ("res", 1), ("ups", 1), ("Ho", 8), ("B", 32768)):
        a = _args(_lib)
        setattr(a, field, value)
        if field in ("H", "W"):                      # keep the output map the input map: only the patch condition is under test
            setattr(a, field + "o", value)
        if sup(a) != 0:
            bad.append((field, value))
    assert not bad, bad
    # the dense launch: 8 tiles go to another tile, the benchmark's 1 200 (16 x 120 x 160) and a forced launch to the 256 x 256 one
    assert big(_args(_lib)) == 0 and big(_args(_lib, lds=3)) == 1 and big(_args(_lib, B=16, H=120, W=160)) == 1
    assert big(_args(_lib, B=16, H=120, W=160, N=200)) == 1 and big(_args(_lib, B=16, H=120, W=160, npad=128, N=128)) == 0


def test_host_argument_checks_need_no_gpu():
    from gim_amd import _lib
    a = _lib.ConvArgs()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert _lib.lib.gim_conv2d_tiles(None, p, p, 4, None) != 0
    assert _lib.lib.gim_conv2d_tiles(ctypes.byref(a), None, p, 4, None) != 0
    assert _lib.lib.gim_conv2d_tiles(ctypes.byref(a), p, None, 4, None) != 0
    assert _lib.lib.gim_conv2d_tiles(ctypes.byref(_args(_lib)), p, p, -1, None) != 0
    assert _lib.lib.gim_conv2d_tiles(ctypes.byref(a), p, p, 4, None) != 0          # no geometry
    assert b"gim_conv2d_tiles_supported" in _lib.lib.gim_last_error()
    L4 = _lib.lib.gim_fine_tile_lists4
    assert L4(p, p, p, p, 1, 1, 8, 8, 4, 32, 64, p, p, p, p, 8, None, p, 2, None) != 0     # tilesq missing
    assert L4(p, p, p, p, 1, 1, 8, 8, 4, 24, 64, p, p, p, p, 8, p, p, 2, None) != 0        # H % 16 != 0
    assert b"whole 8 x 32 patches" in _lib.lib.gim_last_error()
    assert L4(p, p, p, p, 1, 1, 8, 8, 4, 32, 96, p, p, p, p, 8, p, p, 2, None) != 0        # W % 64 != 0
    assert L4(p, p, p, p, 1, 1, 8, 8, 4, 32, 64, p, p, p, p, 8, p, p, 1, None) != 0        # 2 quarter patches, capacity 1
    assert L4(p, p, p, p, 1, 64, 8, 8, 4, 512, 512, p, p, p, p, 10 ** 6, p, p, 10 ** 6, None) != 0   # 131 072 + 32 768 flags
    assert b"flags of the one-workgroup kernel" in _lib.lib.gim_last_error()


# kernel (substring of the demangled name) -> (VGPRs incl. AGPRs, scratch bytes per lane, spilled registers), the worse of the two 16-bit
# flavours' objects.  EXACT: the figures of the parent tree (the one that produced profiles/lateral_sparse_ab.txt) -- the included body
# and the list kernel's body gained a mode each, and no existing instantiation may pay for it.
UNCHANGED = {
    "igemm_persistent_kernel<128, 128, 2, 2, false, false, false, false, false>": (239, 0, 0),
    "igemm_persistent_kernel<128, 128, 2, 2, false, false, true, false, false>": (241, 0, 0),
    "igemm_persistent_kernel<128, 128, 2, 2, false, true, false, false, false>": (227, 0, 0),
    "igemm_persistent_kernel<128, 128, 2, 2, false, true, true, false, false>": (256, 168, 41),
    "igemm_persistent_kernel<128, 128, 2, 2, true, false, false, false, false>": (201, 0, 0),
    "igemm_persistent_kernel<128, 128, 2, 2, true, false, true, false, false>": (219, 0, 0),
    "igemm_persistent_kernel<128, 128, 2, 2, true, true, false, false, false>": (189, 0, 0),
    "igemm_persistent_kernel<128, 128, 2, 2, true, true, true, false, false>": (245, 0, 0),
    "igemm_persistent_kernel<256, 192, 8, 1, true, true, false, false, false>": (223, 0, 0),
    "igemm_persistent_kernel<256, 256, 4, 2, false, false, false, false, false>": (256, 48, 13),
    "igemm_persistent_kernel<256, 256, 4, 2, false, false, false, true, false>": (256, 92, 25),
    "igemm_persistent_kernel<256, 256, 4, 2, false, true, false, false, false>": (256, 12, 2),
    "igemm_persistent_kernel<256, 256, 4, 2, false, true, false, true, false>": (256, 72, 20),
    "igemm_persistent_kernel<256, 256, 4, 2, true, true, false, false, false>": (256, 28, 6),      # the dense layer2_outconv2 first layer
    "igemm_persistent_kernel<256, 256, 4, 2, true, true, false, false, true>": (256, 52, 12),      # the dense layer2_outconv + upsample-add
    "igemm_persistent_kernel<256, 256, 4, 2, true, true, false, true, false>": (256, 0, 0),        # the dense 196-channel 3 x 3 layers
    "igemm_persistent_kernel<256, 256, 4, 2, true, true, false, true, true>": (256, 24, 8),
    "igemm_persistent_kernel<256, 64, 4, 1, false, false, false, false, false>": (256, 12, 2),
    "igemm_persistent_kernel<256, 64, 4, 1, false, false, true, false, false>": (247, 0, 0),
    "igemm_persistent_kernel<256, 64, 4, 1, false, true, false, false, false>": (247, 0, 0),
    "igemm_persistent_kernel<256, 64, 4, 1, false, true, true, false, false>": (256, 244, 67),
    "igemm_persistent_kernel<256, 64, 4, 1, true, false, false, false, false>": (213, 0, 0),
    "igemm_persistent_kernel<256, 64, 4, 1, true, false, true, false, false>": (231, 0, 0),
    "igemm_persistent_kernel<256, 64, 4, 1, true, true, false, false, false>": (201, 0, 0),
    "igemm_persistent_kernel<256, 64, 4, 1, true, true, true, false, false>": (256, 0, 0),
    "igemm_persistent_tiles_kernel<256, 256, 4, 2, false>": (256, 36, 8),
    "igemm_persistent_tiles_kernel<256, 256, 4, 2, true>": (256, 0, 0),
    "fine_tile_list_kernel<false>": (26, 0, 0),
    "fine_tile_list_kernel<true>": (45, 0, 0),
}

# the new instantiations -> (max VGPRs, max scratch bytes).  As built:
#   igemm_conv_tiles_kernel<.., true>    256 registers,  0 B scratch, 0 spilled   (N = 196, fragment skip: layer2_outconv2's second layer)
#   igemm_conv_tiles_kernel<.., false>   256 registers, 16 B scratch, 3 spilled   (its first layer; the dense twin: 28 B, 6 spilled)
#   fine_tile_lists4_kernel               45 registers, no scratch
NEW = {
    "igemm_conv_tiles_kernel<256, 256, 4, 2, true>": (256, 0),
    "igemm_conv_tiles_kernel<256, 256, 4, 2, false>": (256, 28),     # never worse than the dense launch it replaces
    "fine_tile_lists4_kernel": (64, 0),
}


def test_existing_instantiations_kept_their_resources_and_the_new_ones_fit():
    ks = _ut._kr._kernels()
    seen = {n for n in ks if any(n.replace("void ", "").startswith(p) for p in ("igemm_persistent_kernel<", "igemm_persistent_tiles_kernel<", "fine_tile_list_kernel<"))}
    assert len(seen) == len(UNCHANGED), sorted(seen)           # no instantiation of the shared bodies appeared or left
    wrong = []
    for key, want in UNCHANGED.items():
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert len(hit) == 1, (key, hit)
        if hit[0][1] != want:
            wrong.append(f"{key}: {hit[0][1]} (registers, scratch, spills), the parent tree has {want}")
    assert not wrong, "\n".join(wrong)
    for key, (max_regs, max_scratch) in NEW.items():
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert len(hit) == 1, (key, hit)
        regs, scratch, spills = hit[0][1]
        print(f"{key}: {regs} registers, {scratch} B scratch, {spills} spilled")
        assert regs <= max_regs and scratch <= max_scratch, (key, hit[0][1])
