"""gim_fine_tile_lists4_range in the built libgimhip.so, without a GPU: the symbol is exported and bound with the header's signature -- the
arguments of gim_fine_tile_lists4 with the pair range b_lo, b_hi in front of the stream --, it arrived within the current ABI revision (the
header, the ctypes mirror and the library agree on the number, and a library built before it is refused at load by the symbol check of
gim_amd/_lib.py, tests/test_ups_tiles_cpu.py), the entry refuses a malformed range on the host, and the `fine_chains` switch of gim_loftr
reads its config key and GIM_FLAGS."""
import ctypes
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_ups_tiles_cpu_fc", os.path.join(ROOT, "tests", "test_ups_tiles_cpu.py"))
_ut = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ut)


def test_exported_with_the_headers_signature():
    from gim_amd import _lib
    name = "gim_fine_tile_lists4_range"
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib, name)                      # AttributeError: the symbol is missing from the library
    res, args = _ut._header_prototype(name)
    assert (res, args) == _lib.PROTOTYPES[name], (res, args, _lib.PROTOTYPES[name])
    assert fn.restype is res and list(fn.argtypes) == args and len(args) == 22
    old = _lib.PROTOTYPES["gim_fine_tile_lists4"][1]
    assert args == old[:-1] + [ctypes.c_int, ctypes.c_int] + old[-1:]     # b_lo / b_hi in front of the stream


def test_abi_revision_is_the_headers_and_the_librarys():
    from gim_amd import _lib
    assert _lib.ABI_VERSION == _lib.lib.gim_version()
    assert re.findall(r"^ \* (\d{3})\b", open(_ut.HEADER).read(), re.M)[-1] == str(_lib.ABI_VERSION)


def test_host_argument_checks_need_no_gpu():
    from gim_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    R = _lib.lib.gim_fine_tile_lists4_range
    for lo, hi in ((-1, 1), (0, 3), (2, 1)):          # bs = 2
        assert R(p, p, p, p, 1, 2, 8, 8, 4, 32, 64, p, p, p, p, 16, p, p, 4, lo, hi, None) != 0
        assert b"pair range" in _lib.lib.gim_last_error()
    assert R(p, p, p, p, 1, 2, 8, 8, 4, 32, 64, p, p, p, p, 16, None, p, 4, 0, 2, None) != 0     # tilesq missing
    assert R(p, p, p, p, 1, 2, 8, 8, 4, 24, 64, p, p, p, p, 16, p, p, 4, 0, 2, None) != 0        # H % 16 != 0
    assert b"whole 8 x 32 patches" in _lib.lib.gim_last_error()
    assert R(p, p, p, p, 1, 2, 8, 8, 4, 32, 64, p, p, p, p, 15, p, p, 4, 0, 2, None) != 0        # 16 half patches, capacity 15


def test_fine_chains_switch():
    from gim_amd.loftr import LoFTR, get_cfg_defaults, lower_config
    cfg = lower_config(get_cfg_defaults())["loftr"]
    assert LoFTR(dict(cfg)).fine_chains == 2
    assert LoFTR(dict(cfg, fine_chains=1)).fine_chains == 1
    m = LoFTR(dict(cfg, fine_chains=4))
    assert m.fine_chains == 4
    import torch
    a = torch.empty(2, 3, 64, 128)
    m.fine_chains = 1
    k1 = m._graph_key(a, a, None, None)
    m.fine_chains = 2
    assert m._graph_key(a, a, None, None) != k1     # a captured graph keeps its chains: another value is another graph
