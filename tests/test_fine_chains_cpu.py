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


def test_one_patch_list_call_per_depth(monkeypatch):
    """ops.fine_tile_lists without a GPU (the library replaced by a stand-in that notes the entry and its arguments): the C entry of each
    depth, the buffer sizes, the fields a depth does not build, and the refusal of a pair range below depth 3"""
    import pytest
    import torch
    from gim_amd import ops
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(ops, "lib", Lib())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)
    ids, cnt = torch.zeros(3, 5, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    bs = 2
    one = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 36, 72)            # no whole patches: ceil(36 / 8) x ceil(72 / 32)
    assert one.tiles.numel() == 2 * bs * 5 * 3 and one.n_tiles.numel() == 1 and one[2:] == (None,) * 4
    own = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 32, 64, tiles=one.tiles, n_tiles=one.n_tiles)
    assert own.tiles is one.tiles and own.n_tiles is one.n_tiles and calls[-1][1][-2] == one.tiles.numel()
    two = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 32, 64, depth=2)
    assert two.tiles.numel() == two.tiles4.numel() == 2 * bs * 4 * 2 and two.n_tiles4.numel() == 1 and two[4:] == (None, None)
    three = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 32, 64, depth=3)
    ranged = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 32, 64, depth=3, b_range=(1, 2))
    for t in (three, ranged):
        assert t.tiles.numel() == t.tiles4.numel() == 16 * bs and tuple(t.tilesq.shape) == (3, 4 * bs) and t.n_tilesq.numel() == 3
        assert t.tiles4.data_ptr() == t.tiles.data_ptr() + 4 * 16 * bs and t.tilesq.data_ptr() == t.tiles.data_ptr() + 8 * 16 * bs   # one buffer
    assert [c[0] for c in calls] == ["gim_fine_tile_list", "gim_fine_tile_list", "gim_fine_tile_lists", "gim_fine_tile_lists4",
                                     "gim_fine_tile_lists4_range"]
    assert calls[-1][1][-3:-1] == (1, 2) and calls[-1][1][4] == 5                           # b_lo, b_hi in front of the stream; the capacity
    assert [len(c[1]) for c in calls] == [len(_lib_args(c[0])) for c in calls]
    for depth in (1, 2):
        with pytest.raises(ValueError, match="pair range"):
            ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 32, 64, depth=depth, b_range=(0, 1))
    with pytest.raises(AssertionError):
        ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, 8, 8, 4, 24, 64, depth=3)       # the quarter map is not whole patches
    assert len(calls) == 5


def _lib_args(name):
    from gim_amd import _lib
    return _lib.PROTOTYPES[name][1]
