"""The dense matchers' feature bank without a GPU: the ABI of csrc/dense_bank.hip (struct layouts against the header, exported symbols,
argument checks that return before a launch), the slot / LRU bookkeeping of gim_amd.dense_bank.DenseFeatureBank and the geometry-table
builder of gim_amd.adapters against get_padding_size."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from test_abi_layout_cpu import ROOT, _c_fields

NEW = ("gim_dense_gather_pairs", "gim_dense_emit_pairs")


@pytest.mark.parametrize("struct,mirror", [("gim_dense_gather_args", "DenseGatherArgs"), ("gim_dense_pair_geom", "DensePairGeom")])
def test_ctypes_mirror_matches_the_header(tmp_path, struct, mirror):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("gcc not found")
    from gim_amd import _lib
    cls = getattr(_lib, mirror)
    c_names = _c_fields(struct)
    assert c_names == [f[0] for f in cls._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "gim_hip.h"', "int main(void) {", '  printf("%%zu\\n", sizeof(%s));' % struct]
    prog += ['  printf("%%zu\\n", offsetof(%s, %s));' % (struct, n) for n in c_names] + ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    for n, off in zip(c_names, out[1:]):
        assert getattr(cls, n).offset == off, (struct, n)
    if mirror == "DensePairGeom":
        assert ctypes.sizeof(cls) == 16 * 4            # one row of the [B, 16] fp32 table ops.dense_pair_geometry uploads
    else:
        assert cls.MAX == 8 and "#define GIM_DENSE_MAX_LEVELS 8" in open(os.path.join(ROOT, "include", "gim_hip.h")).read()


def test_symbols_are_exported_within_the_revision():
    from gim_amd import _lib
    for name in NEW:
        assert name in _lib.PROTOTYPES
        getattr(_lib.lib, name)                        # AttributeError: the symbol is missing from the library
    assert _lib.lib.gim_version() == _lib.ABI_VERSION == 115          # added exports: they moved no ABI revision
    assert "dense_bank.hip" in __import__("gim_amd.build", fromlist=["SOURCES"]).SOURCES


def test_argument_checks_return_before_a_launch():
    from gim_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    a = _lib.DenseGatherArgs()
    a.slab[0], a.dst[0], a.slot_bytes[0], a.n_levels = p, p + 64, 32, 1
    assert L.gim_dense_gather_pairs(ctypes.byref(a), None, 0, 4, None) == 0          # no entries: nothing to do
    assert L.gim_dense_gather_pairs(ctypes.byref(a), None, 2, 4, None) != 0          # entries without an index array
    for bad_bytes in (0, 24, -16):
        a.slot_bytes[0] = bad_bytes
        assert L.gim_dense_gather_pairs(ctypes.byref(a), p, 2, 4, None) != 0
        assert b"multiple of 16" in L.gim_last_error()
    a.slot_bytes[0] = 32
    a.slab[0] = p + 8
    assert L.gim_dense_gather_pairs(ctypes.byref(a), p, 2, 4, None) != 0 and b"aligned" in L.gim_last_error()
    a.slab[0] = p
    for levels in (0, 9):
        a.n_levels = levels
        assert L.gim_dense_gather_pairs(ctypes.byref(a), p, 2, 4, None) != 0 and b"levels" in L.gim_last_error()
    assert L.gim_dense_emit_pairs(None, None, None, None, None, None, None, 0, 10, 1, None) == 0   # B = 0
    assert L.gim_dense_emit_pairs(p, p, None, p, p, p, p, 1, 10, 1, None) != 0                      # no geometry table
    assert L.gim_dense_emit_pairs(p + 4, p, p, p, p, p, p, 1, 10, 1, None) != 0                     # sparse rows are read 16 bytes at a time


# ------------------------------------------------------------------------------------------------ bookkeeping
class _FakeModel:
    """what DenseFeatureBank needs of a DenseMatcher"""

    def __init__(self):
        self.tag = ("m", 0)

    def feature_tag(self):
        return self.tag


def test_bank_slots_lru_and_invalidation(monkeypatch):
    from gim_amd import dense_bank, ops
    from gim_amd._lib import GimHipError
    from gim_amd.dense import DenseFeatures
    copies = []
    monkeypatch.setattr(ops, "slot_copy", lambda src, dst, dst_idx=None: copies.append(list(dst_idx)))   # no device here
    m = _FakeModel()
    bank = dense_bank.DenseFeatureBank(m, 2)
    assert bank.bytes_per_image is None and len(bank) == 0

    def feats(n=1):
        return DenseFeatures({"lo1": torch.zeros(n, 4, 4, 8, dtype=torch.bfloat16), "black": torch.zeros(n, 4, 4, dtype=torch.uint8)}, m.feature_tag())

    assert bank.put_features(["a"], feats(), meta=[{"g": 1}]) == [0]
    assert bank.put_features(["b"], feats()) == [1]
    assert bank.bytes_per_image == 4 * 4 * 8 * 2 + 16 and bank.nbytes == 2 * bank.bytes_per_image
    assert bank.put_features(["a"], feats(), meta=[{"g": 2}]) == [0] and bank.meta["a"] == {"g": 2}     # overwritten in its slot
    assert bank.slots(["b", "a", "b"]) == [1, 0, 1]
    bank.slots(["a"])
    assert bank.put_features(["c"], feats()) == [1] and "b" not in bank and "b" not in bank.meta          # b was least recently used
    with pytest.raises(GimHipError, match="'b' is not resident"):
        bank.slots(["a", "b"])
    assert bank.stats.evictions == 1 and copies[-1] == [1]
    with pytest.raises(GimHipError, match="distinct"):
        bank.put_features(["x", "x"], feats(2))
    with pytest.raises(GimHipError, match="3 distinct images"):
        bank.put_features(["x", "y", "z"], feats(3))
    with pytest.raises(GimHipError, match="another module"):
        bank.check(_FakeModel())
    stale = feats()
    m.tag = ("m", 1)                                   # load_state_dict / device move / precision change of the owner
    assert "a" not in bank
    with pytest.raises(GimHipError, match="not resident"):
        bank.slots(["a"])
    assert len(bank) == 0 and bank.slabs is None and bank.meta == {} and bank.stats.invalidations == 1
    with pytest.raises(GimHipError, match="before the module changed"):
        bank.put_features(["a"], stale)
    with pytest.raises(GimHipError, match="multiple of 16"):
        bank.put_features(["a"], DenseFeatures({"black": torch.zeros(1, 14, 14, dtype=torch.uint8)}, m.feature_tag()))


def test_feature_tag_moves_with_the_module():
    from gim_amd.dkm import DKMv3
    m = DKMv3(None, 128, 160, upsample_preds=True, precision="bf16")
    t0 = m.feature_tag()
    m.load_state_dict(m.state_dict())
    t1 = m.feature_tag()
    m.float()
    t2 = m.feature_tag()
    m.precision = "fp16"
    t3 = m.feature_tag()
    m.upsample_preds = False
    assert len({t0, t1, t2, t3, m.feature_tag()}) == 5


# ------------------------------------------------------------------------------------------------ geometry table
@pytest.mark.parametrize("hw0,hw1", [((150, 224), (160, 180)), ((672, 896), (480, 640)), ((601, 333), (97, 1001))])
def test_geometry_row_against_get_padding_size(hw0, hw1):
    from gim_amd import _lib
    from gim_amd.adapters import get_padding_size, image_geometry, pair_geometry_row
    h, w = 672, 896
    im0, im1 = torch.zeros(1, 3, *hw0), torch.zeros(1, 3, *hw1)       # the MODEL's first / second image
    row = pair_geometry_row(image_geometry(im0, h, w), image_geometry(im1, h, w), (1.5, 2.0), (0.5, 3.0))
    assert len(row) == len(_lib.DensePairGeom._fields_) == 16
    f = dict(zip((n for n, _ in _lib.DensePairGeom._fields_), row))
    for side, im in (("0", im0), ("1", im1)):
        ow, oh, pl, pr, pt, pb = get_padding_size(im, h, w)
        padded = torch.nn.functional.pad(im, (pl, pr, pt, pb))
        assert (f["wp" + side], f["hp" + side]) == (padded.shape[3], padded.shape[2])
        assert (f["pl" + side], f["pt" + side], f["ow" + side], f["oh" + side]) == (pl, pt, im.shape[3], im.shape[2])
        assert abs(f["wp" + side] / f["hp" + side] - w / h) < 2e-2       # padded to the model's aspect ratio
    assert (f["sx0"], f["sy0"], f["sx1"], f["sy1"]) == (1.5, 2.0, 0.5, 3.0)
    assert all(isinstance(v, float) and v == float(torch.tensor(v, dtype=torch.float32)) for v in row)   # exact in the fp32 table
