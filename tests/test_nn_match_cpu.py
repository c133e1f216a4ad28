"""CPU tests of the root_sift descriptor matcher: the oracle itself (tests/nn_match_oracle.py), the condition under which the GPU parity
tests speak (at most 2 % undecidable rows on the chosen seeds, shown from the fp32 and fp64 oracles alone), the exported entry point,
the missing-detector error and the no-(n0 x n1)-buffer guarantee as far as it shows without a device.

The tests of the oracle and of the seeds (test_seeds_*, test_oracle_on_a_hand_written_case) read tests/nn_match_oracle.py only: they
state the condition of the GPU parity bar and do not depend on the engine, so they pass with or without it.  The others need the
new export, wrapper, module and plugin."""
import ctypes
import importlib.util

import pytest
import torch

import nn_match_oracle as O


@pytest.mark.parametrize("rootsift", [True, False], ids=["rootsift", "plain"])
@pytest.mark.parametrize("shape", O.CASES, ids=str)
def test_seeds_keep_the_undecidable_cap(shape, rootsift):
    """the inputs, not the kernel, keep the cap: undecidable rows <= 2 %, and the fp32 restatement of the reference already agrees with
    the fp64 one on every decidable row (index exact, score within EPS)"""
    k = O.case(*shape, rootsift)
    f = k["f64"]
    d = f["decidable"]
    und = 1.0 - d.float().mean().item()
    print(f"{shape} rootsift={rootsift}: undecidable {und:.4f}, valid {(f['match0'] >= 0).float().mean().item():.3f}")
    assert und <= O.UNDECIDABLE_CAP
    assert torch.equal(k["match32"][d], f["match0"][d])
    assert ((k["score32"].double() - f["score0"]).abs()[d] <= O.EPS).all()
    if shape[0] >= 5:
        valid = (f["match0"] >= 0).float().mean().item()
        assert valid >= 0.2 and 1.0 - valid >= 0.2
    # at SIFT's width and above the accepted matches are the planted columns (16-d descriptors also pair up by chance)
    hit = f["match0"] >= 0
    if shape[2] >= 128:
        assert (f["match0"][hit] == k["truth"][hit]).float().mean().item() > 0.9


@pytest.mark.parametrize("shape", [(257, 130, 128), (1000, 777, 128), (300, 300, 16)], ids=str)
def test_seeds_keep_the_cap_without_ratio_test(shape):
    for ratio in (0.0, -1.0):
        k = O.case(*shape, True, ratio)
        d = k["f64"]["decidable"]
        assert 1.0 - d.float().mean().item() <= O.UNDECIDABLE_CAP
        assert torch.equal(k["match32"][d], k["f64"]["match0"][d])


def test_oracle_on_a_hand_written_case():
    """4 x 3 with unit vectors whose entries are 0, +-.5 or 1 (D = 16, zeros elsewhere): every product is exact in fp32 and fp64.
        e0 = (1,0,0,0)  e1 = (0,1,0,0)  h = (.5,.5,.5,.5)  g = (.5,.5,-.5,-.5)  k = (.5,-.5,.5,-.5)
                 col0 = e0   col1 = h   col2 = g
    row0 = e0       1          .5         .5      best col0, holds the column, ratio sqrt(0 / 1) = 0            -> 0
    row1 = e1       0          .5         .5      two bit-equal maxima: ratio sqrt(1 / 1) = 1                   -> -1
    row2 = h        .5         1          0       best col1, holds the column, ratio 0                          -> 1
    row3 = k        .5         0          0       best col0, ratio sqrt(1 / 2) = .707 passes, but row0 holds the column -> -1"""
    def v(*x):
        r = torch.zeros(16, dtype=torch.float64)
        r[:4] = torch.tensor(x, dtype=torch.float64)
        return r
    e0, e1, h, g, k = v(1, 0, 0, 0), v(0, 1, 0, 0), v(.5, .5, .5, .5), v(.5, .5, -.5, -.5), v(.5, -.5, .5, -.5)
    desc0, desc1 = torch.stack([e0, e1, h, k]), torch.stack([e0, h, g])
    for fp32 in (True, False):
        m, s, sim = O.nn_match(desc0, desc1, rootsift=False, ratio=0.8, fp32=fp32)
        assert sim.tolist() == [[1, .5, .5], [0, .5, .5], [.5, 1, 0], [.5, 0, 0]]
        assert m.tolist() == [0, -1, 1, -1]
        assert s.tolist() == [1, .5, 1, .5]
        # without row0, row3 ties row2 for column 0 and is mutual: accepted at .8 (ratio .707), rejected at .7
        assert O.nn_match(desc0[1:], desc1, False, 0.8, fp32=fp32)[0].tolist() == [-1, 1, 0]
        assert O.nn_match(desc0[1:], desc1, False, 0.7, fp32=fp32)[0].tolist() == [-1, 1, -1]
        # ratio test off: plain mutual nearest neighbour.  Row1 ties columns 1 and 2 bit-exactly and holds column 2 only: the reference's
        # mask.max(1) picks the mutual one (2); the kernel's tie rule reports the lowest (1), which row2 holds -> -1 there.  This is the one
        # documented difference (nn_match.hip header); a decidable row has no tie
        assert O.nn_match(desc0[1:], desc1, False, 0.0, fp32=fp32)[0].tolist() == [2, 1, 0]
        assert not O.margins_f64(desc0[1:], desc1, False, 0.0)["decidable"][0]
        # n1 == 1 has no second neighbour: empty with the ratio test, mutual nearest neighbour without
        assert O.nn_match(desc0, desc1[:1], False, 0.8, fp32=fp32)[0].tolist() == [-1, -1, -1, -1]
        assert O.nn_match(desc0, desc1[:1], False, 0.0, fp32=fp32)[0].tolist() == [0, -1, -1, -1]
    f = O.margins_f64(desc0, desc1, rootsift=False)
    assert f["row_margin"].tolist() == [.5, 0, .5, .5]
    assert [f["col_margin"][i].item() for i in (0, 2, 3)] == [.5, .5, .5]       # row1's arg-max is one of two tied columns
    assert torch.allclose(f["ratio_margin"], torch.tensor([.8, .2, .8, .8 - 0.5 ** 0.5], dtype=torch.float64), atol=1e-12)
    assert f["decidable"].tolist() == [True, False, True, True]
    # RootSIFT: (7,0,0,0) -> e0, (3,3,3,3) -> h, (0,5,0,0) -> e1 exactly; columns h, e0
    r0 = torch.stack([v(7, 0, 0, 0), v(3, 3, 3, 3), v(0, 5, 0, 0)])
    r1 = torch.stack([v(2, 2, 2, 2), v(9, 0, 0, 0)])
    for fp32 in (True, False):
        m, s, sim = O.nn_match(r0, r1, rootsift=True, ratio=0.8, fp32=fp32)
        assert sim.tolist() == [[.5, 1], [1, .5], [.5, 0]] and m.tolist() == [1, 0, -1]


def test_entry_point_is_exported_and_takes_no_matrix_sized_workspace():
    from gim_amd import _lib
    assert hasattr(_lib.lib, "gim_nn_match") and hasattr(_lib.lib, "gim_nn_match_ws_bytes")
    assert _lib.lib.gim_version() == _lib.ABI_VERSION == 115          # an added export: it moved no ABI revision
    res, args = _lib.PROTOTYPES["gim_nn_match"]
    assert args.count(ctypes.c_void_p) == 7                          # desc0, desc1, match0, score0, count, ws, stream: one workspace
    n, D = 4096, 128
    for rootsift in (0, 1):
        ws = _lib.lib.gim_nn_match_ws_bytes(n, n, D, rootsift)
        # O((n0 + n1) D) bytes: the normalised copies (rootsift), 16 column splits x 3 row statistics, the column maxima, alignment
        assert 0 < ws <= 4 * (rootsift * 2 * n * D + 3 * 16 * n + n) + 8 * 256
        assert ws < n * n                                            # bytes, against the ELEMENTS of the similarity matrix
    # linear in n: doubling both sides doubles the workspace (up to alignment)
    a, b = _lib.lib.gim_nn_match_ws_bytes(4096, 4096, 128, 1), _lib.lib.gim_nn_match_ws_bytes(8192, 8192, 128, 1)
    assert abs(b - 2 * a) <= 4096
    # invalid descriptor widths are refused by the library before any launch (no device needed to see it)
    for bad in (8, 24, 272):
        one = ctypes.c_int32(0)
        rc = _lib.lib.gim_nn_match(None, None, 4, 4, bad, 1, 0.8, None, None, ctypes.addressof(one), None, None)
        assert rc == -1 and b"D=" in _lib.lib.gim_last_error()


def test_wrapper_allocates_nothing_of_matrix_size(monkeypatch):
    """ops.nn_match at n0 = n1 = 4096: every torch.empty / torch.zeros request is below n0 * n1 elements (the launch itself is stubbed:
    there is no device here)"""
    from gim_amd import ops
    n, D = 4096, 128
    requests = []

    def spy(fn):
        def f(*size, **kw):
            shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
            numel = 1
            for x in shape:
                numel *= int(x)
            requests.append(numel)
            kw["device"] = "cpu"
            return fn(*size, **kw)
        return f

    class Lib:
        gim_nn_match_ws_bytes = staticmethod(ops.lib.gim_nn_match_ws_bytes)

        @staticmethod
        def gim_nn_match(*a):
            return 0

    monkeypatch.setattr(ops.torch, "empty", spy(torch.empty))
    monkeypatch.setattr(ops.torch, "zeros", spy(torch.zeros))
    monkeypatch.setattr(ops, "lib", Lib)
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    desc = torch.ones(n, D)
    m, s = ops.nn_match(desc, desc, rootsift=True)
    assert m.shape == s.shape == (n,)
    assert requests and max(requests) < n * n
    assert sum(requests) <= 4 * (2 * n * D + 3 * 16 * n + n) + 8 * 256 + 2 * n + 1      # workspace bytes + match0 + score0 + count


def test_inference_without_cv2_raises_the_documented_error():
    if importlib.util.find_spec("cv2") is not None:
        pytest.skip("cv2 is installed: the detector exists")
    from gim_amd._lib import GimHipError
    from gim_amd.nn_match import RootSiftMatcher
    data = {"color0": torch.zeros(1, 3, 16, 16), "color1": torch.zeros(1, 3, 16, 16), "image0": torch.zeros(1, 1, 16, 16),
            "image1": torch.zeros(1, 1, 16, 16)}
    with pytest.raises(GimHipError, match="SIFT detector"):
        RootSiftMatcher().inference(data)
    assert "mkpts0_f" not in data
    from gim_amd import demo
    assert "root_sift" in demo.MODELS
    with pytest.raises(GimHipError, match="SIFT detector"):
        demo.build("root_sift")
    with pytest.raises(GimHipError, match="SIFT detector"):
        demo.main(["--model", "root_sift"])


def test_hloc_plugin_is_found_and_refuses_one_way_matching():
    from hloc.utils.base_model import dynamic_load

    import gim_amd.hloc_matchers as matchers
    Model = dynamic_load(matchers, "nn_ratio_hip")
    assert Model.required_inputs == ["descriptors0", "descriptors1"]
    assert set(Model.default_conf) >= {"ratio_threshold", "do_mutual_check"}
    with pytest.raises(NotImplementedError):
        Model({"do_mutual_check": False})
    assert Model({}).ratio == pytest.approx(0.8)
