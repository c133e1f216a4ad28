"""Host-side plumbing of gim_loftr that needs no device: the launch scope that arms the fp32 mode's split products per module (never through
`ops.FP32_SPLIT`), the one decision between a graph replay and eager launches, and the conversion / checks of the per-pair inputs."""
import warnings

import pytest
import torch

from tools import synth_loftr as S

CPU = torch.device("cpu")


def _model(precision="fp32", **cfg):
    return S.synthetic_model(precision, **cfg)[0]


# ---- launch scope ------------------------------------------------------------------------------------------------------------------
def test_scope_arms_true_for_fp32_split_only():
    from gim_amd import ops
    glob = ops.FP32_SPLIT
    for precision, cfg, armed in (("fp32", {}, True), ("fp32", {"fp32_split": False}, None), ("fp16", {}, None), ("bf16", {}, None)):
        m = _model(precision, **cfg)
        assert m._split16 is None
        with m._launch_scope(CPU):
            assert m._split16 is armed, (precision, cfg)
            assert ops.FP32_SPLIT is glob
        assert m._split16 is None and ops.FP32_SPLIT is glob


def test_nested_scope_after_the_guard_turned_split_off():
    from gim_amd import ops
    glob = ops.FP32_SPLIT
    m = _model("fp32")
    with m._launch_scope(CPU):
        assert m._split16 is True
        m.fp32_split = False   # what _range_guard does before the batch runs again
        with m._launch_scope(CPU):
            assert m._split16 is None and ops.FP32_SPLIT is glob
        assert m._split16 is True   # the outer scope's own value is back
    assert m._split16 is None and ops.FP32_SPLIT is glob


def test_scope_restores_when_the_body_raises():
    from gim_amd import ops
    glob = ops.FP32_SPLIT
    m = _model("fp32")
    with pytest.raises(KeyError):
        with m._launch_scope(CPU):
            assert m._split16 is True
            raise KeyError("body")
    assert m._split16 is None and ops.FP32_SPLIT is glob
    with m._launch_scope(CPU):
        with pytest.raises(ZeroDivisionError):
            with m._launch_scope(CPU):
                1 / 0
        assert m._split16 is True
    assert m._split16 is None


def test_scope_packs_first_and_dead_channels_arm_none():
    """the `_dead_channels` recipe of tests/test_split16_guard_cpu.py: the pack-time weight check turns fp32_split off before the scope arms"""
    from gim_amd import ops
    glob = ops.FP32_SPLIT
    m, sd = S.synthetic_model("fp32")
    sd = {k: v.clone() for k, v in sd.items()}
    sd["backbone.encode.layer2.0.bn2.running_var"][:3] = 0.0
    m.load_state_dict(sd)
    assert m.fp32_split and m._packed is None
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with m._launch_scope(CPU):
            assert m._split16 is None and m._packed is not None
            assert ops.FP32_SPLIT is glob
    assert m.split_overflowed and not m.fp32_split and m._split16 is None
    assert any("exact fp32 products" in str(w.message) for w in rec)
    assert ops.FP32_SPLIT is glob


def test_health_word_follows_the_armed_value_not_the_global_alone(monkeypatch):
    from gim_amd import ops
    word = object()
    m = _model("fp32")
    monkeypatch.setattr(ops, "FP32_SPLIT", False)
    assert m._health_word(word) is None            # outside an entry point: the default
    with m._launch_scope(CPU):
        assert m._health_word(word) is word        # armed: the split launches report into the word
    monkeypatch.setattr(ops, "FP32_SPLIT", True)
    assert m._health_word(word) is word            # default on (fp32_split_all): as before
    assert _model("fp16")._health_word(word) is word and _model("bf16")._health_word(word) is None


# ---- graphed or eager --------------------------------------------------------------------------------------------------------------
class _Stubs:
    def __init__(self, graphed_raises=None):
        self.calls, self.graphed_raises = [], graphed_raises

    def graphed(self):
        self.calls.append("graphed")
        if self.graphed_raises is not None:
            raise self.graphed_raises
        return "g"

    def eager(self):
        self.calls.append("eager")
        return "e"


def test_first_call_is_eager_and_counted_second_is_graphed():
    m, s = _model("fp16"), _Stubs()
    assert m._run_stage("k", s.graphed, s.eager) == ("e", False)
    assert s.calls == ["eager"] and m._seen["k"] == 1
    assert m._run_stage("k", s.graphed, s.eager) == ("g", True)
    assert s.calls == ["eager", "graphed"] and m._seen["k"] == 1
    # another key starts over; graph = False and the debug dumps never count
    assert m._run_stage("k2", s.graphed, s.eager) == ("e", False) and m._seen["k2"] == 1
    m.use_graph = False
    assert m._run_stage("k", s.graphed, s.eager) == ("e", False) and m._seen["k"] == 1
    m.use_graph, m.debug = True, {}
    assert m._run_stage("k", s.graphed, s.eager) == ("e", False) and m._seen["k"] == 1


def test_failed_capture_warns_once_and_goes_eager():
    m = _model("fp16")
    s = _Stubs(RuntimeError("operation not permitted when stream is capturing"))
    m._seen["k"] = 1
    m._graphs["other"] = ("graph", [], {})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert m._run_stage("k", s.graphed, s.eager) == ("e", False)
        assert m._run_stage("k", s.graphed, s.eager) == ("e", False)   # eager from now on, silently
    msgs = [str(w.message) for w in rec]
    assert len(msgs) == 1 and "HIP graph capture failed" in msgs[0] and "using eager kernel launches" in msgs[0]
    assert s.calls == ["graphed", "eager", "eager"]
    assert m.use_graph is False and len(m._graphs) == 0 and m._seen["k"] == 1   # eager calls are no longer counted


def test_other_errors_propagate():
    m = _model("fp16")
    m._seen["k"] = 1
    s = _Stubs(RuntimeError("other"))
    with pytest.raises(RuntimeError, match="other"):
        m._run_stage("k", s.graphed, s.eager)
    assert s.calls == ["graphed"] and m.use_graph
    # a capture error for a key that is already cached is no failed capture (the graph exists: a replay went wrong)
    s = _Stubs(RuntimeError("operation not permitted when stream is capturing"))
    m._graphs["k"] = ("graph", [], {})
    with pytest.raises(RuntimeError, match="capturing"):
        m._run_stage("k", s.graphed, s.eager)
    assert s.calls == ["graphed"] and m.use_graph and "k" in m._graphs
    # ... and nothing but RuntimeError is looked at
    s = _Stubs(ValueError("capturing"))
    with pytest.raises(ValueError):
        m._run_stage("k", s.graphed, s.eager)


def test_seen_is_trimmed_to_64_keys():
    m, s = _model("fp16"), _Stubs()
    for k in range(100):
        m._run_stage(("shape", k), s.graphed, s.eager)
        assert len(m._seen) <= 64
    assert len(m._seen) == 64 and ("shape", 99) in m._seen and ("shape", 35) not in m._seen and s.calls == ["eager"] * 100


# ---- per-pair inputs ---------------------------------------------------------------------------------------------------------------
def test_pair_inputs_converts_and_checks():
    from gim_amd.loftr import LoFTR
    assert LoFTR._pair_inputs({}, CPU, (2, 8, 12), (2, 12, 8)) == (None, None, None, None)
    data = {"scale0": torch.ones(2, 2, dtype=torch.float64), "scale1": torch.ones(2, 2, dtype=torch.float64) * 2,
            "mask0": torch.tensor([[[True, False]]] * 2), "mask1": torch.full((2, 1, 3), 7)}
    s0, s1, m0, m1 = LoFTR._pair_inputs(data, CPU, (2, 1, 2), (2, 1, 3), per="P", rows=2)
    assert s0.dtype == s1.dtype == torch.float32 and s1[0, 0] == 2 and s0.is_contiguous()
    assert m0.dtype == m1.dtype == torch.uint8 and m0.tolist() == [[[1, 0]]] * 2 and m1.unique().tolist() == [1]
    # forward's wording, match_features' wording
    with pytest.raises(ValueError, match=r"mask0/mask1 must be \[N, H/8, W/8\]: got \(2, 1, 2\), \(2, 1, 3\)"):
        LoFTR._pair_inputs(data, CPU, (2, 1, 2), (2, 1, 2))
    with pytest.raises(ValueError, match=r"mask0/mask1 must be \[P, H/8, W/8\]: got \(2, 1, 2\), \(2, 1, 3\)"):
        LoFTR._pair_inputs(data, CPU, (2, 1, 3), (2, 1, 3), per="P", rows=2)
    # one scale row per pair: match_features only
    with pytest.raises(ValueError, match=r"scale0/scale1 must have one row per pair \(3\)"):
        LoFTR._pair_inputs(data, CPU, (2, 1, 2), (2, 1, 3), per="P", rows=3)
    assert LoFTR._pair_inputs({"scale0": data["scale0"], "scale1": data["scale1"]}, CPU, (3, 1, 2), (3, 1, 3))[0].shape == (2, 2)
