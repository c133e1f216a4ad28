"""The gim_conv_args structs that gim_amd/ops.py hands to the library, without a GPU: `ops.lib` is replaced by a stand-in that copies every struct
it is handed, answers 0 for the launches and forwards the four predicates (gim_conv_ups_supported, gim_conv_ups_tiles_supported,
gim_conv2d_tiles_supported, gim_conv2d_big_tile) to the real library, which computes them on the host.  The public wrappers are then driven
with CPU tensors, and every recorded call -- entry, every non-pointer field, whether each pointer field is null, the capacity of a patch
list, a predicate's answer -- is compared with tests/golden/conv_args_parent.json.

The fixture was recorded by `record()` below on commit 0876606, the parent of the change that gave the four hand-filled structs of ops.py one
builder (`ops._conv_args`) and the dense launch one routing rule (`ops._dense_route`): the structs of that tree are the reference, so do not
regenerate the fixture with the code under test.  A last test needs no fixture: what `_dense_route` answers for a shape is what `conv2d`
then launches."""
import ctypes
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_args_parent.json")
B, H, W, CIN = 2, 16, 64, 128
ROWS = B * H * W
PREDICATES = ("gim_conv_ups_supported", "gim_conv_ups_tiles_supported", "gim_conv2d_tiles_supported", "gim_conv2d_big_tile")
KINDS = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _fields(a):
    """every non-pointer field of a gim_conv_args, and of every pointer field whether it is set"""
    return {name: bool(getattr(a, name)) if typ is ctypes.c_void_p else int(getattr(a, name)) for name, typ in type(a)._fields_}


class _Recorder:
    """stands in for `ops.lib`: see the module docstring"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        def call(*args):
            rec = {"entry": name}
            if args and hasattr(args[0], "_obj"):              # ctypes.byref(gim_conv_args)
                rec["args"] = _fields(args[0]._obj)
                if len(args) == 5:                              # the patch-list entries: (args, tiles, n_tiles, tiles_cap, stream)
                    rec["tiles_cap"] = int(args[3])
            if name in PREDICATES:
                rec["answer"] = int(getattr(self.real, name)(*args))
            self.calls.append(rec)
            return rec.get("answer", 0)
        return call


def _packs(dt):
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    d = ops.gim_dtype(torch.empty(0, dtype=dt))
    z = torch.zeros
    return {"lin": pack_conv(z(256, CIN), None, d, "cpu"), "c1": pack_conv(z(256, CIN, 1, 1), None, d, "cpu", bias=z(256)),
            "c3s2": pack_conv(z(256, CIN, 3, 3), None, d, "cpu", stride=2, pad=1, bias=z(256)),
            "c3": pack_conv(z(256, CIN, 3, 3), None, d, "cpu", stride=1, pad=1, bias=z(256)),
            "c3n196": pack_conv(z(196, CIN, 3, 3), None, d, "cpu", stride=1, pad=1)}


def record(mp, kind):
    """{case: [recorded call, ...]} of the cases below for one operand kind ("bf16", "fp16": every case; "fp32": the split-product ones).
    mp: a pytest MonkeyPatch; the stand-in stays in place until it is undone."""
    from gim_amd import ops
    from gim_amd._lib import ACT_GELU, ACT_LEAKY, ACT_RELU
    rec = _Recorder(ops.lib)
    mp.setattr(ops, "lib", rec)
    mp.setattr(ops, "_stream", lambda: None)
    mp.setattr(ops, "_req_cuda", lambda *ts: None)
    out = {}

    def case(name, fn, **switches):
        with mp.context() as m:
            for k, v in switches.items():
                m.setattr(ops, k, v)
            del rec.calls[:]
            try:
                ans = fn()
            except RuntimeError as e:                        # (a refused view: part of the record)
                ans = None
                rec.calls.append({"raised": type(e).__name__})
            out[name] = list(rec.calls)
        return ans

    def pred(name, fn, **switches):
        """a `*_supported` wrapper: the library's answers it asked for, then its own"""
        ans = case(name, fn, **switches)
        out[name].append({"wrapper": bool(ans)})

    health = torch.zeros(1, dtype=torch.int32)
    if kind == "fp32":
        P = _packs(torch.float32)
        x = torch.zeros(B, H, W, CIN)
        case("04 fp32 split16 with a health word", lambda: ops.conv2d(x, P["c1"], split16=True, health=health))
        case("05 fp32 split16 without lds_dma", lambda: ops.conv2d(x, P["c1"], split16=True, lds_dma=False, health=health))
        return out
    dt = KINDS[kind]
    P = _packs(dt)
    x = torch.zeros(B, H, W, CIN, dtype=dt)
    ups = torch.zeros(B, H // 2, W // 2, 256, dtype=dt)
    y = torch.zeros(B, H, W, 256, dtype=dt)
    tiles, n_tiles = torch.zeros(B * (H // 8) * (W // 32), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    case("01 linear on a strided row view", lambda: ops.linear(torch.zeros(ROWS, 160, dtype=dt)[:, :CIN], P["lin"], y.view(ROWS, 256), ACT_GELU,
                                                               act_cols=128))
    case("02 conv2d 1x1", lambda: ops.conv2d(x, P["c1"], ACT_RELU))
    case("03 conv2d 3x3 stride 2 with residual and health word",
         lambda: ops.conv2d(x, P["c3s2"], ACT_RELU, res=torch.zeros(B, H // 2, W // 2, 256, dtype=dt), health=health))
    case("06 conv2d ups fused", lambda: ops.conv2d(x, P["c1"], ups=ups), FORCE_BIG_TILE=True)
    case("07 conv2d ups in a second pass", lambda: ops.conv2d(x, P["c1"], ups=ups), FORCE_BIG_TILE=False)
    case("08 conv3x3_halo dense", lambda: ops.conv3x3_halo(x, P["c3"], y, ACT_LEAKY))
    case("09 conv3x3_halo with a tile list", lambda: ops.conv3x3_halo(x, P["c3"], y, ACT_LEAKY, tiles=tiles, n_tiles=n_tiles))
    case("10 conv2d routed to halo", lambda: ops.conv2d(x, P["c3"], ACT_LEAKY), HALO=True, HALO_MIN_TILES=0)
    # the halo rule's terms that no caller above leaves unmet: an output of another dtype takes the generic kernel, an x that is not rows of
    # cin_pad is refused before any launch (both packs and shapes are halo-eligible, as in case 10)
    case("16 conv2d with another out_dtype keeps off the halo kernel", lambda: ops.conv2d(x, P["c3"], ACT_LEAKY, out_dtype=torch.float32),
         HALO=True, HALO_MIN_TILES=0)
    case("17 conv2d refuses a non-contiguous x", lambda: ops.conv2d(torch.zeros(2 * B, H, W, CIN, dtype=dt)[::2], P["c3"], ACT_LEAKY),
         HALO=True, HALO_MIN_TILES=0)
    for big in (False, True):
        tag = " force_big_tile" if big else ""
        case("11 conv2d_tiles N=256" + tag, lambda: ops.conv2d_tiles(x, P["c3"], tiles, n_tiles, ACT_LEAKY), FORCE_BIG_TILE=big)
        case("12 conv2d_tiles N=196" + tag, lambda: ops.conv2d_tiles(x, P["c3n196"], tiles, n_tiles), FORCE_BIG_TILE=big)
        case("13 conv2d_ups_tiles" + tag, lambda: ops.conv2d_ups_tiles(x, P["c1"], ups, tiles, n_tiles), FORCE_BIG_TILE=big)
        case("14 conv2d_tiles H=12 runs dense" + tag,
             lambda: ops.conv2d_tiles(torch.zeros(B, 12, W, CIN, dtype=dt), P["c3"], tiles, n_tiles, ACT_LEAKY), FORCE_BIG_TILE=big)
        for dense_too in (False, True):
            tag2 = tag + (" dense_too" if dense_too else "")
            pred("15 conv_tiles_supported N=256" + tag2, lambda: ops.conv_tiles_supported(x.shape, P["c3"], dense_too=dense_too), FORCE_BIG_TILE=big)
            pred("15 conv_tiles_supported N=196" + tag2, lambda: ops.conv_tiles_supported(x, P["c3n196"], dense_too=dense_too), FORCE_BIG_TILE=big)
            pred("15 conv_tiles_supported where conv2d takes the halo kernel" + tag2,
                 lambda: ops.conv_tiles_supported(x.shape, P["c3"], dense_too=dense_too), FORCE_BIG_TILE=big, HALO=True, HALO_MIN_TILES=0)
            pred("15 conv_ups_tiles_supported" + tag2, lambda: ops.conv_ups_tiles_supported(x.shape, P["c1"], ups.shape, dense_too=dense_too),
                 FORCE_BIG_TILE=big)
            pred("15 conv_ups_tiles_supported with a residual" + tag2,
                 lambda: ops.conv_ups_tiles_supported(x, P["c1"], ups, res=y, dense_too=dense_too), FORCE_BIG_TILE=big)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _diff(g, w):
    return g.get("entry"), {k: (v, w.get("args", {}).get(k)) for k, v in g.get("args", {}).items() if v != w.get("args", {}).get(k)}


@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp32"])
def test_every_launch_struct_is_the_parents(kind, golden, monkeypatch):
    """per case, call for call and in the parent's order: the launches, the questions put to the library with their answers, and what the
    `*_supported` wrappers answered"""
    got = record(monkeypatch, kind)
    want = golden[kind]
    assert sorted(got) == sorted(want)
    for name in want:
        assert len(got[name]) == len(want[name]), (name, [c.get("entry") for c in got[name]], [c.get("entry") for c in want[name]])
        for g, w in zip(got[name], want[name]):
            assert g == w, (name,) + _diff(g, w)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_the_recorded_cases_say_what_their_names_say(kind, monkeypatch):
    """what the fixture cannot get wrong silently: the cases reach the entries and the field values they are there for"""
    got = record(monkeypatch, kind)
    launches = lambda name: [c for c in got[name] if c.get("entry") not in PREDICATES]   # noqa: E731
    assert got["02 conv2d 1x1"][-1]["args"]["Wo"] == ROWS and got["02 conv2d 1x1"][-1]["args"]["B"] == 1          # the flat geometry
    a3 = got["03 conv2d 3x3 stride 2 with residual and health word"][-1]["args"]
    assert a3["res"] and a3["health"] and a3["stride"] == 2
    assert [c["entry"] for c in launches("06 conv2d ups fused")] == ["gim_conv2d_bn_act"] and launches("06 conv2d ups fused")[0]["args"]["ups"]
    two = launches("07 conv2d ups in a second pass")
    assert [c["entry"] for c in two] == ["gim_conv2d_bn_act", "gim_upsample2x_add"] and not two[0]["args"]["ups"] and two[0]["args"]["ups_h"] == H // 2
    for name, entry in (("08 conv3x3_halo dense", "gim_conv2d_bn_act"), ("09 conv3x3_halo with a tile list", "gim_conv3x3_halo_tiles"),
                        ("10 conv2d routed to halo", "gim_conv2d_bn_act")):
        (c,) = launches(name)
        assert c["entry"] == entry and c["args"]["use_lds_dma"] == 2 and c["args"]["res_mod"] == CIN
    for big in ("", " force_big_tile"):
        assert [c["entry"] for c in launches("11 conv2d_tiles N=256" + big)] == ["gim_conv2d_tiles"]
        assert [c["entry"] for c in launches("12 conv2d_tiles N=196" + big)] == ["gim_conv2d_tiles"]
        assert [c["entry"] for c in launches("14 conv2d_tiles H=12 runs dense" + big)] == ["gim_conv2d_bn_act"]
    assert [c["entry"] for c in launches("13 conv2d_ups_tiles force_big_tile")] == ["gim_conv2d_ups_tiles"]
    got32 = record(monkeypatch, "fp32")
    a4, a5 = (got32[n][-1]["args"] for n in ("04 fp32 split16 with a health word", "05 fp32 split16 without lds_dma"))
    assert a4["split16"] == 1 and a4["health"] and a5["split16"] == 0 and not a5["health"] and a5["use_lds_dma"] == 0


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_the_route_rule_is_what_conv2d_launches(kind, big, monkeypatch):
    """for the shapes of cases 10, 11 and 13, `_dense_route`, asked with shapes alone as the `dense_too` predicates ask it, names the launch
    `conv2d` then makes: the entry, its use_lds_dma and whether `ups` is set"""
    from gim_amd import ops
    from gim_amd._lib import ACT_LEAKY, lib as real
    rec = _Recorder(real)
    monkeypatch.setattr(ops, "lib", rec)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_req_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", big)
    dt = KINDS[kind]
    P = _packs(dt)
    x = torch.zeros(B, H, W, CIN, dtype=dt)
    ups = torch.zeros(B, H // 2, W // 2, 256, dtype=dt)
    flat = (1, 1, ROWS, 1, ROWS)
    cases = (("c3", {"HALO_MIN_TILES": 0, "HALO": True}, (B, H, W, H, W), None, ACT_LEAKY),      # case 10
             ("c3", {}, (B, H, W, H, W), None, ACT_LEAKY), ("c3n196", {}, (B, H, W, H, W), None, ACT_LEAKY),   # cases 11, 12
             ("c1", {}, flat, ups, 0))                                                            # case 13
    seen = set()
    for name, switches, geom, u, act in cases:
        pk = P[name]
        with monkeypatch.context() as m:
            for k, v in switches.items():
                m.setattr(ops, k, v)
            a = ops._conv_args(pk, geom, pk.cin_pad, pk.n_store, act=act, ups=None if u is None else u.shape)
            route = ops._dense_route(pk, a, (B, H, W), tile=True)
            del rec.calls[:]
            ops.conv2d(x, pk, act, ups=u)
            sent = [c for c in rec.calls if c["entry"] not in PREDICATES]
        assert sent[0]["entry"] == "gim_conv2d_bn_act"
        s = sent[0]["args"]
        assert (route == "halo") == (s["use_lds_dma"] == 2)
        assert (route == "ups") == bool(s["ups"]) and (route == "ups" or u is None) == (len(sent) == 1)
        if route != "halo":
            assert s["use_lds_dma"] == (3 if big else 1)
            b = ops._conv_args(pk, geom, pk.cin_pad, pk.n_store, act=act)
            assert (route == "big") == bool(not s["ups"] and real.gim_conv2d_big_tile(ctypes.byref(b)))
            assert {k: v for k, v in _fields(a).items() if k not in ("x", "y", "ups")} == {k: v for k, v in s.items() if k not in ("x", "y", "ups")}
        seen.add(route)
    assert seen == ({"halo", "ups", "big"} if big else {"halo", "other"})
