"""Video pseudo-labels without a GPU: video_labels.link_tables (the numpy restatement of csrc/label_link.hip) against the dict / set
formulation of tests/label_link_oracle.py, propagate against the oracle's recursion on the synthetic video of
tests/label_link_cases.py, LabelStore against a directory in the reference's naming, label_pack_np against the numpy expressions of
the labeller's tail, the new exports against the header, the kernels' resources, and tools/label_key_host_check.cpp (the header on
the CPU) against numpy.  Every comparison is exact: indices are integers and coordinates are copied or rounded in a fixed way."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import host_check
import label_link_cases as C
import label_link_oracle as O
from gim_amd import video_labels as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_link(case):
    out, ij, dropped = V.link_tables(case.lab0, case.lab1, case.width, case.height)
    want = O.link_ij(case.lab0, case.lab1, case.width)
    assert dropped == (0, 0), (case.name, dropped)
    assert np.array_equal(ij.T, want), case.name
    assert _same_bits(out, np.concatenate([case.lab0[want[0], :2], case.lab1[want[1], 2:]], 1)), case.name
    return len(out)


@pytest.mark.parametrize("case", C.link_cases(), ids=lambda c: c.name)
def test_link_tables_equal_the_dict_formula(case):
    n = _check_link(case)
    if case.name in ("random-1000x900-96", "random-3000x2500-1920", "half-integer", "one-key", "alias"):
        assert n > 0
    if case.name == "no-shared" or "-0x" in case.name or case.name.endswith("x0-96"):
        assert n == 0


def test_half_integers_round_to_even():
    assert V.label_keys(np.float32([0.5, 1.5, 2.5, -0.5]), np.float32([0, 0, 0, 0]), 96).tolist() == [0.0, 2.0, 2.0, -0.0]
    c = C.half_integer_case()
    _, ij, _ = V.link_tables(c.lab0, c.lab1, c.width, c.height)
    # lab0's x = k + 0.5 lands on the even neighbour: only even pixels of the y = 2 row are hit (2.5 -> 2), by the last of their rows
    keys = V.label_keys(c.lab0[:, 2], c.lab0[:, 3], c.width)
    assert set(np.unique(keys[ij[:, 0]]) % 2) == {0.0}
    assert len(ij) and all(i == np.flatnonzero(keys == keys[i]).max() for i in ij[:, 0])


def test_the_last_row_of_a_key_wins_on_both_sides():
    c = C.one_key_case()
    _, ij, _ = V.link_tables(c.lab0, c.lab1, c.width, c.height)
    k0, k1 = V.label_keys(c.lab0[:, 2], c.lab0[:, 3], c.width), V.label_keys(c.lab1[:, 0], c.lab1[:, 1], c.width)
    key = np.float32(17 + 9 * c.width)
    assert (k0 == key).sum() >= 300 and (k1 == key).sum() >= 300
    hit = ij[k0[ij[:, 0]] == key]
    assert hit.tolist() == [[np.flatnonzero(k0 == key).max(), np.flatnonzero(k1 == key).max()]]


def test_the_alias_of_the_reference_is_kept():
    c = C.alias_case()
    _, ij, dropped = V.link_tables(c.lab0, c.lab1, c.width, c.height)
    assert dropped == (0, 0) and ij.tolist() == [[0, 0], [1, 1], [2, 2]]


@pytest.mark.parametrize("extra", [-1, 0])
def test_min_final_matches(extra):
    c = C.random_case(257, 255)
    n = len(O.link_ij(c.lab0, c.lab1, c.width)[0])
    assert n > 8
    got = V.link(c.lab0, c.lab1, c.width, c.height, n - extra)          # extra = -1: one more than there are
    want = O.link(c.lab0, c.lab1, c.width, n - extra)
    if extra < 0:
        assert got is None and want is None
    else:
        assert _same_bits(got, want) and len(got) == n


def test_unusable_keys_are_dropped_and_counted():
    c, ok0, ok1 = C.dropped_case()
    out, ij, dropped = V.link_tables(c.lab0, c.lab1, c.width, c.height)
    assert dropped == (int((~ok0).sum()), int((~ok1).sum())) == (9, 4)
    i, j = O.link_ij(c.lab0[ok0], c.lab1[ok1], c.width)                   # the oracle on the filtered input, in the full rows' numbering
    want = np.stack([np.flatnonzero(ok0)[i], np.flatnonzero(ok1)[j]], 1)
    assert len(want) > 50 and np.array_equal(ij, want)
    assert _same_bits(out, np.concatenate([c.lab0[want[:, 0], :2], c.lab1[want[:, 1], 2:]], 1))


def test_frame_sizes_are_checked():
    c = C.alias_case()
    for w, h in ((0, 10), (10, 0), (-3, 5), (4096, 4096), (1 << 24, 1)):
        with pytest.raises(ValueError):
            V.link_tables(c.lab0, c.lab1, w, h)
    V.link_tables(c.lab0[:0], c.lab1[:0], 4096, 4095)                      # 2^24 exactly is the largest key range


# ---- propagate ---------------------------------------------------------------------------------------------------------------------
def test_propagate_equals_the_sequential_oracle(monkeypatch):
    w, h = C.SMALL
    store = C.video_store()
    walk = O.Walk(C.video(), w, C.VIDEO_MIN_FINAL)
    failed = []
    real_link = V.link

    def counting_link(*a, **k):
        r = real_link(*a, **k)
        failed.append(r is None)
        return r

    monkeypatch.setattr(V, "link", counting_link)
    some = 0
    for idx0, idx1, skips in C.PROPAGATE_REQUESTS:
        got = V.propagate(store, idx0, idx1, skips, width=w, height=h, min_final_matches=C.VIDEO_MIN_FINAL)
        want = walk.propagate(idx0, idx1, skips)
        assert got[1:] == want[1:], (idx0, idx1, skips, got[1:], want[1:])
        assert (got[0] is None) == (want[0] is None)
        if want[0] is not None:
            some += 1
            assert _same_bits(got[0], want[0]) and len(got[0]) >= 1
    # both branches were taken, by the oracle and by the code under test
    assert "fallback" in walk.trace and "none" in walk.trace
    assert any(failed) and not all(failed) and some >= 6
    # the hop 8 -> 12 cannot be linked; the fall-back shortens it to 8 -> 11, 8 -> 10 and 8 -> 9, where the first 60 tracks still live
    assert walk.propagate(0, 12, C.VIDEO_SKIPS)[1:] == (0, 9)
    assert walk.propagate(5, 6, [1]) == (None, None, None)                 # the missing pair
    assert V.propagate(store, 5, 6, [1], width=w, height=h, min_final_matches=C.VIDEO_MIN_FINAL) == (None, None, None)


def test_label_store_reads_the_reference_layout(tmp_path):
    labels = C.video()
    dirs = {}
    for skip in (1, 2):
        for s in range(2 if skip == 1 else 1):
            d = tmp_path / f"src{s} SP{skip}"
            d.mkdir()
            pairs = sorted(labels[skip])
            for pair in pairs:
                np.save(str(d / "{}.npy".format(str(np.array(pair)))), labels[skip][pair][s].astype(np.float64 if s else np.float32))
            np.save(str(d / "idxs.npy"), np.array(pairs))
            np.save(str(d / "nums.npy"), np.array([len(labels[skip][p][s]) for p in pairs]))
            dirs.setdefault(skip, []).append(str(d))
    store = V.LabelStore.from_dirs(dirs)
    walk = O.Walk(labels, C.SMALL[0], C.VIDEO_MIN_FINAL)
    for skip in (1, 2):
        assert store.pairs(skip) == sorted(labels[skip])
        for pair in labels[skip]:
            got = store.dump(skip, pair)
            assert got.dtype == np.float32 and _same_bits(got, walk.dump(skip, pair))
    assert len(store.dump(1, C.VIDEO_MISSING)) == 0 and len(store.dump(4, (0, 4))) == 0
    with pytest.raises(FileNotFoundError):
        V.LabelStore.from_dirs({1: [str(tmp_path)]})


# ---- label_pack ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257, 1000])
def test_label_pack_np_equals_the_labellers_expressions(n):
    k0, k1, keep = C.pack_case(n)
    moved = ~(np.abs(k0 - k1) < 1).min(axis=1) if n else np.zeros(0, dtype=bool)     # video_preprocessor.py:516
    if n > 2:
        assert moved[n // 2] and not moved.all() and moved[0]                        # the NaN row; static rows; exactly one pixel
    s0, o0, s1, o1 = (np.array([C.AFFINE[i:i + 2]]) for i in (0, 2, 4, 6))
    inl = keep.astype(bool)
    for thr, m in ((1.0, moved), (0.0, np.ones(n, dtype=bool))):
        assert _same_bits(V.label_pack_np(k0, k1, moved_thr=thr), np.concatenate([k0[m], k1[m]], 1))
        # line 549: fp32 points times an fp64 scale, plus an fp64 offset, times vratio; line 555: the cast
        want = np.concatenate([(k0[m & inl] * s0 + o0) * C.VRATIO, (k1[m & inl] * s1 + o1) * C.VRATIO], axis=1).astype(np.float32)
        assert _same_bits(V.label_pack_np(k0, k1, keep=keep, moved_thr=thr, affine=C.AFFINE, vratio=C.VRATIO), want)
        # line 552: fp32 points times the Python float
        want = np.concatenate([k0[m & inl] * C.VRATIO, k1[m & inl] * C.VRATIO], axis=1).astype(np.float32)
        assert want.dtype == np.float32 and _same_bits(V.label_pack_np(k0, k1, keep=keep, moved_thr=thr, vratio=C.VRATIO), want)


# ---- the library ------------------------------------------------------------------------------------------------------------------
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def test_exports_follow_the_header_within_revision_115():
    from gim_amd import _lib
    for name, n_args in (("gim_label_link_ws_bytes", 2), ("gim_label_link", 16), ("gim_label_pack", 10)):
        res, args = _header_prototype(name)
        fn = getattr(_lib.lib, name)
        assert (res, args) == _lib.PROTOTYPES[name] and len(args) == n_args, name
        assert fn.restype is res and list(fn.argtypes) == args and args[-1] is (ctypes.c_void_p if n_args > 2 else ctypes.c_int)
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    lib = _lib.lib
    assert lib.gim_label_link_ws_bytes(1, 1920 * 1081 + 1) == 2 * 4 * (1920 * 1081 + 1)
    assert lib.gim_label_link_ws_bytes(5, 0) == 0 and lib.gim_label_link_ws_bytes(-1, 8) < 0 and lib.gim_label_link_ws_bytes(1, -8) < 0
    # refused before anything is launched (no device is needed to be refused)
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    wh = lambda w, h: (ctypes.c_int32 * 2)(w, h)   # noqa: E731
    link = lambda B, n0, n1, size, mk=1 << 25, lab0=p, ij=p, offs=None, whd=None: lib.gim_label_link(   # noqa: E731
        lab0, offs, n0, p, offs, n1, size, whd, B, mk, p, p, ij, p, p, None)
    assert link(0, 0, 0, None) == 0                                                       # no link: nothing is touched
    assert link(-1, 0, 0, wh(96, 54)) != 0
    assert link(1, -1, 0, wh(96, 54)) != 0 and b"negative" in lib.gim_last_error()
    assert link(1, 0, -5, wh(96, 54)) != 0 and b"negative" in lib.gim_last_error()
    assert link(1, 4, 4, wh(0, 54)) != 0 and link(1, 4, 4, wh(96, 0)) != 0 and link(1, 4, 4, wh(96, -2)) != 0
    assert link(1, 4, 4, wh(4096, 4096)) != 0 and b"2^24" in lib.gim_last_error()
    assert link(1, 4, 4, wh(96, 54), mk=96 * 55) != 0 and b"max_keys" in lib.gim_last_error()
    assert link(2, 4, 4, (ctypes.c_int32 * 4)(96, 54, 96, 54)) != 0 and b"offsets" in lib.gim_last_error()
    assert link(1, 4, 4, wh(96, 54), lab0=off(8)) != 0 and b"aligned" in lib.gim_last_error()
    assert link(1, 4, 4, wh(96, 54), ij=off(4)) != 0 and b"misaligned" in lib.gim_last_error()
    assert link(1, 4, 4, wh(96, 54), lab0=None) != 0 and b"NULL" in lib.gim_last_error()
    pack = lambda n, k0=p, out=p, count=p: lib.gim_label_pack(k0, p, None, n, 1.0, None, 1.0, out, count, None)   # noqa: E731
    assert pack(-1) != 0
    assert pack(4, k0=None) != 0 and b"NULL" in lib.gim_last_error()
    assert pack(0, count=None) != 0 and b"NULL" in lib.gim_last_error()
    assert pack(4, k0=off(4)) != 0 and pack(4, out=off(8)) != 0 and b"aligned" in lib.gim_last_error()


def test_wrappers_refuse_bad_arguments_before_a_launch(monkeypatch):
    import torch
    from gim_amd import _lib, ops

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(ops, "lib", NoLaunch())
    lab = torch.zeros(4, 4)
    with pytest.raises(_lib.GimHipError):
        ops.label_link(lab, lab, 96, 54)                                   # host tensors
    with pytest.raises(_lib.GimHipError):
        ops.label_pack(lab[:, :2], lab[:, :2])
    with pytest.raises(ValueError):
        ops._label_sizes(0, 54, 1)
    with pytest.raises(ValueError):
        ops._label_sizes(4096, 4096, 1)
    with pytest.raises(ValueError):
        ops._label_sizes([96, 96], [54, 54], 3)
    assert ops._label_sizes(96, 54, 3).tolist() == [[96, 54]] * 3 and ops.label_link_max_keys([96, 1920], [54, 1080]) == 1920 * 1081 + 1
    with pytest.raises(ValueError):
        V.link(lab.numpy(), lab.numpy(), 0, 54, 1, device="cuda:0")
    with pytest.raises(ValueError):
        V.label_pair({"scores": None}, device="cuda:0")


def test_kernels_target_gfx950_without_scratch():
    """label_link_rows_kernel 12, label_link_compact_kernel 59, label_pack_kernel 56-59 VGPRs on the build that wrote this test;
    the bar is no scratch and no spilled register"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr._kernels()
    for key in ("label_link_rows_kernel<false>", "label_link_rows_kernel<true>", "label_link_compact_kernel(", "label_pack_kernel<false>",
                "label_pack_kernel<true>"):
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert hit, f"{key} not found in the library"
        for n, (regs, scratch, spills) in hit:
            print(f"{n[:40]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
            assert scratch == 0 and spills == 0, (n, regs, scratch, spills)


def _f32(h):
    return np.array([int(h, 16)], dtype=np.uint32).view(np.float32)[0]


def _f64(h):
    return np.array([int(h, 16)], dtype=np.uint64).view(np.float64)[0]


def test_host_check_agrees_with_numpy(tmp_path):
    """tools/label_key_host_check.cpp is plain C++ over csrc/label_key.h; built with the host compiler, every key, slot, watermark
    test and rescaled coordinate it prints equals the numpy restatement bit for bit (a NaN as a NaN).  The sanitizer run of the same
    program is a development step, recorded in profiles/label_link.txt."""
    r = host_check.run("label_key_host_check", tmp_path, "-ffp-contract=off")
    rows = [ln.split() for ln in r.stdout.splitlines()]
    seen = {"K": 0, "M": 0, "R": 0}
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()   # noqa: E731
    for f in rows:
        seen[f[0]] += 1
        if f[0] == "K":
            x, y, w, h = _f32(f[1]), _f32(f[2]), int(f[3]), int(f[4])
            key = V.label_keys(np.array([x]), np.array([y]), w)
            assert same(key[0], _f32(f[5])), f
            assert int(V.label_slots(key, w, h)[0]) == int(f[6]), f
        elif f[0] == "M":
            k0, k1 = np.array([[_f32(f[1]), _f32(f[2])]]), np.array([[_f32(f[3]), _f32(f[4])]])
            assert len(V.label_pack_np(k0, k1, moved_thr=_f32(f[5]))) == int(f[6]), f
        else:
            x, s, o, v = _f32(f[1]), _f64(f[2]), _f64(f[3]), _f64(f[4])
            k = np.array([[x, x]], dtype=np.float32)
            got = V.label_pack_np(k, k, affine=[s, s, o, o, s, s, o, o], vratio=v)[0, 0]
            assert same(got, _f32(f[5])), f
            assert same(V.label_pack_np(k, k, vratio=v)[0, 0], _f32(f[6])), f
    assert seen == {"K": 4 * 18 * 16, "M": 2 * 10 * 10, "R": 5 * 5 * 4 * 9}, seen
    slots = [int(f[6]) for f in rows if f[0] == "K"]
    assert min(slots) == -1 and max(slots) == 1 << 24 and 0 in slots


def test_importing_video_labels_changes_no_existing_symbol():
    """pose, zeb and demo keep their public names, defaults and code: a fresh interpreter compares them before and after the import"""
    code = (
        "import inspect\n"
        "from gim_amd import pose, zeb, demo\n"
        "def snap():\n"
        "    out = {}\n"
        "    for m in (pose, zeb, demo):\n"
        "        for n, v in sorted(vars(m).items()):\n"
        "            if inspect.isfunction(v):\n"
        "                out[m.__name__, n] = (str(inspect.signature(v)), v.__code__.co_code, v.__defaults__, str(v.__kwdefaults__))\n"
        "            elif isinstance(v, (int, float, str, tuple)):\n"
        "                out[m.__name__, n] = v\n"
        "            else:\n"
        "                out[m.__name__, n] = id(v)\n"
        "    return out\n"
        "a = snap()\n"
        "import gim_amd.video_labels\n"
        "assert a == snap() and len(a) > 100\n"
        "print('same')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("same"), r.stdout + r.stderr
