"""gim_ransac_score / gim_ransac_mask (csrc/ransac_score.hip) and the scorer hook of gim_amd/pose.py, without a GPU: the symbols are
exported and bound with the header's signatures, they moved no ABI revision (the library is at 115), the kernels are gfx950 code objects without scratch or
spills (AMDGPU metadata notes, like tests/test_feature_bank_resources_cpu.py), and the RANSAC loop driven through a scorer object --
here a numpy one that calls pose.sampson_error -- returns what the host path returns for the same seed, one pair at a time and
several pairs in lockstep (find_essential_mat_batch)."""
import ctypes
import importlib.util
import os
import re

import numpy as np

from gim_amd import pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
_kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kr)

# C parameter type (pointer levels collapsed) -> the ctypes type gim_amd/_lib.py uses for it
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]])
    return _CTYPE[m.group(1)], args


def test_both_symbols_are_exported_with_the_headers_signatures():
    from gim_amd import _lib
    for name, nargs in (("gim_ransac_score", 10), ("gim_ransac_mask", 8)):
        assert name in _lib.PROTOTYPES
        fn = getattr(_lib.lib, name)                   # AttributeError: the symbol is missing from the library
        res, args = _header_prototype(name)
        assert (res, args) == _lib.PROTOTYPES[name], (name, res, args, _lib.PROTOTYPES[name])
        assert fn.restype is res and list(fn.argtypes) == args and len(args) == nargs
        assert ctypes.c_double in args and ctypes.c_float not in args      # thr2 crosses the ABI in fp64


def test_abi_revision_is_still_114():
    """(named after the revision these exports arrived in; 115 gave the fused kernels their dtype tag)"""
    from gim_amd import _lib
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    assert re.findall(r"^ \* (\d{3})\b", open(HEADER).read(), re.M)[-1] == "115"


def test_host_argument_checks_need_no_gpu():
    """the entry points return for empty problems and refuse malformed arguments before they touch the device"""
    from gim_amd import _lib
    score, mask = _lib.lib.gim_ransac_score, _lib.lib.gim_ransac_mask
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert score(None, None, None, None, None, 0, 7, 1e-6, None, None) == 0      # B == 0
    assert score(None, None, None, None, None, 3, 0, 1e-6, None, None) == 0      # K == 0
    assert mask(None, None, None, None, 0, 1e-6, None, None) == 0
    assert score(p, None, p, p, p, -1, 4, 1e-6, p, None) != 0
    assert score(p, None, None, p, p, 1, 4, 1e-6, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert score(p, None, ctypes.c_void_p(p.value + 8), p, p, 1, 4, 1e-6, p, None) != 0 and b"16-byte" in _lib.lib.gim_last_error()
    assert mask(p, p, p, None, 1, 1e-6, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert mask(p, p, ctypes.c_void_p(p.value + 8), p, 1, 1e-6, p, None) != 0


def test_kernels_target_gfx950_without_scratch_or_spills():
    ks = _kr._kernels()          # asserts the gfx950 target of every code object it parses
    for key in ("ransac_score_kernel(", "ransac_mask_kernel("):
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert hit, f"{key[:-1]} not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
            assert regs <= 128, f"{n}: {regs} VGPRs"     # nine fp64 coefficients + four unrolled points: four waves per SIMD at least


# ---- the scorer hook of pose._ransac -------------------------------------------------------------------------------------------
class NumpyScorer:
    """the interface of pose.DeviceScorer on the host, through pose.sampson_error (one pair, or pairs concatenated + offsets)"""

    def __init__(self, x0, x1, thr2, offsets=None):
        self.x0, self.x1, self.thr2, self.offsets = x0, x1, thr2, offsets
        self.count_calls = self.mask_calls = 0

    def _pair(self, b):
        o = self.offsets
        return self.x0[o[b]:o[b + 1]], self.x1[o[b]:o[b + 1]]

    def counts(self, Ms, valid):
        self.count_calls += 1
        if self.offsets is None:
            return np.where(valid, (pose.sampson_error(Ms, self.x0, self.x1) <= self.thr2).sum(-1), 0).astype(np.int64)
        return np.stack([np.where(valid[b], (pose.sampson_error(Ms[b], *self._pair(b)) <= self.thr2).sum(-1), 0)
                         for b in range(len(self.offsets) - 1)]).astype(np.int64)

    def mask(self, M):
        self.mask_calls += 1
        if self.offsets is None:
            return pose.sampson_error(M, self.x0, self.x1) <= self.thr2
        return np.concatenate([pose.sampson_error(M[b], *self._pair(b)) <= self.thr2 for b in range(len(self.offsets) - 1)])


def _scene(rng, n, noise=0.0, outliers=0):
    """the two-view scene of tests/test_pose_cpu.py: normalised points of n 3-D points under a known pose"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(0.25) * Kx + (1 - np.cos(0.25)) * Kx @ Kx
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1)
    Y = X @ R.T + t
    x0, x1 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    x0 = x0 + rng.normal(size=x0.shape) * noise
    x1 = x1 + rng.normal(size=x1.shape) * noise
    x1[:outliers] = rng.uniform(-0.5, 0.5, (outliers, 2))
    return x0, x1


def test_ransac_through_a_scorer_equals_the_host_path():
    rng = np.random.default_rng(21)
    x0, x1 = _scene(rng, 400, noise=2e-4, outliers=200)
    thr = 1e-3
    E, mask = pose._ransac(x0, x1, pose.five_point, 5, thr, 0.99999, 1000, np.random.default_rng(3))
    S = NumpyScorer(x0, x1, thr ** 2)
    E2, mask2 = pose._ransac(x0, x1, pose.five_point, 5, thr, 0.99999, 1000, np.random.default_rng(3), scorer=S)
    assert E is not None and mask.sum() > 150
    assert np.array_equal(E, E2) and np.array_equal(mask, mask2) and mask2.dtype == bool
    assert S.count_calls >= 1 and S.mask_calls == 1          # the loop went through the scorer, with one final mask call
    assert np.array_equal(pose.find_essential_mat(x0, x1, thr, prob=0.99999, seed=3)[0], E)
    # a run that finds nothing does not ask for a mask
    S0 = NumpyScorer(x0, x1, -1.0)                           # no error is <= -1: every count is 0
    assert pose._ransac(x0, x1, pose.five_point, 5, thr, 0.99999, 250, np.random.default_rng(3), scorer=S0)[0] is None and S0.mask_calls == 0


def test_batch_in_lockstep_equals_the_single_calls():
    rng = np.random.default_rng(22)
    pairs = [_scene(rng, 300, noise=2e-4, outliers=150),     # 50 % outliers: several steps
             _scene(rng, 200),                               # noise-free: one step is enough
             tuple(a[:4] for a in _scene(rng, 10))]          # 4 points: no model
    thr, seed = 1e-3, 5
    offsets = np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs])])
    S = NumpyScorer(np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs]), thr ** 2, offsets)
    got = pose.find_essential_mat_batch(pairs, thr, prob=0.99999, max_iters=1000, seed=seed, scorer=S)
    assert len(got) == 3 and S.mask_calls == 1
    steps = []
    for (a, b), (E, mask) in zip(pairs, got):
        S1 = NumpyScorer(a, b, thr ** 2)
        E1, mask1 = pose._ransac(a, b, pose.five_point, 5, thr, 0.99999, 1000, np.random.default_rng(seed), scorer=S1)
        steps.append(S1.count_calls)
        Eh, maskh = pose.find_essential_mat(a, b, thr, prob=0.99999, max_iters=1000, seed=seed)
        assert (E is None) == (Eh is None) and np.array_equal(mask, maskh) and mask.shape == (len(a),) and mask.dtype == bool
        assert E is None or (np.array_equal(E, Eh) and np.array_equal(E, E1))
    assert got[2][0] is None and not got[2][1].any() and got[0][0] is not None and got[1][1].all()
    assert steps[0] > steps[1] == 1 and steps[2] == 0        # the pairs really finish at different steps
    assert S.count_calls == max(steps)                       # one scoring call per lockstep step, for all pairs together
    # without a device or a scorer the pairs run one by one on the host
    host = pose.find_essential_mat_batch(pairs, thr, prob=0.99999, max_iters=1000, seed=seed)
    assert all(np.array_equal(h[1], g[1]) for h, g in zip(host, got)) and pose.find_essential_mat_batch([], thr) == []
