"""The least-squares refit without a GPU: pose.homography_dlt_ge / eight_point_ge / refit_ge (the numpy restatement of
csrc/model_refit_solve.h) on exact geometry and against LAPACK, the loop's rules and stops, the new keywords of the public surface,
the cap on undecidable points that the GPU test relies on, the new export against the header, the kernel's resources, and
tools/refit_host_check.cpp (the header on the CPU) against the restatement.  tests/model_refit_cases.py builds the inputs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import host_check
import model_refit_cases as C
from gim_amd import demo, pose, pose_math, video_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_CTYPE = {"int": ctypes.c_int, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _fit(kind, a, b):
    return pose.homography_dlt_ge(a, b) if kind == 0 else pose.eight_point_ge(a, b)


def _norm_T(p):
    c = p.mean(0)
    s = np.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(1)).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _system(kind, a, b):
    """the normalised linear system of the fit and its two transforms -> (A [rows, 9], Ta, Tb)"""
    Ta, Tb = _norm_T(a), _norm_T(b)
    p, q = a * Ta[0, 0] + Ta[:2, 2], b * Tb[0, 0] + Tb[:2, 2]
    if kind == 1:
        return pose_math._epipolar_rows(p, q), Ta, Tb
    x, y, u, v = p[:, 0], p[:, 1], q[:, 0], q[:, 1]
    o, z = np.ones_like(x), np.zeros_like(x)
    return np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], 1), np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], 1)]), Ta, Tb


def _lapack(kind, a, b):
    """the same fit with LAPACK's SVDs: pose.homography_dlt, and the textbook normalised eight-point algorithm"""
    if kind == 0:
        return pose.homography_dlt(a, b)
    A, Ta, Tb = _system(1, a, b)
    F = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, s, Vt = np.linalg.svd(F)
    F = Tb.T @ (U @ np.diag([s[0], s[1], 0.0]) @ Vt) @ Ta
    return F / np.linalg.norm(F)


def _residual(kind, M, a, b):
    """(|A h| of the model in the normalised system, h of unit norm; |A|_F, the scale of that evaluation's own rounding)"""
    A, Ta, Tb = _system(kind, a, b)
    h = (Tb @ M @ np.linalg.inv(Ta)) if kind == 0 else (np.linalg.inv(Tb).T @ M @ np.linalg.inv(Ta))
    return np.linalg.norm(A @ (h.ravel() / np.linalg.norm(h))), np.linalg.norm(A)


# ---- exact geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.EXACT_SEEDS)
def test_exact_geometry(seed):
    a, b, H, _ = C.exact(0, seed)
    G = pose.homography_dlt_ge(a, b)
    assert G[2, 2] == 1.0 and np.abs(G - H).max() <= C.EXACT_BAR * np.abs(H).max()
    assert pose.transfer_error(G, a, b).max() < 1e-18 * 640 ** 2
    a, b, F, _ = C.exact(1, seed)
    G = pose.eight_point_ge(a, b)
    assert C.model_diff(1, G, F) <= C.EXACT_BAR
    assert abs(np.linalg.norm(G) - 1.0) <= 1e-15 and abs(np.linalg.det(G)) < 1e-15
    # on the noisy scenes too, the rank is 2 and the norm is 1
    a, b, _, inl = C.noisy(1, C.NOISY_SEEDS[0])
    G = pose.eight_point_ge(a[inl], b[inl])
    assert abs(np.linalg.norm(G) - 1.0) <= 1e-15 and abs(np.linalg.det(G)) < 1e-15
    assert pose.homography_dlt_ge(a[:3], b[:3]) is None and pose.eight_point_ge(a[:7], b[:7]) is None


def test_against_lapack():
    """the model difference and the algebraic residual of both on the inliers of every problem the GPU test runs; the measured
    differences are those of model_refit_cases.H_MEASURED / F_MEASURED, far below the 1e-9 at which A^T A would be a finding"""
    for kind in (0, 1):
        worst, worst_res = 0.0, 0.0
        for seed in C.NOISY_SEEDS:
            for n in C.SIZES[kind]:
                a, b, _, mask = C.problem(kind, seed, n)
                if mask.sum() < pose.MR_MIN_POINTS[kind]:
                    continue
                a, b = a[mask], b[mask]
                G, L = _fit(kind, a, b), _lapack(kind, a, b)
                (rg, scale), (rl, _) = _residual(kind, G, a, b), _residual(kind, L, a, b)
                diff = C.model_diff(kind, G, L)
                print(f"kind {kind} seed {seed} n {n} ({len(a)} inliers): |ge - lapack| {diff:.3g}, |A h| ge {rg:.6g} lapack {rl:.6g}")
                worst, worst_res = max(worst, diff), max(worst_res, abs(rg - rl) / max(rl, 1e-12))
                # equal to 1e-9 of the residual, beyond what evaluating |A h| itself rounds (the model goes through two 3 x 3
                # products and a matrix-vector product of |A|_F: 64 ulp of that is generous and still 1e-13)
                assert abs(rg - rl) <= 1e-9 * rl + 64 * np.finfo(float).eps * scale
        print(f"kind {kind}: largest difference {worst:.3g}, largest relative residual difference {worst_res:.3g}")
        assert worst <= (C.H_MEASURED, C.F_MEASURED)[kind] < 1e-9 / 8


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def _by_hand(kind, a, b, M, thr2, rounds, mask=None):
    err = C.error(kind)
    cur, cur_mask = M, (err(M, a, b) <= thr2) if mask is None else mask
    n0, accepted = int(cur_mask.sum()), 0
    for _ in range(rounds):
        cand = _fit(kind, a[cur_mask], b[cur_mask]) if cur_mask.sum() >= pose.MR_MIN_POINTS[kind] else None
        if cand is None:
            break
        cand_mask = err(cand, a, b) <= thr2
        if cand_mask.sum() < cur_mask.sum():
            break
        same = np.array_equal(cand_mask, cur_mask)
        cur, cur_mask, accepted = cand, cand_mask, accepted + 1
        if same:
            break
    return cur, cur_mask, (n0, int(cur_mask.sum())), accepted


@pytest.mark.parametrize("kind", [0, 1])
def test_loop(kind):
    stops = set()
    for seed in C.NOISY_SEEDS:
        a, b, M, own = C.problem(kind, seed)
        for rounds in (1, 4, 8):
            for with_mask in (False, True):
                model, mask, counts, accepted, info = C.oracle(kind, seed, rounds, with_mask)
                visited = info["counts"][(0 if with_mask else 1):]                       # the candidates' counts
                stops.add(info["stop"])
                assert counts[0] == own.sum() and counts[1] == mask.sum() and 0 <= accepted <= rounds
                run = [counts[0]] + visited[:accepted]
                assert all(y >= x for x, y in zip(run, run[1:])) and run[-1] == counts[1]                 # counts never decrease
                assert len(visited) == accepted + (info["stop"] == "rejected")
                if info["stop"] == "rejected":
                    assert visited[-1] < counts[1]
                if info["stop"] == "rounds":
                    assert accepted == rounds
                if info["stop"] == "fixed":
                    assert accepted >= 1 and (accepted == 1 or visited[accepted - 1] == visited[accepted - 2])
                assert model.tobytes() == (info["models"][(-2 if info["stop"] == "rejected" else -1)]).tobytes()
                assert max(info["off"]) < 1e-30                                                           # the Jacobi sweeps converged
                # a sequential loop over the *_ge fits gives the same (it sums over the compacted inliers, the loop over the lanes of
                # the masked pair: another order, so the model agrees to rounding and everything else exactly)
                hm, hmask, hcounts, hacc = _by_hand(kind, a, b, M, C.THR2, rounds, own if with_mask else None)
                assert C.model_diff(kind, hm, model) <= C.bar(kind) and np.array_equal(hmask, mask) and hcounts == counts and hacc == accepted
        # mask=None is the model's own mask
        x, y = C.oracle(kind, seed, 4, False), C.oracle(kind, seed, 4, True)
        assert x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1]) and x[2:4] == y[2:4]
    assert "rounds" in stops and ({"fixed", "rejected"} & stops)
    with pytest.raises(ValueError):
        pose.refit_ge(kind, a, b, M, C.THR2, rounds=0)
    with pytest.raises(ValueError):
        pose.refit_ge(kind, a, b, M, C.THR2, rounds=9)
    with pytest.raises(ValueError):
        pose.refit_ge(2, a, b, M, C.THR2)


@pytest.mark.parametrize("kind", [0, 1])
def test_stops_and_skips(kind):
    m = pose.MR_MIN_POINTS[kind]
    a, b, M, _ = C.problem(kind, C.SEED, m + 1)
    ones = np.ones(m + 1, dtype=bool)
    # one short of the minimum: nothing happens; the minimum: a candidate is made
    model, mask, counts, acc, info = pose.refit_ge(kind, a[:m - 1], b[:m - 1], M, C.THR2, mask=ones[:m - 1], rounds=4, detail=True)
    assert (acc, counts, info["stop"]) == (0, (m - 1, m - 1), "few") and model.tobytes() == np.asarray(M).tobytes() and mask.all()
    model, mask, counts, acc, info = pose.refit_ge(kind, a[:m], b[:m], M, C.THR2, mask=ones[:m], rounds=4, detail=True)
    assert info["stop"] in ("fixed", "rejected", "rounds") and len(info["models"]) >= 1 and np.isfinite(model).all()
    # all inliers on one point: no extent to normalise by
    same_a, same_b = np.repeat(a[:1], 12, 0), np.repeat(b[:1], 12, 0)
    model, mask, counts, acc, info = pose.refit_ge(kind, same_a, same_b, M, C.THR2, mask=np.ones(12, dtype=bool), detail=True)
    assert (acc, info["stop"]) == (0, "degenerate") and model.tobytes() == np.asarray(M).tobytes()
    if kind == 0:
        # collinear inliers: the candidate is arbitrary, the count rule decides; the output is finite either way
        t = np.linspace(0.0, 1.0, 12)[:, None]
        line_a = np.array([50.0, 60.0]) + t * np.array([400.0, 250.0])
        line_b = np.array([80.0, 40.0]) + t * np.array([380.0, 300.0])
        model, mask, counts, acc, info = pose.refit_ge(0, line_a, line_b, M, C.THR2, mask=np.ones(12, dtype=bool), rounds=2, detail=True)
        assert np.isfinite(model).all() and counts[1] >= 12 or acc == 0
        assert info["stop"] in ("rejected", "fixed", "rounds", "degenerate")
    # a NaN under the mask stops the loop, one outside it changes nothing
    a2, b2, M2, own = C.problem(kind, C.SEED, 256)
    ref = pose.refit_ge(kind, a2, b2, M2, C.THR2, mask=own, rounds=2)
    bad = np.array(a2)
    bad[np.flatnonzero(own)[2], 0] = np.nan
    model, mask, counts, acc, info = pose.refit_ge(kind, bad, b2, M2, C.THR2, mask=own, rounds=2, detail=True)
    assert (acc, info["stop"]) == (0, "nonfinite") and np.array_equal(mask, own) and model.tobytes() == np.asarray(M2).tobytes()
    out = np.array(a2)
    out[np.flatnonzero(~own)[2], 0] = np.nan
    got = pose.refit_ge(kind, out, b2, M2, C.THR2, mask=own, rounds=2)
    assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1]) and got[2:] == ref[2:]
    # a zero or NaN model: the pair is skipped
    for Mbad in (np.zeros((3, 3)), np.where(np.eye(3) > 0, np.nan, M2)):
        model, mask, counts, acc = pose.refit_ge(kind, a2, b2, Mbad, C.THR2, mask=own)
        assert acc == -1 and counts == (0, 0) and not mask.any() and not model.any() and mask.shape == (256,)


def test_decidability_cap():
    """the oracle alone leaves no point of these scenes within 1e-6 (relative) of the threshold under any model it visits: the GPU test
    cannot hide a failure behind exclusions"""
    for kind in (0, 1):
        for seed in C.NOISY_SEEDS:
            for n in C.SIZES[kind]:
                for rounds in (1, 4):
                    for with_mask in (False, True):
                        dec = C.decidable(C.oracle(kind, seed, rounds, with_mask, n)[4])
                        assert len(dec) == n and (~dec).sum() <= C.UNDECIDABLE_CAP * max(n, 1)
                        assert dec.all()


# ---- public surface ----------------------------------------------------------------------------------------------------------------
def test_new_keywords_default_to_the_old_call():
    sig = lambda f: inspect.signature(f).parameters   # noqa: E731
    assert sig(pose.find_homography)["refit"].default == "host"
    for f in (pose.find_fundamental_mat, pose.find_fundamental_mat_batch, pose.verify_pairs, video_labels.label_pair):
        assert sig(f)["refine"].default == 0, f
    assert sig(demo.match_pair)["ransac_refine"].default == 0 and sig(demo.compute_geom)["ransac_refine"].default == 0
    assert sig(demo.compute_geom)["homography_refit"].default == "host"
    assert sig(pose.refit_ge)["rounds"].default == 1 and sig(pose.refit_ge)["mask"].default is None
    from gim_amd import ops
    p = sig(ops.model_refit)
    assert list(p)[:5] == ["kind", "a", "b", "models", "thr2"] and (p["mask"].default, p["offsets"].default, p["rounds"].default) == (None, None, 1)


def test_invalid_combinations_raise_before_a_launch(monkeypatch):
    from gim_amd import ops

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(ops, "lib", NoLaunch())
    a, b, _, _ = C.noisy(0, C.SEED)
    for kw in (dict(refit="device"), dict(refit="gpu"), dict(refit="ge", device="cuda:0"), dict(refit="device", sampler="device")):
        with pytest.raises(ValueError):
            pose.find_homography(a, b, **kw)
    for kw in (dict(refine=-1), dict(refine=9), dict(refine=2, solve="device")):
        with pytest.raises(ValueError):
            pose.find_fundamental_mat(a, b, **kw)
    with pytest.raises(ValueError):
        pose.find_fundamental_mat_batch([(a, b)], device="cuda:0", refine=9)
    with pytest.raises(ValueError):
        pose.verify_pairs([(a, b)], device="cuda:0", refine=-1)
    with pytest.raises(SystemExit):
        demo.main(["--ransac-refine", "9"])
    with pytest.raises(TypeError):
        pose.DeviceEssential.refit(None, np.eye(3))


def test_find_homography_refit_ge():
    for seed in C.NOISY_SEEDS:
        a, b, _, _ = C.noisy(0, seed)
        Hh, mh = pose.find_homography(a, b, C.THR, max_iters=2000, seed=seed)
        Hg, mg = pose.find_homography(a, b, C.THR, max_iters=2000, seed=seed, refit="ge")
        with np.errstate(all="ignore"):
            dec = np.abs(pose.transfer_error(Hh, a, b) - C.THR2) / C.THR2 >= C.DECIDE
        print(f"seed {seed}: inliers host {int(mh.sum())} ge {int(mg.sum())}, H diff {C.model_diff(0, Hg, Hh):.3g}")
        assert dec.all() and np.array_equal(mg, mh) and C.model_diff(0, Hg, Hh) <= C.H_BAR and Hg[2, 2] == 1.0


def test_find_fundamental_refine():
    for seed in C.NOISY_SEEDS:
        a, b, _, inl = C.noisy(1, seed)
        F0, m0 = pose.find_fundamental_mat(a, b, C.THR, max_iters=2000, seed=seed, solve="ge", sampler="philox")
        F3, m3 = pose.find_fundamental_mat(a, b, C.THR, max_iters=2000, seed=seed, solve="ge", sampler="philox", refine=3)
        e0, e3 = pose.sampson_error(F0, a, b)[inl].mean(), pose.sampson_error(F3, a, b)[inl].mean()
        print(f"seed {seed}: inliers {int(m0.sum())} -> {int(m3.sum())}, mean Sampson error over the true inliers {e0:.4f} -> {e3:.4f} px^2")
        assert F0.tobytes() == np.asarray(C.start_model(1, seed)).tobytes()
        assert m3.sum() >= m0.sum() and e3 < e0 and abs(np.linalg.det(F3)) < 1e-15
        want = C.oracle(1, seed, 3, False)
        assert F3.tobytes() == want[0].tobytes() and np.array_equal(m3, want[1])
    # the host solver's model is refined the same way
    Fh, mh = pose.find_fundamental_mat(a[:400], b[:400], C.THR, max_iters=500, seed=1, refine=2)
    F_, m_ = pose.find_fundamental_mat(a[:400], b[:400], C.THR, max_iters=500, seed=1)
    assert mh.sum() >= m_.sum() and pose.find_fundamental_mat(a[:5], b[:5], refine=2)[0] is None


# ---- the library -------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def test_export_follows_the_header_within_revision_115():
    from gim_amd import _lib
    fn = _lib.lib.gim_model_refit
    res, args = _header_prototype("gim_model_refit")
    assert (res, args) == _lib.PROTOTYPES["gim_model_refit"] and len(args) == 14
    assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    err = _lib.lib.gim_last_error
    # an empty batch returns before anything is touched; malformed calls are refused before a launch
    assert fn(0, None, None, None, 0, None, None, 1.0, 1, None, None, None, None, None) == 0
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    assert fn(2, p, p, p, 1, p, None, 1.0, 1, p, p, p, p, None) != 0 and b"kind" in err()
    assert fn(-1, p, p, p, 1, p, None, 1.0, 1, p, p, p, p, None) != 0 and b"kind" in err()
    assert fn(0, p, p, p, 1, p, None, 1.0, 0, p, p, p, p, None) != 0 and b"rounds" in err()
    assert fn(1, p, p, p, 1, p, None, 1.0, 9, p, p, p, p, None) != 0 and b"rounds" in err()
    assert fn(0, p, p, p, 1, None, None, 1.0, 1, p, p, p, p, None) != 0 and b"NULL" in err()
    assert fn(0, None, p, p, 1, p, None, 1.0, 1, p, p, p, p, None) != 0 and b"NULL" in err()
    assert fn(0, p, p, p, 1, p, None, 1.0, 1, p, None, p, p, None) != 0 and b"NULL" in err()
    assert fn(0, p, p, p, 1, p, None, 1.0, 1, p, p, p, None, None) != 0 and b"NULL" in err()
    assert fn(0, p, off(8), p, 1, p, None, 1.0, 1, p, p, p, p, None) != 0 and b"16-byte" in err()
    assert fn(0, p, p, p, 1, off(4), None, 1.0, 1, p, p, p, p, None) != 0 and b"misaligned" in err()
    assert fn(0, p, p, off(2), 1, p, None, 1.0, 1, p, p, p, p, None) != 0 and b"misaligned" in err()
    assert fn(0, p, p, p, 1, p, None, 1.0, 1, off(4), p, p, p, None) != 0 and b"misaligned" in err()
    assert fn(0, p, p, p, 1, p, None, 1.0, 1, p, p, off(2), p, None) != 0 and b"misaligned" in err()
    assert fn(0, p, p, p, 1, p, None, 1.0, 1, p, p, p, off(2), None) != 0 and b"misaligned" in err()
    assert fn(0, p, p, p, 65536, p, None, 1.0, 1, p, p, p, p, None) != 0 and b"65535" in err()
    assert fn(0, p, p, p, -1, p, None, 1.0, 1, p, p, p, p, None) != 0


def test_kernel_targets_gfx950_without_scratch():
    """model_refit_kernel<0> / <1>: 596 / 604 registers as the resource test counts them (VGPRs + AGPRs; the 45 partial sums of a lane
    are 90), 3 280 bytes of LDS, no scratch, no spilled vector register on the build that wrote this test; one workgroup per pair, so
    occupancy is not what the kernel lives on.  The bar is no scratch and no spills"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hit = [(n, v) for n, v in kr._kernels().items() if "model_refit_kernel<" in n]
    assert len(hit) >= 2, "model_refit_kernel<0> and <1> not found in the library"
    for n, (regs, scratch, spills) in hit:
        print(f"{n[:48]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (n, regs, scratch, spills)


def test_host_check_agrees_with_the_numpy_oracle(tmp_path):
    """tools/refit_host_check.cpp is plain C++ over the kernel's header; built with the host compiler (no sanitizer here: that run is
    a development step, recorded in the README), its self-check passes and the models it prints equal the restatement's to 1e-12 on
    the scenes it prints"""
    r = host_check.run("refit_host_check", tmp_path)
    assert r.stdout.strip().endswith("OK"), r.stdout[-2000:]
    lines = r.stdout.strip().split("\n")
    i, scenes = 0, 0
    while lines[i].startswith("scene"):
        _, _, _, kind, P = lines[i].split()
        kind, P = int(kind), int(P)
        pts = np.array([[float(v) for v in ln.split()] for ln in lines[i + 1:i + 1 + P]])
        a, b = pts[:, :2], pts[:, 2:]
        fit, start, refit, mask = (lines[i + 1 + P + k].split() for k in range(4))
        assert (fit[0], start[0], refit[0], mask[0]) == ("fit", "start", "refit", "mask")
        keep = np.arange(P) % 3 != 2
        want = _fit(kind, a[keep], b[keep])
        # gim_mr_fit sums over the lanes of the masked pair, *_ge over the compacted points: another order, the same model to rounding
        assert np.abs(np.array(fit[1:], dtype=float).reshape(3, 3) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        M0 = np.array(start[1:], dtype=float).reshape(3, 3)
        model, m, counts, acc = pose.refit_ge(kind, a, b, M0, 1.0, rounds=4)
        assert [int(v) for v in refit[1:4]] == [acc, *counts]
        assert np.abs(np.array(refit[4:], dtype=float).reshape(3, 3) - model).max() <= 1e-12 * max(1.0, np.abs(model).max())
        assert mask[1] == "".join("1" if v else "0" for v in m)
        i += 5 + P
        scenes += 1
    assert scenes == 6 and lines[i] == "OK"
