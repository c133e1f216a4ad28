"""GPU tests of the least-squares refit (gim_amd/csrc/model_refit.hip through ops.model_refit, and `refit=` / `refine=` through pose,
video_labels and the demo) against pose.refit_ge, the numpy restatement of the kernel's arithmetic: counts and `accepted` equal,
masks equal on every decidable point (tests/test_model_refit_cpu.py caps the undecidable ones on the CPU: none on these seeds),
models within the bar measured against LAPACK there.  Inputs: tests/model_refit_cases.py."""
import numpy as np
import pytest
import torch

import model_refit_cases as C
from gim_amd import demo, ops, pose, video_labels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def d(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cases are frozen


def _run(kind, a, b, M, mask, rounds, offsets=None):
    out = ops.model_refit(kind, d(a), d(b), d(M), C.THR2, mask=None if mask is None else d(mask), offsets=None if offsets is None else d(offsets),
                          rounds=rounds)
    return tuple(t.cpu().numpy() for t in out)


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("rounds", [1, 4])
@pytest.mark.parametrize("kind", [0, 1])
def test_kernel_equals_the_oracle(kind, rounds, with_mask):
    seen = set()
    for n in C.SIZES[kind]:
        a, b, M, mask = C.problem(kind, C.SEED, n)
        want_M, want_mask, want_counts, want_acc, info = C.oracle(kind, C.SEED, rounds, with_mask, n)
        got_M, got_mask, got_counts, got_acc = _run(kind, a, b, M, mask if with_mask else None, rounds)
        dec = C.decidable(info)
        diff = C.model_diff(kind, got_M, want_M) if want_acc > 0 else float(np.abs(got_M - want_M).max())
        print(f"kind {kind} rounds {rounds} mask {with_mask} P {n}: counts {got_counts.tolist()} accepted {int(got_acc)} "
              f"({info['stop']}), undecidable {int((~dec).sum())}, model diff {diff:.3g} (bar {C.bar(kind):.3g})")
        assert got_mask.dtype == bool and got_mask.shape == (n,) and got_M.shape == (3, 3)
        assert tuple(got_counts.tolist()) == want_counts and int(got_acc) == want_acc
        assert np.array_equal(got_mask[dec], want_mask[dec])
        if want_acc > 0:
            assert diff <= C.bar(kind)
            assert got_M[2, 2] == 1.0 if kind == 0 else abs(np.linalg.norm(got_M) - 1.0) <= 1e-15
        else:
            assert got_M.tobytes() == np.asarray(M).tobytes()                            # nothing accepted: the input model, untouched
        seen.add(info["stop"])
    assert "few" in seen and len(seen) >= 2                                              # the minimum-count stop and a proper end


def test_ragged_batch_equals_single_calls_bit_for_bit():
    for kind in (0, 1):
        small = C.SIZES[kind][1]                                                         # 3 / 7: below the minimum
        a2, b2, M, m2 = C.problem(kind, C.SEED, 2000)
        a256, b256, _, m256 = C.problem(kind, C.SEED, 256)
        a_s, b_s, _, m_s = C.problem(kind, C.SEED, small)
        nan_a = np.array(a256[:100])
        nan_a[int(np.flatnonzero(m256[:100])[3]), 1] = np.nan                            # under the mask
        pairs = [(a2, b2, M, m2), (a256, b256, M, m256), (a_s, b_s, M, m_s), (a256[:64], b256[:64], np.zeros((3, 3)), m256[:64]),
                 (nan_a, b256[:100], M, m256[:100]), (a2[:0], b2[:0], M, m2[:0])]
        offsets = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int32)
        singles = [_run(kind, a, b, Mb, mask, 4) for a, b, Mb, mask in pairs]
        assert [int(s[3]) for s in singles][2:] == [0, -1, 0, 0] and int(singles[0][3]) >= 1 and int(singles[1][3]) >= 1
        assert singles[4][0].tobytes() == np.asarray(M).tobytes() and np.array_equal(singles[4][1], m256[:100])
        A, Bp = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
        Ms, masks = np.stack([p[2] for p in pairs]), np.concatenate([p[3] for p in pairs])
        for mask_in in (masks, None):
            if mask_in is None:                                                          # the NaN point is then outside every mask
                singles = [_run(kind, a, b, Mb, None, 4) for a, b, Mb, _ in pairs]
                assert int(singles[4][3]) >= 0 and singles[4][2][1] >= singles[4][2][0] > 0
            got = _run(kind, A, Bp, Ms, mask_in, 4, offsets)
            assert got[0].tobytes() == np.stack([s[0] for s in singles]).tobytes()
            assert np.array_equal(got[1], np.concatenate([s[1] for s in singles]))
            assert np.array_equal(got[2], np.stack([s[2] for s in singles])) and np.array_equal(got[3], np.stack([s[3] for s in singles]))
        # guard bytes and words around every output, through the library entry: offsets that start inside the mask buffer
        from gim_amd._lib import check, lib
        G, P, B = 64, int(offsets[-1]), len(pairs)
        mask_out = torch.full((G + P + G,), 0xAB, dtype=torch.uint8, device=DEV)
        models_out = torch.full((9 + 9 * B + 9,), -7.0, dtype=torch.float64, device=DEV)
        counts = torch.full((2 + 2 * B + 2,), -7, dtype=torch.int32, device=DEV)
        accepted = torch.full((2 + B + 2,), -7, dtype=torch.int32, device=DEV)
        pts_a = torch.cat([torch.zeros(G, 2, dtype=torch.float64, device=DEV), d(A)])   # the points shifted as the offsets are
        pts_b = torch.cat([torch.zeros(G, 2, dtype=torch.float64, device=DEV), d(Bp)])
        mask_in = torch.cat([torch.ones(G, dtype=torch.uint8, device=DEV), d(masks).view(torch.uint8)])
        off = d(offsets + G)
        check(lib.gim_model_refit(kind, pts_a.data_ptr(), pts_b.data_ptr(), off.data_ptr(), B, d(Ms).data_ptr(), mask_in.data_ptr(), C.THR2, 4,
                                  models_out[9:].data_ptr(), mask_out.data_ptr(), counts[2:].data_ptr(), accepted[2:].data_ptr(), None),
              "gim_model_refit")
        torch.cuda.synchronize()
        mo, mm, cc, aa = models_out.cpu().numpy(), mask_out.cpu().numpy(), counts.cpu().numpy(), accepted.cpu().numpy()
        assert (mm[:G] == 0xAB).all() and (mm[G + P:] == 0xAB).all() and set(np.unique(mm[G:G + P]).tolist()) <= {0, 1}
        assert (mo[:9] == -7.0).all() and (mo[-9:] == -7.0).all() and (cc[:2] == -7).all() and (cc[-2:] == -7).all()
        assert (aa[:2] == -7).all() and (aa[-2:] == -7).all()
        first = [_run(kind, a, b, Mb, mask, 4) for a, b, Mb, mask in pairs]
        assert mo[9:-9].tobytes() == np.stack([s[0] for s in first]).tobytes() and np.array_equal(aa[2:-2], np.stack([s[3] for s in first]))
        assert np.array_equal(mm[G:G + P].astype(bool), np.concatenate([s[1] for s in first]))


# ---- entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["host", "philox", "device"])
def test_find_homography_refit_on_the_device(sampler, monkeypatch):
    a, b, _, _ = C.noisy(0, C.SEED)
    Hh, mh = pose.find_homography(a, b, C.THR, 0.999999, 2000, seed=3, device=DEV, sampler=sampler, refit="host")
    calls = []
    real = ops.homography_mask
    monkeypatch.setattr(ops, "homography_mask", lambda *x, **k: calls.append(1) or real(*x, **k))
    Hd, md = pose.find_homography(a, b, C.THR, 0.999999, 2000, seed=3, device=DEV, sampler=sampler, refit="device")
    assert Hh is not None and Hd is not None and md.dtype == bool and md.shape == mh.shape
    if sampler == "device":
        assert calls == []                                   # the refit's launch took the RANSAC's mask too
    with np.errstate(all="ignore"):
        margin = np.abs(pose.transfer_error(Hh, a, b) - C.THR2) / C.THR2
    dec = margin >= C.DECIDE
    print(f"sampler {sampler}: inliers host {int(mh.sum())} device {int(md.sum())}, undecidable {int((~dec).sum())}, "
          f"H diff {C.model_diff(0, Hd, Hh):.3g} (bar {C.H_BAR:.3g})")
    assert (~dec).mean() <= C.UNDECIDABLE_CAP
    assert C.model_diff(0, Hd, Hh) <= C.H_BAR and np.array_equal(md[dec], mh[dec]) and mh.sum() > 800


def test_find_fundamental_refine_on_the_device():
    a, b, _, _ = C.noisy(1, C.SEED)
    Fd, md = pose.find_fundamental_mat(a, b, C.THR, max_iters=2000, seed=C.SEED, device=DEV, solve="device", sampler="philox", refine=3)
    Fg, mg = pose.find_fundamental_mat(a, b, C.THR, max_iters=2000, seed=C.SEED, device=None, solve="ge", sampler="philox", refine=3)
    info = pose.refit_ge(1, a, b, C.start_model(1, C.SEED), C.THR2, rounds=3, detail=True)[4]
    dec = C.decidable(info)
    print(f"inliers device {int(md.sum())} ge {int(mg.sum())}, undecidable {int((~dec).sum())}, F diff {C.model_diff(1, Fd, Fg):.3g} (bar {C.F_BAR:.3g})")
    assert C.model_diff(1, Fd, Fg) <= C.F_BAR and np.array_equal(md[dec], mg[dec]) and md.sum() >= 1000
    # the host-solved run scored on the device refits there too
    Fs, ms = pose.find_fundamental_mat(a, b, C.THR, max_iters=2000, seed=C.SEED, device=DEV, refine=3)
    F0, m0 = pose.find_fundamental_mat(a, b, C.THR, max_iters=2000, seed=C.SEED, device=DEV)
    assert ms.sum() >= m0.sum() and abs(np.linalg.norm(Fs) - 1.0) <= 1e-15


def test_batch_and_verify_pairs_equal_single_calls(monkeypatch):
    a, b, _, _ = C.noisy(1, C.SEED)
    a2, b2, _, _ = C.noisy(1, C.NOISY_SEEDS[1])
    rng = np.random.default_rng(5)
    junk = (rng.uniform(0, 640, (40, 2)), rng.uniform(0, 480, (40, 2)))
    pairs = [(a[:600], b[:600]), (a[:5], b[:5]), (a2[:400], b2[:400]), junk, (a[:0], b[:0])]
    for sampler in ("philox", "device"):
        got = pose.find_fundamental_mat_batch(pairs, C.THR, max_iters=500, seed=2, device=DEV, sampler=sampler, refine=2)
        ver = pose.verify_pairs(pairs, C.THR, device=DEV, max_iters=500, seed=2, batch=3, sampler=sampler, refine=2)
        for (pa, pb), g, v in zip(pairs, got, ver):
            F1, m1 = pose.find_fundamental_mat(pa, pb, C.THR, max_iters=500, seed=2, device=DEV, solve="device", sampler=sampler, refine=2)
            for F, m in (g, v):
                assert (F is None) == (F1 is None) and (F is None or F.tobytes() == F1.tobytes())
                assert m.dtype == bool and np.array_equal(m, m1)
        assert got[0][0] is not None and got[2][0] is not None and got[1][0] is None and got[4][0] is None
        plain = pose.find_fundamental_mat_batch(pairs, C.THR, max_iters=500, seed=2, device=DEV, sampler=sampler)
        assert got[0][1].sum() >= plain[0][1].sum() and got[2][1].sum() >= plain[2][1].sum()
    # a batch without any model launches no refit
    monkeypatch.setattr(ops, "model_refit", lambda *x, **k: (_ for _ in ()).throw(AssertionError("launched")))
    for sampler in ("philox", "device"):
        none = pose.find_fundamental_mat_batch([(a[:5], b[:5]), (a[:0], b[:0])], C.THR, device=DEV, sampler=sampler, refine=2)
        assert [g[0] for g in none] == [None, None]


def test_label_pair_and_demo_pass_refine_through():
    a, b, _, _ = C.noisy(1, C.SEED)
    k0, k1 = a.astype(np.float32), b.astype(np.float32)
    kw = dict(device=DEV, threshold=1.0, max_iters=2000, seed=1)
    plain = video_labels.label_pair((k0, k1), **kw)
    fine = video_labels.label_pair((k0, k1), refine=2, **kw)
    print(f"label_pair rows: refine=0 {len(plain)}, refine=2 {len(fine)}")
    assert fine.shape[1] == 4 and len(fine) >= len(plain) > 800
    out = {"mkpts0_f": torch.from_numpy(k0).to(DEV), "mkpts1_f": torch.from_numpy(k1).to(DEV)}
    g0 = demo.compute_geom(out, device=DEV, ransac_solve="device", ransac_sampler="device")
    g2 = demo.compute_geom(out, device=DEV, ransac_solve="device", ransac_sampler="device", ransac_refine=2, homography_refit="device")
    p0, p1 = k0.astype(np.float64), k1.astype(np.float64)
    n0 = int((pose.sampson_error(g0["Fundamental"], p0, p1) <= 1.0).sum())
    n2 = int((pose.sampson_error(g2["Fundamental"], p0, p1) <= 1.0).sum())
    print(f"compute_geom inliers: refine=0 {n0}, refine=2 {n2}")
    assert n2 >= n0 > 800
    assert g2["Homography"] is None or (g2["Homography"].shape == (3, 3) and g2["Homography"][2, 2] == 1.0)
