"""GPU tests of recoverPose on the device (gim_amd/csrc/recover_pose.hip, ops.recover_pose, pose.recover_pose(device=),
pose.DeviceEssential.recover and `recover="device"` through zeb) against pose.recover_pose_ge, the numpy restatement of the kernel's
arithmetic: counts, winner and mask exactly on decidable points, R and t within C.RT_BAR (8 x the difference measured between
recover_pose_ge and LAPACK, tests/recover_pose_cases.py), and against recover="host" end to end.  Inputs:
tests/recover_pose_cases.py."""
import numpy as np
import pytest
import torch

import recover_pose_cases as C
from gim_amd import ops, pose, zeb
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def d(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cases are frozen


def _check_pair(got, E, x0, x1, dthr=1e9, mask=None):
    """one pair's (n_good, best, R, t, mask_out) as numpy against recover_pose_ge"""
    n_good, best, R, t, good = got
    n, Rg, tg, goodg, counts, bestg = pose.recover_pose_ge(E, x0, x1, dthr, mask=mask, detail=True)
    dec = C.decidable(E, x0, x1, dthr) if bestg >= 0 and len(x0) else np.ones(len(x0), dtype=bool)
    assert (~dec).mean() <= C.UNDECIDABLE_CAP if len(dec) else True
    dR, dt = float(np.abs(R - Rg).max()), float(np.abs(t - tg).max())
    print(f"P {len(x0)}: undecidable {int((~dec).sum())}, counts {n_good.tolist()}, best {int(best)}, |dR| {dR:.3e}, |dt| {dt:.3e}")
    if dec.all():
        assert n_good.tolist() == counts.tolist() and int(best) == bestg
    assert int(best) == bestg and np.array_equal(good[dec], goodg[dec])
    assert dR <= C.RT_BAR and dt <= C.RT_BAR
    assert good.dtype == bool and good.shape == (len(x0),)


@pytest.mark.parametrize("P", [0, 1, 5, 255, 256, 257, 2000])
def test_one_pair_equals_the_numpy_oracle(P):
    E, x0, x1, _, _ = C.scene(101 if P == 2000 else 120 + P, P)
    out = ops.recover_pose(d(E), d(x0), d(x1))
    assert [tuple(o.shape) for o in out] == [(4,), (), (3, 3), (3,), (P,)] and out[0].dtype == torch.int32 and out[4].dtype == torch.bool
    assert all(o.device == torch.device(DEV) for o in out)
    _check_pair([o.cpu().numpy() for o in out], E, x0, x1)
    if P in (257, 2000):
        holes = C.mask_with_holes(P)
        for m in (d(holes), d(holes.astype(np.uint8))):
            _check_pair([o.cpu().numpy() for o in ops.recover_pose(d(E), d(x0), d(x1), mask=m, distance_thresh=5.0)], E, x0, x1, 5.0, holes)
        n, R, t, good = pose.recover_pose(E, x0, x1, 5.0, mask=holes, device=DEV)                     # the wrapper of pose
        ref = ops.recover_pose(d(E), d(x0), d(x1), mask=d(holes), distance_thresh=5.0)
        assert n == int(ref[0][int(ref[1])]) and np.array_equal(R, ref[2].cpu().numpy()) and np.array_equal(t, ref[3].cpu().numpy())
        assert np.array_equal(good, ref[4].cpu().numpy()) and n > 0


def test_edges_of_one_pair():
    E, x0, x1, _, _ = C.scene(101, 2000)
    n_good, best, R, t, good = ops.recover_pose(d(E), d(x0), d(x1), mask=d(np.zeros(2000, dtype=bool)))
    assert not n_good.any() and int(best) == 0 and not good.any()
    Eb, b0, b1 = C.behind_scene()
    _check_pair([o.cpu().numpy() for o in ops.recover_pose(d(Eb), d(b0), d(b1))], Eb, b0, b1)
    assert not ops.recover_pose(d(Eb), d(b0), d(b1))[0].any()
    for bad in (np.zeros((3, 3)), np.where(np.eye(3) > 0, np.nan, E), np.where(np.eye(3) > 0, -np.inf, E)):
        n_good, best, R, t, good = ops.recover_pose(d(bad), d(x0), d(x1))
        assert not n_good.any() and int(best) == -1 and not R.any() and not t.any() and not good.any()
        assert pose.recover_pose(bad, x0, x1, device=DEV)[0] == 0
    ref = [o.cpu().numpy() for o in ops.recover_pose(d(E), d(x0), d(x1))]
    for scale in (-1.0, 1e-6):
        got = [o.cpu().numpy() for o in ops.recover_pose(d(scale * E), d(x0), d(x1))]
        _check_pair(got, scale * E, x0, x1)
        assert sorted(got[0].tolist()) == sorted(ref[0].tolist()) and C.same_pose(got[2], got[3], ref[2], ref[3])
        assert np.array_equal(got[4], ref[4])


def test_ragged_batch_equals_the_single_calls():
    E, x0, x1, offsets, mask = C.ragged_batch()
    Ptot = int(offsets[-1])
    dx0, dx1, dE, doff, dmask = d(x0), d(x1), d(E), d(offsets), d(mask)
    n_good, best, R, t, good = ops.recover_pose(dE, dx0, dx1, mask=dmask, offsets=doff, distance_thresh=50.0)
    assert n_good.shape == (4, 4) and best.shape == (4,) and R.shape == (4, 3, 3) and t.shape == (4, 3) and good.shape == (Ptot,)
    assert best.tolist()[1] == 0 and best.tolist()[3] == -1 and not n_good[1].any() and not n_good[3].any()
    assert not R[3].any() and not t[3].any() and not good[offsets[3]:].any()
    for b in range(4):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        one = ops.recover_pose(dE[b].clone(), dx0[lo:hi].clone(), dx1[lo:hi].clone(), mask=dmask[lo:hi].clone(), distance_thresh=50.0)
        got = (n_good[b], best[b], R[b], t[b], good[lo:hi])
        assert all(torch.equal(a, c) for a, c in zip(got, one)), b                                  # bit for bit
        _check_pair([o.cpu().numpy() for o in got], E[b], x0[lo:hi], x1[lo:hi], 50.0, mask[lo:hi])
    assert n_good[0].max() > 50 and n_good[2].max() > 50


def test_nothing_is_written_outside_a_pair(monkeypatch):
    """mask_out is allocated by the wrapper, so the sentinel goes through the entry point: a buffer of Ptot + 64 bytes filled with
    0xAB, the kernel sees its first Ptot bytes; the 64 behind the last pair's end (and a zero-E pair's range apart from its zeros)
    keep the sentinel"""
    E, x0, x1, offsets, mask = C.ragged_batch()
    Ptot = int(offsets[-1])
    buf = torch.full((Ptot + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    R, t = torch.full((5, 3, 3), 7.0, dtype=torch.float64, device=DEV), torch.full((5, 3), 7.0, dtype=torch.float64, device=DEV)
    n_good, best = torch.full((5, 4), 77, dtype=torch.int32, device=DEV), torch.full((5,), 77, dtype=torch.int32, device=DEV)
    p = lambda x: x.data_ptr()   # noqa: E731
    dE, dx0, dx1, doff, dmask = d(E), d(x0), d(x1), d(offsets), d(mask.astype(np.uint8))
    rc = ops.lib.gim_recover_pose(p(dE), p(dx0), p(dx1), p(doff), 4, p(dmask), 50.0, p(R), p(t), p(n_good), p(best), p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert (buf[Ptot:] == 0xAB).all() and (buf[:Ptot] <= 1).all()
    assert (R[4] == 7.0).all() and (t[4] == 7.0).all() and (n_good[4] == 77).all() and int(best[4]) == 77
    ref = ops.recover_pose(dE, dx0, dx1, mask=dmask, offsets=doff, distance_thresh=50.0)
    assert torch.equal(buf[:Ptot].view(torch.bool), ref[4]) and torch.equal(R[:4], ref[2]) and torch.equal(best[:4], ref[1])


def test_argument_errors_raise_before_a_launch():
    E, x0, x1, offsets, mask = C.ragged_batch()
    with pytest.raises(GimHipError):
        ops.recover_pose(d(E.astype(np.float32)), d(x0), d(x1), offsets=d(offsets))
    with pytest.raises(GimHipError):
        ops.recover_pose(d(E), d(x0), d(x1))                                                         # [B,3,3] without offsets
    with pytest.raises(GimHipError):
        ops.recover_pose(d(E[0]), d(x0), d(x1[:10]))
    with pytest.raises(GimHipError):
        ops.recover_pose(d(E[0]), d(x0), d(x1), mask=d(mask[:10]))
    with pytest.raises(GimHipError):
        ops.recover_pose(d(E[0]), d(x0), d(x1), mask=d(mask.astype(np.int32)))
    with pytest.raises(GimHipError):
        ops.recover_pose(d(E), d(x0), d(x1), offsets=d(np.array([0, 300, 200, 557, 621], dtype=np.int32)))
    with pytest.raises(GimHipError):
        ops.recover_pose(torch.from_numpy(E[0].copy()), d(x0), d(x1))                                # host memory
    out = ops.recover_pose(torch.empty(0, 3, 3, dtype=torch.float64, device=DEV), d(x0[:0]), d(x1[:0]), offsets=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert out[0].shape == (0, 4) and out[4].shape == (0,)


# ---- through zeb --------------------------------------------------------------------------------------------------------------------
def _same_result(dev, host, exact=False):
    assert (dev is None) == (host is None)
    if dev is not None:
        assert np.array_equal(dev[2], host[2]) and dev[2].dtype == bool                              # the RANSAC mask
        if exact:
            assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
        else:
            dR, dt = float(np.abs(dev[0] - host[0]).max()), float(np.abs(dev[1] - host[1]).max())
            print(f"|dR| {dR:.3e} |dt| {dt:.3e}")
            assert dR <= C.RT_BAR and dt <= C.RT_BAR


@pytest.mark.parametrize("solve,sampler", [("device", "device"), ("device", "host"), ("device", "philox"), ("host", "host"), ("host", "philox")])
def test_estimate_pose_recover_device_agrees_with_host(monkeypatch, solve, sampler):
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    some = 0
    for pair in C.ransac_pairs():
        dev = zeb.estimate_pose(*pair, device=DEV, solve=solve, sampler=sampler, recover="device")
        host = zeb.estimate_pose(*pair, device=DEV, solve=solve, sampler=sampler, recover="host")
        _same_result(dev, host)
        some += dev is not None
    assert some >= 2
    one = zeb.device_estimator(DEV, solve=solve, sampler=sampler, recover="device")
    _same_result(one(*C.ransac_pairs()[0]), zeb.estimate_pose(*C.ransac_pairs()[0], device=DEV, solve=solve, sampler=sampler, recover="device"), exact=True)


@pytest.mark.parametrize("solve,sampler", [("device", "device"), ("device", "host"), ("host", "host")])
def test_batch_estimator_equals_the_single_calls(monkeypatch, solve, sampler):
    """a batch with a pair of fewer than five matches and (solve="device": the solver refuses coincident points) a pair with no model"""
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    pairs = C.ransac_pairs()
    many = zeb.device_batch_estimator(DEV, solve=solve, sampler=sampler, recover="device")(pairs)
    assert len(many) == 4 and many[0] is not None and many[1] is not None and many[2] is None
    if solve == "device":
        assert many[3] is None
    for pair, got in zip(pairs, many):
        _same_result(got, zeb.estimate_pose(*pair, device=DEV, solve=solve, sampler=sampler, recover="device"), exact=True)
    assert zeb.device_batch_estimator(DEV, solve=solve, sampler=sampler, recover="device")([]) == []


def test_a_pair_without_a_model_launches_no_recover(monkeypatch):
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    calls = []
    real = ops.recover_pose
    monkeypatch.setattr(ops, "recover_pose", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    pairs = C.ransac_pairs()
    for solve, sampler in (("device", "device"), ("device", "host"), ("host", "host")):
        assert zeb.estimate_pose(*pairs[2], device=DEV, solve=solve, sampler=sampler, recover="device") is None      # four matches
        assert zeb.device_batch_estimator(DEV, solve=solve, sampler=sampler, recover="device")([pairs[2], pairs[2]]) == [None, None]
    for sampler in ("device", "host"):
        assert zeb.estimate_pose(*pairs[3], device=DEV, solve="device", sampler=sampler, recover="device") is None   # no model
        assert zeb.device_batch_estimator(DEV, solve="device", sampler=sampler, recover="device")([pairs[3], pairs[2]]) == [None, None]
    assert not calls
    assert zeb.estimate_pose(*pairs[1], device=DEV, solve="device", sampler="device", recover="device") is not None
    assert len(calls) == 1
    zeb.device_batch_estimator(DEV, solve="device", sampler="device", recover="device")(pairs)
    assert len(calls) == 2                                                                            # one launch for the batch
