"""Video pseudo-labels on the device: ops.label_link / ops.label_pack (csrc/label_link.hip) against the dict / set oracle of
tests/label_link_oracle.py and numpy, video_labels.link / propagate with a device against their numpy paths, and label_pair on a
seeded two-view scene.  Every comparison is exact.  Inputs: tests/label_link_cases.py."""
import numpy as np
import pytest
import torch

import fundamental_cases as F
import label_link_cases as C
import label_link_oracle as O
from gim_amd import ops, pose
from gim_amd import video_labels as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_FILL, IJ_FILL = 0x7FC0DEAD, -7            # what the output buffers hold before a call: a NaN pattern no input has, an impossible row


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the cases are frozen


def _buffers(n):
    out = torch.full((n, 4), OUT_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
    return out, torch.full((n, 2), IJ_FILL, dtype=torch.int32, device=DEV)


def _link(case, ws):
    """one link on the device -> (out bits [N,4], ij [N,2], count, dropped [2]); the workspace is all zero afterwards"""
    out, ij = _buffers(len(case.lab0))
    got = ops.label_link(_up(case.lab0), _up(case.lab1), case.width, case.height, workspace=ws, out=out, ij=ij)
    assert got[0] is out and got[1] is ij and got[2].shape == (1,) and got[3].shape == (1, 2)
    assert int(torch.count_nonzero(ws).item()) == 0, case.name
    return _bits(out.cpu().numpy()), ij.cpu().numpy(), int(got[2].item()), got[3].cpu().numpy()[0]


def _expect(lab0, lab1, i, j, n_rows):
    """the buffers a link must leave: the joined rows in front, the fill behind"""
    out = np.full((n_rows, 4), OUT_FILL, dtype=np.uint32)
    ij = np.full((n_rows, 2), IJ_FILL, dtype=np.int32)
    out[:len(i)] = _bits(np.concatenate([lab0[i, :2], lab1[j, 2:]], 1))
    ij[:len(i)] = np.stack([i, j], 1)
    return out, ij


def _check(case, ws):
    out, ij, count, dropped = _link(case, ws)
    i, j = O.link_ij(case.lab0, case.lab1, case.width)
    want_out, want_ij = _expect(case.lab0, case.lab1, i, j, len(case.lab0))
    assert count == len(i) and dropped.tolist() == [0, 0], (case.name, count, len(i), dropped)
    assert np.array_equal(ij, want_ij) and np.array_equal(out, want_out), case.name
    return out, ij, count


@pytest.fixture(scope="module")
def ws_small():
    return ops.label_link_workspace(1, ops.label_link_max_keys(*C.SMALL), DEV)


def test_link_equals_the_oracle_around_the_workgroup_and_chunk_edges(ws_small):
    joined = 0
    for n in C.SIZES:
        for m in C.SIZES:
            joined += _check(C.random_case(n, m), ws_small)[2]
    assert joined > 5000
    again = _check(C.random_case(1000, 257), ws_small)                        # the same workspace, the same answer
    first = _check(C.random_case(1000, 257), ops.label_link_workspace(1, ops.label_link_max_keys(*C.SMALL), DEV))
    assert all(np.array_equal(a, b) for a, b in zip(again[:2], first[:2])) and again[2] == first[2]


def test_link_at_the_labellers_frame_size():
    ws = ops.label_link_workspace(1, ops.label_link_max_keys(*C.FULL), DEV)
    assert ws.numel() == 2 * (1920 * 1081 + 1)
    assert _check(C.random_case(3000, 2500, C.FULL), ws)[2] > 500
    # without a workspace of the caller's, and without buffers: the wrapper allocates them
    c = C.random_case(257, 255)
    out, ij, count, dropped = ops.label_link(_up(c.lab0), _up(c.lab1), c.width, c.height)
    i, j = O.link_ij(c.lab0, c.lab1, c.width)
    assert int(count.item()) == len(i) and np.array_equal(ij[:len(i)].cpu().numpy(), np.stack([i, j], 1)) and not dropped.any().item()


@pytest.mark.parametrize("case", [C.one_key_case(), C.alias_case(), C.half_integer_case(), C.no_shared_case()], ids=lambda c: c.name)
def test_link_special_cases(case, ws_small):
    count = _check(case, ws_small)[2]
    assert (count == 0) == (case.name == "no-shared")


def test_unusable_keys_are_dropped_and_counted(ws_small):
    c, ok0, ok1 = C.dropped_case()
    out, ij, count, dropped = _link(c, ws_small)
    i, j = O.link_ij(c.lab0[ok0], c.lab1[ok1], c.width)
    i, j = np.flatnonzero(ok0)[i], np.flatnonzero(ok1)[j]
    want_out, want_ij = _expect(c.lab0, c.lab1, i, j, len(c.lab0))
    assert dropped.tolist() == [int((~ok0).sum()), int((~ok1).sum())] and count == len(i) > 50
    assert np.array_equal(ij, want_ij) and np.array_equal(out, want_out)


def test_ragged_batch_equals_the_single_calls():
    other = (64, 40)
    cases = [C.random_case(257, 255), C.random_case(0, 10), C.no_shared_case(), C.random_case(1000, 900), C.random_case(300, 4097, other)]
    B = len(cases)
    widths, heights = [c.width for c in cases], [c.height for c in cases]
    max_keys = ops.label_link_max_keys(widths, heights)
    assert max_keys == 96 * 55 + 1
    ws1, wsB = ops.label_link_workspace(1, max_keys, DEV), ops.label_link_workspace(B, max_keys, DEV)
    singles = [_link(c, ws1) for c in cases]
    off0 = np.concatenate([[0], np.cumsum([len(c.lab0) for c in cases])]).astype(np.int32)
    off1 = np.concatenate([[0], np.cumsum([len(c.lab1) for c in cases])]).astype(np.int32)
    lab0, lab1 = np.concatenate([c.lab0 for c in cases]), np.concatenate([c.lab1 for c in cases])
    for pad in (0, 5):                                            # pad: rows behind the last link, which belong to no link
        lab0p = np.concatenate([lab0, np.full((pad, 4), 3.0, dtype=np.float32)])
        out, ij = _buffers(len(lab0p))
        got = ops.label_link(_up(lab0p), _up(lab1), widths, heights, offsets0=_up(off0), offsets1=off1.tolist(), workspace=wsB, out=out, ij=ij)
        assert int(torch.count_nonzero(wsB).item()) == 0
        out, ij, count, dropped = _bits(out.cpu().numpy()), ij.cpu().numpy(), got[2].cpu().numpy(), got[3].cpu().numpy()
        assert not dropped.any() and count[1] == 0 and count[2] == 0 and count[0] > 0 and count[3] > 0 and count[4] > 0
        for b, (s_out, s_ij, s_count, _) in enumerate(singles):
            assert count[b] == s_count, b
            assert np.array_equal(out[off0[b]:off0[b + 1]], s_out) and np.array_equal(ij[off0[b]:off0[b + 1]], s_ij), b
        assert (out[off0[-1]:] == OUT_FILL).all() and (ij[off0[-1]:] == IJ_FILL).all()
    with pytest.raises(ValueError):
        ops.label_link(_up(lab0), _up(lab1), widths[:2], heights[:2], offsets0=off0.tolist(), offsets1=off1.tolist())


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 4097])
def test_label_pack_equals_numpy(n):
    k0, k1, keep = C.pack_case(n)
    d0, d1 = _up(k0).reshape(n, 2), _up(k1).reshape(n, 2)
    for kp in (None, keep):
        for affine in (None, C.AFFINE):
            for thr in (0.0, 1.0):
                want = V.label_pack_np(k0, k1, keep=kp, moved_thr=thr, affine=affine, vratio=C.VRATIO)
                buf = _buffers(n)[0]
                out, count = ops.label_pack(d0, d1, keep=None if kp is None else _up(kp), moved_thr=thr, affine=affine, vratio=C.VRATIO, out=buf)
                got = _bits(out.cpu().numpy())
                assert int(count.item()) == len(want), (n, kp is None, affine is None, thr)
                assert np.array_equal(got[:len(want)], _bits(want)) and (got[len(want):] == OUT_FILL).all(), (n, kp is None, affine is None, thr)
    if n > 2:                                                     # the NaN row counts as moved; static rows and kept-out rows leave
        assert np.isnan(V.label_pack_np(k0, k1, moved_thr=1.0)).any()
        assert 0 < len(V.label_pack_np(k0, k1, keep=keep, moved_thr=1.0)) < len(V.label_pack_np(k0, k1, moved_thr=1.0)) < n


def test_link_and_propagate_on_the_device_equal_the_host_paths():
    w, h = C.SMALL
    c = C.random_case(257, 255)
    n = len(O.link_ij(c.lab0, c.lab1, c.width)[0])
    assert V.link(c.lab0, c.lab1, w, h, n + 1, device=DEV) is None and V.link(c.lab0, c.lab1, w, h, n + 1) is None
    got = V.link(c.lab0, c.lab1, w, h, n, device=DEV)
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(V.link(c.lab0, c.lab1, w, h, n)))
    host, dev = C.video_store(), C.video_store()
    labels = nones = 0
    for idx0, idx1, skips in C.PROPAGATE_REQUESTS:
        want = V.propagate(host, idx0, idx1, skips, width=w, height=h, min_final_matches=C.VIDEO_MIN_FINAL)
        got = V.propagate(dev, idx0, idx1, skips, width=w, height=h, min_final_matches=C.VIDEO_MIN_FINAL, device=DEV)
        assert got[1:] == want[1:], (idx0, idx1, skips)
        if want[0] is None:
            nones += 1
            assert got[0] is None
        else:
            labels += 1
            assert got[0].is_cuda and np.array_equal(_bits(got[0].cpu().numpy()), _bits(want[0]))
    assert labels >= 6 and nones >= 2
    assert V.propagate(dev, 0, 12, C.VIDEO_SKIPS, width=w, height=h, min_final_matches=C.VIDEO_MIN_FINAL, device=DEV)[1:] == (0, 9)


def test_label_pair_on_a_two_view_scene(monkeypatch):
    k0, k1, static = C.pair_scene()
    kw = dict(threshold=0.5, confidence=0.999999, max_iters=10000, seed=0)
    moved = V.label_pack_np(k0, k1, moved_thr=1.0)
    assert len(moved) == int((~static).sum()) == 300              # the 50 watermark rows leave, nothing else does
    Fm, mask = pose.find_fundamental_mat(moved[:, :2].astype(np.float64), moved[:, 2:].astype(np.float64), threshold=0.5, prob=0.999999,
                                         max_iters=10000, seed=0, device=DEV, solve="device", sampler="device")
    assert Fm is not None and 200 <= mask.sum() <= 230
    # plain coordinates: no watermark row survives, every row is an inlier of the model (Sampson, fp64; 1e-9: the kernel's rounding)
    plain = V.label_pair({"mkpts0_f": _up(k0), "mkpts1_f": _up(k1)}, device=DEV, **kw)
    assert plain.is_cuda and plain.dtype == torch.float32
    rows = plain.cpu().numpy()
    assert np.array_equal(_bits(rows), _bits(V.label_pack_np(moved[:, :2], moved[:, 2:], keep=mask)))
    assert not ((np.abs(rows[:, :2] - rows[:, 2:]) < 1).all(1)).any()
    err = F.sampson(Fm, rows[:, :2].astype(np.float64), rows[:, 2:].astype(np.float64))
    assert len(rows) == mask.sum() and (err <= 0.25 * (1 + 1e-9)).all()
    # the rescale of a resized labelling run; arrays in place of tensors
    scaled = V.label_pair((k0, k1), device=DEV, affine=C.AFFINE, vratio=C.VRATIO, **kw)
    want = V.label_pack_np(moved[:, :2], moved[:, 2:], keep=mask, affine=C.AFFINE, vratio=C.VRATIO)
    assert np.array_equal(_bits(scaled.cpu().numpy()), _bits(want))
    # six moving matches (and watermarks): an empty label after ONE label_pack launch
    calls = []
    real = ops.label_pack
    monkeypatch.setattr(ops, "label_pack", lambda *a, **k: calls.append(1) or real(*a, **k))
    six = np.concatenate([np.flatnonzero(~static)[:6], np.flatnonzero(static)])
    empty = V.label_pair((k0[six], k1[six]), device=DEV, **kw)
    assert empty.shape == (0, 4) and empty.is_cuda and len(calls) == 1
    assert V.label_pair((k0[six[:7]], k1[six[:7]]), device=DEV, **kw).shape == (0, 4) and len(calls) == 2
