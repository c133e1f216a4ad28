"""Frame preparation on the device: ops.frame_prep (csrc/frame_prep.hip) against frame_prep.frame_prep_np, byte for byte and bit for
bit, on the cases of tests/frame_prep_cases.py; a ragged batch against its single-job calls with guard elements around every output;
every subset of the outputs; the kept counts; the refusals that come before a launch."""
import numpy as np
import pytest
import torch

import frame_prep_cases as C
from gim_amd import frame_prep as fp
from gim_amd import ops
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = C.cases()
FILL = 0xA5                                   # what every output byte holds before a call (fp32: a pattern no output has)
DTYPES = (torch.uint8, torch.uint8, torch.uint8, torch.float32, torch.float32, torch.float32)


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the cases are shared


def _raw(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _same(got, want, what):
    want = np.ascontiguousarray(want)
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    assert _raw(got).tobytes() == want.tobytes(), what


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_output_of_every_case(case):
    want = fp.frame_prep_np(case["frame"], case["seg"], case["exclude"], case["box"], case["size"], case["flags"])
    r = ops.frame_prep(_up(case["frame"][None]), _up(case["seg"][None]), case["exclude"], [(0, case["box"], case["size"], case["flags"])])
    names = [n for k, n in enumerate(fp.OUTPUTS) if case["flags"] & (1 << k)]
    assert sorted(r.plan.views[0]) == sorted(names) and len(names) >= 5
    for name in names:
        _same(r.get(0, name), want[name], (case["name"], name))
    assert r.kept.dtype == torch.int32 and r.kept.tolist() == [want["kept"]]


def _guarded(elems):
    return {name: torch.full((n * (4 if dt == torch.float32 else 1),), FILL, dtype=torch.uint8, device=DEV).view(dt)
            for name, n, dt in zip(fp.OUTPUTS, elems, DTYPES) if n}


def _check_batch(frames, seg, exclude, jobs, guard):
    pl = fp.plan(frames.shape[1:3], jobs, guard=guard)
    bufs = _guarded(pl.elems)
    r = ops.frame_prep(_up(frames), _up(seg), exclude, jobs, buffers=bufs, guard=guard)
    touched = {name: np.zeros(bufs[name].numel() * bufs[name].element_size(), dtype=bool) for name in bufs}
    for j, (slot, box, size, flags) in enumerate(jobs):
        want = fp.frame_prep_np(frames[slot], seg[slot], exclude, box, size, flags)
        assert sorted(r.plan.views[j]) == sorted(n for k, n in enumerate(fp.OUTPUTS) if flags & (1 << k))
        for name, (off, shape) in r.plan.views[j].items():
            _same(r.get(j, name), want[name], (j, name))
            sz = bufs[name].element_size()
            assert not touched[name][off * sz:(off + int(np.prod(shape))) * sz].any()       # ranges do not overlap
            touched[name][off * sz:(off + int(np.prod(shape))) * sz] = True
        assert int(r.kept[j]) == want["kept"], j
    for name in bufs:                                              # every byte outside the jobs' ranges is what it was
        raw = _raw(bufs[name])
        assert (raw[~touched[name]] == FILL).all(), name
        assert (~touched[name]).sum() >= 2 * guard * len([1 for v in r.plan.views if name in v])
    return r


def test_ragged_batch_equals_its_single_jobs_and_stays_inside_its_ranges():
    frames, seg, exclude, jobs = C.ragged_batch()
    assert len(jobs) == 6 and sorted({j[0] for j in jobs}) == [0, 1, 2] and [j[0] for j in jobs].count(1) == 3
    r = _check_batch(frames, seg, exclude, jobs, guard=64)
    # ... and equals the single-job calls of the device
    fd, sd = _up(frames), _up(seg)
    for j, job in enumerate(jobs):
        one = ops.frame_prep(fd, sd, exclude, [job])
        for name in one.plan.views[0]:
            assert torch.equal(one.get(0, name), r.get(j, name)), (j, name)
        assert int(one.kept[0]) == int(r.kept[j])


def test_every_output_subset():
    frames, seg, exclude, _ = C.ragged_batch()
    boxes = [(3, 4, 40, 33), None, (20, 11, 31, 18), (5, 20, 45, 27)]
    jobs = [(s % 3, boxes[s % 4], (16, 8), s | (fp.MASKED if s % 2 else 0)) for s in range(64)]
    _check_batch(frames, seg, exclude, jobs, guard=16)


def test_kept_is_exact_on_many_tiles():
    """a job of 15 x 5 tiles: the count crosses waves, workgroups and the atomics of one job, beside a second job"""
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 90, 1000, 3), dtype=np.uint8)
    seg = rng.integers(0, C.CLASSES, (2, 45, 333), dtype=np.uint8)
    jobs = [(1, (1, 2, 999, 88), (15 * 64 - 3, 5 * 16 - 5), fp.OUT_MASK), (0, None, (80, 24), fp.OUT_MASK8 | fp.OUT_GRAY)]
    r = ops.frame_prep(_up(frames), _up(seg), C.EXCLUDE, jobs)
    for j, (slot, box, size, flags) in enumerate(jobs):
        want = fp.frame_prep_np(frames[slot], seg[slot], C.EXCLUDE, box, size, flags)
        assert int(r.kept[j]) == want["kept"] and 0 < want["kept"] < size[0] * size[1]
        for name in r.plan.views[j]:
            _same(r.get(j, name), want[name], (j, name))


def test_without_class_maps():
    case = CASES[0]
    r = ops.frame_prep(_up(case["frame"][None]), None, None, [(0, case["box"], case["size"], fp.OUT_U8 | fp.OUT_RGB | fp.OUT_NORM)])
    want = fp.frame_prep_np(case["frame"], None, [], case["box"], case["size"], fp.OUT_U8 | fp.OUT_RGB | fp.OUT_NORM)
    assert r.kept is None
    for name in ("u8", "rgb", "norm"):
        _same(r.get(0, name), want[name], name)
    with pytest.raises(GimHipError):
        ops.frame_prep(_up(case["frame"][None]), None, None, [(0, None, (16, 8), fp.OUT_MASK)])


def test_an_empty_batch_launches_nothing_and_refusals_come_before_a_launch(monkeypatch):
    case = CASES[0]
    frames, seg = _up(case["frame"][None]), _up(case["seg"][None])
    frames160 = torch.zeros(1, 40, 160, 3, dtype=torch.uint8, device=DEV)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} must not be called")

    real = ops.lib
    monkeypatch.setattr(ops, "lib", NoLaunch())
    r = ops.frame_prep(frames, seg, C.EXCLUDE, [])
    assert r.buffers == {} and r.kept.shape == (0,)
    for box, size in C.REFUSED:                                    # a factor above 16
        with pytest.raises(GimHipError, match="more than 16"):
            ops.frame_prep(frames160, None, None, [(0, box, size, fp.OUT_U8)])
    for bad in [(1, None, (16, 8), fp.OUT_U8), (0, (0, 0, 51, 40), (16, 8), fp.OUT_U8), (0, None, (12, 8), fp.OUT_MASK8),
                (0, None, (16, 8), 128), (0, None, (0, 8), fp.OUT_U8)]:
        with pytest.raises(GimHipError):
            ops.frame_prep(frames, seg, C.EXCLUDE, [bad])
    with pytest.raises(GimHipError):
        ops.frame_prep(frames.cpu(), seg, C.EXCLUDE, [(0, None, (16, 8), fp.OUT_U8)])
    monkeypatch.setattr(ops, "lib", real)
    # factor 16 exactly is served
    r = ops.frame_prep(frames160, None, None, [(0, (0, 0, 128, 8), (8, 8), fp.OUT_U8)])
    assert int(r.get(0, "u8").sum()) == 0
