"""Coarse matching with real padding masks (the mask branch of csrc/coarse_match.hip: the -INF fill of the similarity tile, the
128 x 128 statistics kernel that 16-bit features take when masks are given, cm_mask_extent_kernel and the border removal measured from
each pair's valid extent) against conf_matrix_dual_softmax + get_coarse_match of oracle/loftr_oracle.py on planted features.

Masks are mixed across the pairs of one call so that the per-pair extents differ: rectangular prefixes (different for the two
images), all valid, an L away from the origin and two diagonal blocks (the reference's extent is the maximum of the column sums / row
sums, coarse_matching.py:36-37, which is neither the bounding box nor the last valid index + 1 there), a pair whose valid extent is
4 x 16 (at most 2 * border_rm rows: no match survives) and a pair whose image 1 is wholly masked (a uniform, finite conf matrix).
16-bit features: the reference is evaluated on the 16-bit-rounded features, so indices are exact and confidences differ by
summation order only.

Before the device comparison every case asserts, on the host, that the oracle finds at least 20 matches and that every
mutual-maximum cell of the oracle's conf matrix lies at least 1e-4 (ten times the confidence bar) from `thr`: the reference alone
decides every match.  The seeds below were picked for that."""
import functools

import pytest
import torch

import loftr_oracle as O

pytestmark = pytest.mark.gpu

THR, BORDER, TEMP, C = 0.2, 2, 0.1, 256
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _rect(h, w, vh, vw):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[:vh, :vw] = True
    return m


def _ell(h, w):
    """an L that does not touch row 0: a bar down the left side from row 2, a bar along the bottom, two columns short of the right edge.
    max of column sums = h - 2 (bounding box from the origin: h), max of row sums = w - 2"""
    m = torch.zeros(h, w, dtype=torch.bool)
    m[2:, :w // 2] = True
    m[h - 5:, :w - 2] = True
    return m


def _blocks(h, w):
    """two blocks on the diagonal: extent (h - h // 2, w - w // 2) by the reference's rule, bounding box (h, w)"""
    m = torch.zeros(h, w, dtype=torch.bool)
    m[:h // 2, :w // 2] = True
    m[h // 2:, w // 2:] = True
    return m


def _mask(kind, h, w):
    if kind == "all":
        return torch.ones(h, w, dtype=torch.bool)
    if kind == "none":
        return torch.zeros(h, w, dtype=torch.bool)
    if kind == "ell":
        return _ell(h, w)
    if kind == "blocks":
        return _blocks(h, w)
    return _rect(h, w, *kind)


# (id, N, hw0, hw1, [(mask of image 0, mask of image 1) per pair], scaled, strided, seed)
CASES = [
    ("3x12x16-rect-all-ell-scaled", 3, (12, 16), (12, 16), [((12, 13), (10, 16)), ("all", "all"), ("ell", (12, 15))], True, False, 31),
    ("3x12x16-blocks-rect-none", 3, (12, 16), (12, 16), [("blocks", "all"), ("all", (12, 14)), ("all", "none")], False, False, 32),
    ("2x15x20-4x16-rect-strided", 2, (15, 20), (15, 20), [((4, 16), (15, 20)), ((13, 20), (15, 17))], False, True, 33),
    ("2x15x20-ell-none", 2, (15, 20), (15, 20), [("ell", "all"), ("all", "none")], False, False, 34),
    ("2x12x16x10x13-rect-none", 2, (12, 16), (10, 13), [((12, 15), (10, 13)), ("all", "none")], False, False, 35),
    ("2x12x16x10x13-ell-all-scaled", 2, (12, 16), (10, 13), [("ell", "all"), ("all", (10, 11))], True, False, 36),
]
EMPTY_PAIRS = {"3x12x16-blocks-rect-none": (2,), "2x15x20-4x16-rect-strided": (0,), "2x15x20-ell-none": (1,), "2x12x16x10x13-rect-none": (1,)}


@functools.lru_cache(maxsize=None)
def _reference(case_id, dt):
    """host side of a case: (f0, f1 in dtype dt, m0, m1 bool [N,h,w], scale0, scale1, conf, oracle dict)"""
    _, N, hw0, hw1, masks, scaled, _, seed = next(c for c in CASES if c[0] == case_id)
    f0, f1, _ = O.planted_coarse_features(N, hw0, sigma=1.0, eps=0.5, seed=seed)
    f1 = f1[:, :hw1[0] * hw1[1]].contiguous()          # L != S: the first S planted partners
    f0, f1 = f0.to(TDT[dt]), f1.to(TDT[dt])
    m0 = torch.stack([_mask(a, *hw0) for a, _ in masks])
    m1 = torch.stack([_mask(b, *hw1) for _, b in masks])
    s0 = s1 = None
    if scaled:
        g = torch.Generator().manual_seed(seed + 1000)
        s0, s1 = 0.5 + 2 * torch.rand(N, 2, generator=g), 0.5 + 2 * torch.rand(N, 2, generator=g)
    conf = O.conf_matrix_dual_softmax(f0.float(), f1.float(), TEMP, m0.flatten(-2), m1.flatten(-2))
    ref = O.get_coarse_match(conf, (hw0[0] * 8, hw0[1] * 8), (hw1[0] * 8, hw1[1] * 8), hw0, hw1, THR, BORDER, s0, s1, m0, m1)
    return f0, f1, m0, m1, s0, s1, conf, ref


def _host_conditions(case_id, dt):
    """the two conditions that make the oracle the judge of every match -> (matches, distance of the nearest mutual maximum from thr)"""
    *_, conf, ref = _reference(case_id, dt)
    mutual = (conf == conf.max(dim=2, keepdim=True)[0]) & (conf == conf.max(dim=1, keepdim=True)[0])
    return ref["b_ids"].numel(), (conf[mutual] - THR).abs().min().item()


def _close(got, ref, tol, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max|err|={err:.3e} scale={scale:.3e} tol={tol}"
    return err / scale


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_coarse_match_with_padding_masks(case, dt):
    from gim_amd import ops
    dev = torch.device("cuda:0")
    case_id, N, hw0, hw1, _, scaled, strided, _ = case
    L, S = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0, f1, m0, m1, s0, s1, conf, ref = _reference(case_id, dt)
    nref, margin = _host_conditions(case_id, dt)
    assert nref >= 20, f"{case_id} {dt}: the oracle finds {nref} matches"
    assert margin >= 1e-4, f"{case_id} {dt}: a mutual maximum lies {margin:.2e} from thr"
    per_pair = torch.bincount(ref["b_ids"], minlength=N).tolist()
    for b in range(N):
        assert (per_pair[b] == 0) == (b in EMPTY_PAIRS.get(case_id, ())), (case_id, per_pair)
    if strided:                                            # [x | other columns] of one buffer, as the token buffers are
        assert L == S
        buf = torch.full((2 * N * L, 2 * C), 7.0, dtype=TDT[dt], device=dev)
        buf[:N * L, :C], buf[N * L:, :C] = f0.reshape(-1, C).to(dev), f1.reshape(-1, C).to(dev)
        d0, d1 = buf[:N * L].view(N, L, 2 * C)[:, :, :C], buf[N * L:].view(N, S, 2 * C)[:, :, :C]
    else:
        d0, d1 = f0.to(dev), f1.to(dev)
    r = ops.coarse_match(d0, d1, hw0, hw1, 8.0, TEMP, THR, BORDER, s0.to(dev) if scaled else None, s1.to(dev) if scaled else None,
                         m0.reshape(N, -1).to(torch.uint8).to(dev).contiguous(), m1.reshape(N, -1).to(torch.uint8).to(dev).contiguous())
    cnt = r.count.cpu()
    M = int(cnt[0])
    assert M == nref, f"M={M} ref={nref}"
    assert int(cnt[1]) == 0                                 # health word: finite similarities, also beside a wholly masked image
    assert cnt[2:].tolist() == per_pair
    for k in ("b_ids", "i_ids", "j_ids"):
        got = getattr(r, k)[:M].cpu()
        assert got.dtype == torch.int64 and torch.equal(got, ref[k]), k
    e_conf = _close(r.mconf[:M], ref["mconf"], 1e-5, "mconf")
    _close(r.mkpts0_c[:M], ref["mkpts0_c"].float(), 1e-6, "mkpts0_c")
    _close(r.mkpts1_c[:M], ref["mkpts1_c"].float(), 1e-6, "mkpts1_c")
    e_cm = _close(ops.coarse_conf_matrix(r), conf, 1e-5, "conf_matrix")
    print(f"[coarse mask] {case_id} {dt}: M={M} per pair {per_pair}, nearest mutual maximum {margin:.1e} from thr; mconf {e_conf:.2e}, "
          f"conf matrix {e_cm:.2e} of scale (bar 1e-5)")
