"""Case builders and plain references of the sparse head's edge tests (test_sparse_head_cases_cpu.py, test_gpu_sparse_head_edges.py):
SuperPoint's selection tail (sp_nms / sp_topk / sp_sample_desc) and LightGlue's assignment (lg_assign / lg_log_assignment /
lg_emit_matches).  CPU only; every case is seeded, built once and left unchanged (_CACHE).

topk_reference     what select_keypoints (superpoint.py:260-300) gives, with the one thing torch.topk leaves open -- the order of equal
                   scores -- fixed to the kernel's documented rule: lower flat index first (numpy.lexsort).
assign_reference   O.log_assignment + O.filter_matches in float64 on the same fp32 descriptors, arg-max = the LOWEST index among the
                   entries within TIE_EPS of the maximum, plus what a test needs to know which indices fp32 arithmetic may not
                   decide: the size of that tie group and its gap to the best entry outside it, per row and per column.

Assignment cases (ASSIGN): `_assign_inputs` of test_gpu_lightglue.py (random descriptors, half of min(M, N) planted, final_proj x 0.1)
unless noted.  (B, M, N):
  ragged_129_127  (3,129,127)   one past / one short of the 128 tile on the two sides, B > 1
  ragged_257_64   (2,257,64)    three row tiles, half a column tile
  filter_1100     (2,1100,1030) second 1024-round of the filter 76 rows full; rows planted on both sides of row 1024
  m1_n5, m5_n1, m1_n1, m1_n130  (1,1,5) (1,5,1) (1,1,1) (2,1,130)   nothing planted
  ties_cols       (2,200,260)   ~20 column pairs j < j' of image 1 made bit-identical (descriptor and final_proj row), j planted:
                                pairs inside one 128-tile, across tiles, and with j' in the ragged last tile (256..259)
  ties_rows       (2,260,200)   the same construction transposed: duplicate rows of image 0
  empty_middle    (3,150,140)   pair 1: unrelated descriptors pushed down the matchability direction (sigmoid(z) ~ 1e-5), so that no
                                score of it reaches the threshold 0.1 while its arg-maxima stay as decided as anyone's
  no_match        (2,140,150)   threshold 1.0
  thr_zero        (2,140,150)   threshold 0.0: every mutual pair is valid
  unscaled        (2,300,170)   O.planted_descriptors, final_proj as the model has it (40 I + w): the peaked regime, mscores near 1
  base_*                        the three inputs of the existing test_lg_assign (for the reference-vs-oracle check)
"""
import numpy as np
import torch
import torch.nn.functional as F

import lightglue_oracle as O

TIE_EPS = 1e-9      # log units: entries this close to the maximum form its tie group
LOW_GAP = 1e-3      # log units: below this gap an index is not pinned (fp32 scores are good to ~1e-5 near the maximum)
LAYER = 8
_CACHE = {}


# ------------------------------------------------------------------------------------------------ sp_topk
def topk_reference(scores, thr, k):
    """scores [B,H,W] -> per image (kpts [n,2] float32 (x, y), scores [n] float32), and nvalid (list of n).  Candidates: scores > thr;
    more than k of them: the first k by (score descending, flat index ascending); else all of them in flat-index order."""
    s = scores.detach().cpu().numpy().astype(np.float32)
    B, H, W = s.shape
    kpts, sc, nvalid = [], [], []
    for b in range(B):
        flat = s[b].reshape(-1)
        idx = np.nonzero(flat > np.float32(thr))[0]
        if len(idx) > k:
            order = np.lexsort((idx, -flat[idx].astype(np.float64)))[:k]     # last key is the primary one
            idx = idx[order]
        kpts.append(torch.from_numpy(np.stack([idx % W, idx // W], -1).astype(np.float32)))
        sc.append(torch.from_numpy(flat[idx].copy()))
        nvalid.append(len(idx))
    return kpts, sc, nvalid


def distinct_map(B, H, W, seed):
    """every pixel a different positive value in (0, 1), another permutation per image"""
    g = torch.Generator().manual_seed(seed)
    hw = H * W
    return torch.stack([(torch.randperm(hw, generator=g) + 1).float() / (hw + 1) for _ in range(B)]).view(B, H, W)


def quantised_map(B, H, W, seed, levels=16):
    """distinct_map rounded up to `levels` equal levels: H*W / levels pixels share each value, scattered over the whole map"""
    return torch.ceil(distinct_map(B, H, W, seed) * levels) / levels


def sparse_map(B, H, W, n, seed):
    """zeros but for exactly n distinct positive pixels per image, at seeded positions"""
    g = torch.Generator().manual_seed(seed)
    s = torch.zeros(B, H * W)
    for b in range(B):
        pos = torch.randperm(H * W, generator=g)[:n]
        s[b, pos] = (torch.randperm(n, generator=g) + 1).float() / (n + 1)
    return s.view(B, H, W)


def threshold_map(thr, seed):
    """96x64 map (two candidate workgroups) of pixels exactly at thr, one ulp above, one ulp below, and zeros"""
    g = torch.Generator().manual_seed(seed)
    t = np.float32(thr)
    vals = torch.tensor([float(t), float(np.nextafter(t, np.float32(1))), float(np.nextafter(t, np.float32(0))), 0.0])
    return vals[torch.randint(0, 4, (2, 96, 64), generator=g)], float(vals[1])


def smooth_map(B, H, W, seed):
    """_score_map of test_gpu_lightglue.py (3x3-averaged noise: maxima spaced like real score maps), another content per image, with
    constant plateaus -- equal neighbours both survive (superpoint.py:63) -- across the NMS tile borders x = 64 and y = 16 where the
    map reaches them"""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(B, H, W, generator=g) * 0.05
    s = F.avg_pool2d(s[:, None], 3, 1, 1)[:, 0].contiguous()
    s[:, 14:18, 60:68] = 0.04          # clipped by the map where it is smaller
    s[0, 2:4, 62:66] = 0.045
    s[-1, 15:17, 5:9] = 0.045
    return s


# ------------------------------------------------------------------------------------------------ lg_assign
def assign_reference(sd, layer, d0, d1, th, dup=None):
    """O.log_assignment + O.filter_matches in float64.  dup: [(side, b, src, dst)] -- rows made identical by the builder; their float64
    final_proj rows and matchability logits are copied the same way, so that the reference sees the duplicates the kernel sees.
    -> dict: scores [B,M+1,N+1], m0 / m1 (int64, -1 = none), ms0 / ms1, arg0 / arg1 (the arg-maxima), size0 / size1 (entries within
    TIE_EPS of the maximum), gap0 / gap1 (maximum minus the best entry outside that group; inf when there is none)"""
    p = f"log_assignment.{layer}"
    W, bias = sd[p + ".final_proj.weight"].double(), sd[p + ".final_proj.bias"].double()
    wz, bz = sd[p + ".matchability.weight"].double(), sd[p + ".matchability.bias"].double()
    x0, x1 = d0.double(), d1.double()
    d = x0.shape[-1]
    md = [F.linear(x0, W, bias) / d ** 0.25, F.linear(x1, W, bias) / d ** 0.25]
    z = [F.linear(x0, wz, bz).squeeze(-1), F.linear(x1, wz, bz).squeeze(-1)]
    for side, b, src, dst in dup or ():
        md[side][b, dst] = md[side][b, src]
        z[side][b, dst] = z[side][b, src]
    sim = torch.einsum("bmd,bnd->bmn", md[0], md[1])
    B, M, N = sim.shape
    core = (F.log_softmax(sim, 2) + F.log_softmax(sim, 1)) + (F.logsigmoid(z[0])[:, :, None] + F.logsigmoid(z[1])[:, None, :])
    scores = sim.new_zeros(B, M + 1, N + 1)
    scores[:, :M, :N] = core
    scores[:, :M, N] = F.logsigmoid(-z[0])
    scores[:, M, :N] = F.logsigmoid(-z[1])
    c = core.numpy()

    def best(axis):
        mx = c.max(axis, keepdims=True)
        grp = c >= mx - TIE_EPS
        arg = grp.argmax(axis)                                   # numpy: the first (lowest) index of the group
        rest = np.where(grp, -np.inf, c).max(axis)
        return mx.squeeze(axis), arg, grp.sum(axis), mx.squeeze(axis) - rest

    max0, arg0, size0, gap0 = best(2)
    _, arg1, size1, gap1 = best(1)
    i0, i1 = np.arange(M)[None], np.arange(N)[None]
    mutual0 = np.take_along_axis(arg1, arg0, 1) == i0
    mutual1 = np.take_along_axis(arg0, arg1, 1) == i1
    ms0 = np.where(mutual0, np.exp(max0), 0.0)
    ms1 = np.where(mutual1, np.take_along_axis(ms0, arg1, 1), 0.0)
    valid0 = mutual0 & (ms0 > th)
    valid1 = mutual1 & np.take_along_axis(valid0, arg1, 1)
    t = torch.from_numpy
    return {"scores": scores, "m0": t(np.where(valid0, arg0, -1)), "m1": t(np.where(valid1, arg1, -1)), "ms0": t(ms0), "ms1": t(ms1),
            "arg0": t(arg0), "arg1": t(arg1), "size0": t(size0), "size1": t(size1), "gap0": t(gap0), "gap1": t(gap1)}


def low_gap(ref):
    """(rows, columns) whose arg-max the reference does not pin: gap below LOW_GAP"""
    return ref["gap0"] < LOW_GAP, ref["gap1"] < LOW_GAP


def exempt(ref):
    """(rows, columns) whose matches0 / matches1 entry a test may leave open: their own arg-max is low-gap, or the one of the column
    (row) it points at, which decides `mutual`.  Everything else must equal the reference."""
    lg0, lg1 = low_gap(ref)
    return lg0 | lg1.gather(1, ref["arg0"]), lg1 | lg0.gather(1, ref["arg1"])


def _state(scale):
    _, lg = O.make_state_dicts(0)
    p = f"log_assignment.{LAYER}"
    if scale != 1.0:
        lg[p + ".final_proj.weight"] = lg[p + ".final_proj.weight"] * scale
    return lg


def _planted(B, M, N, seed, rows=None):
    """_assign_inputs of test_gpu_lightglue.py; rows: the rows of image 0 that get a correspondence (default: the first min(M, N) // 2)"""
    g = torch.Generator().manual_seed(seed)
    d0 = torch.randn(B, M, 256, generator=g)
    d1 = torch.randn(B, N, 256, generator=g)
    rows = torch.arange(min(M, N) // 2) if rows is None else rows
    nm = len(rows)
    cols = []
    for b in range(B):
        perm = torch.randperm(N, generator=g)[:nm]
        d1[b, perm] = d0[b, rows] + 0.05 * torch.randn(nm, 256, generator=g)
        cols.append(perm)
    return d0, d1, cols


def _dup_pairs(planted, N):
    """column pairs (j, j'), j < j', j a planted column, no column in two pairs: 3 inside tile 0, 2 inside tile 1, 3 from tile 0 into
    tile 1, and as many as the ragged last tile [256, N) has columns with j' there (j from tile 0 and 1 in turn)"""
    planted = sorted(int(c) for c in planted)
    used, pairs = set(), []

    def src(lo, hi):
        return next(c for c in planted if lo <= c < hi and c not in used)

    def add(j, lo, hi):
        jj = next(c for c in range(max(lo, j + 1), hi) if c not in used)
        used.update((j, jj))
        pairs.append((j, jj))

    for c in range(256, N):
        used.add(c)                      # kept for the ragged pairs
    for _ in range(3):
        add(src(0, 100), 0, 128)
    for _ in range(2):
        add(src(128, 230), 128, 256)
    for _ in range(3):
        add(src(0, 128), 128, 256)
    for n, c in enumerate(range(256, N)):
        j = src(0, 128) if n % 2 == 0 else src(128, 256)
        used.update((j,))
        pairs.append((j, c))
    return pairs


ASSIGN = {
    "ragged_129_127": dict(B=3, M=129, N=127, seed=21, th=0.1, rich=True),
    "ragged_257_64": dict(B=2, M=257, N=64, seed=22, th=0.1, rich=True),
    "filter_1100": dict(B=2, M=1100, N=1030, seed=23, th=0.1, rich=True),
    "m1_n5": dict(B=1, M=1, N=5, seed=24, th=0.1),
    "m5_n1": dict(B=1, M=5, N=1, seed=25, th=0.1),
    "m1_n1": dict(B=1, M=1, N=1, seed=26, th=0.1),
    "m1_n130": dict(B=2, M=1, N=130, seed=27, th=0.1),
    "ties_cols": dict(B=2, M=200, N=260, seed=28, th=0.1, rich=True),
    "ties_rows": dict(B=2, M=260, N=200, seed=29, th=0.1, rich=True),
    "empty_middle": dict(B=3, M=150, N=140, seed=30, th=0.1, rich=True),
    "no_match": dict(B=2, M=140, N=150, seed=31, th=1.0, none=True),
    "thr_zero": dict(B=2, M=140, N=150, seed=31, th=0.0, rich=True),
    "unscaled": dict(B=2, M=300, N=170, seed=33, th=0.1, rich=True, scale=1.0),
    "base_128": dict(B=2, M=128, N=128, seed=10, th=0.1, rich=True),
    "base_300_170": dict(B=1, M=300, N=170, seed=10, th=0.1, rich=True),
    "base_2048": dict(B=2, M=2048, N=2048, seed=10, th=0.1, rich=True),
}
EDGE_CASES = [k for k in ASSIGN if not k.startswith("base_")]


def assign_case(name):
    """-> dict: the ASSIGN entry + sd (LightGlue state dict, final_proj scaled), d0 / d1 (fp32), md0 / md1 (fp32 final_proj outputs,
    what the kernel takes), dup"""
    key = ("case", name)
    if key in _CACHE:
        return _CACHE[key]
    c = dict(ASSIGN[name])
    B, M, N, seed = c["B"], c["M"], c["N"], c["seed"]
    sd = _state(c.get("scale", 0.1))
    p = f"log_assignment.{LAYER}"
    dup = []
    if name == "unscaled":
        _, d0, _, d1 = O.planted_descriptors(B, M, seed=seed)
        d1 = d1[:, :N].contiguous()
    elif name in ("ties_cols", "ties_rows"):
        d0, d1, cols = _planted(B, 200, 260, seed)
        for b in range(B):
            dup += [(1, b, j, jj) for j, jj in _dup_pairs(cols[b], 260)]
        if name == "ties_rows":
            d0, d1 = d1, d0
            dup = [(0, b, j, jj) for _, b, j, jj in dup]
    elif name == "filter_1100":
        d0, d1, _ = _planted(B, M, N, seed, rows=torch.cat([torch.arange(400), torch.arange(990, 1100)]))
    else:
        d0, d1, _ = _planted(B, M, N, seed)
    if name == "empty_middle":
        # pair 1: unrelated descriptors, moved along -w so that z = w . d + b ~ -12: no score of the pair can pass 0.1
        g = torch.Generator().manual_seed(seed + 1000)
        w = sd[p + ".matchability.weight"].reshape(-1)
        shift = -(15.0 / w.dot(w)) * w
        d0[1] = torch.randn(M, 256, generator=g) + shift
        d1[1] = torch.randn(N, 256, generator=g) + shift
    md0 = F.linear(d0, sd[p + ".final_proj.weight"], sd[p + ".final_proj.bias"])
    md1 = F.linear(d1, sd[p + ".final_proj.weight"], sd[p + ".final_proj.bias"])
    for side, b, j, jj in dup:            # bit for bit: the descriptor and its final_proj row
        (d0, d1)[side][b, jj] = (d0, d1)[side][b, j]
        (md0, md1)[side][b, jj] = (md0, md1)[side][b, j]
    assert d0.shape == (B, M, 256) and d1.shape == (B, N, 256)
    c.update(name=name, sd=sd, d0=d0, d1=d1, md0=md0.contiguous(), md1=md1.contiguous(), dup=dup)
    _CACHE[key] = c
    return c


def assign_ref(name):
    """assign_reference of the case, computed once"""
    key = ("ref", name)
    if key not in _CACHE:
        c = assign_case(name)
        _CACHE[key] = assign_reference(c["sd"], LAYER, c["d0"], c["d1"], c["th"], c["dup"])
    return _CACHE[key]


def emit_inputs(c):
    """keypoints and per-pair scales of the adapter leg of lg_emit_matches"""
    g = torch.Generator().manual_seed(c["seed"] + 500)
    B, M, N = c["B"], c["M"], c["N"]
    kp0, kp1 = torch.rand(B, M, 2, generator=g) * 600, torch.rand(B, N, 2, generator=g) * 600
    sc0 = torch.tensor([[1.5, 2.0], [0.75, 1.25], [3.0, 0.5]])[:B].contiguous()
    sc1 = torch.tensor([[0.5, 1.25], [2.0, 1.0], [1.5, 0.25]])[:B].contiguous()
    return kp0, kp1, sc0, sc1


def expected_lists(m0, ms0, kp0, kp1, sc0, sc1):
    """the packed lists of lg_emit_matches from matches0 / matching_scores0 [B,M] (torch.where order): matches [T,2], scores, mkpts0,
    mkpts1, m_bids"""
    B = m0.shape[0]
    rows = [torch.where(m0[b] > -1)[0] for b in range(B)]
    matches = torch.cat([torch.stack([rows[b], m0[b][rows[b]]], -1) for b in range(B)])
    scores = torch.cat([ms0[b][rows[b]] for b in range(B)])
    mk0 = torch.cat([kp0[b][rows[b]] * sc0[b] for b in range(B)])
    mk1 = torch.cat([kp1[b][m0[b][rows[b]]] * sc1[b] for b in range(B)])
    bids = torch.cat([torch.full((len(rows[b]),), b, dtype=torch.int64) for b in range(B)])
    return matches, scores, mk0, mk1, bids


def sample_desc_keypoints(B, K, h, w, seed):
    """[B,K,2] integer pixel positions of an (8h x 8w) image: the four corners, points along the last row and the last column, the
    rest seeded"""
    g = torch.Generator().manual_seed(seed)
    W8, H8 = 8 * w, 8 * h
    kp = torch.stack([torch.randint(0, W8, (B, K), generator=g), torch.randint(0, H8, (B, K), generator=g)], -1).float()
    fixed = [(0, 0), (W8 - 1, 0), (0, H8 - 1), (W8 - 1, H8 - 1)]
    fixed += [(x, H8 - 1) for x in range(1, W8 - 1, max(1, W8 // 7))] + [(W8 - 1, y) for y in range(1, H8 - 1, max(1, H8 // 7))]
    assert len(fixed) < K
    for b in range(B):
        for n, xy in enumerate(fixed):
            kp[b, (n + 5 * b) % K] = torch.tensor(xy, dtype=torch.float32)   # another slot per image
    kp[B - 1, K - 1] = torch.tensor([W8 - 1.0, H8 - 1.0])                    # the last wave of the launch
    return kp


# sp_topk cases shared by the CPU and the GPU tests: 96 x 160 = 15360 pixels = 4 candidate workgroups of 4096 pixels (the last: 3072)
TOPK_HW = (96, 160)
CAND_PPB = 4096          # pixels per candidate workgroup (superpoint.hip)
TIE_K = 3 * 960 + 500    # quantised_map: 960 pixels per level; three whole levels, then 500 of the fourth
FEW_N = 37               # sparse_map: candidates of the `few` switch cases
THR = 0.015625           # 2^-6: exact in fp32
