"""GPU tests of the kernels that took per-sequence lengths for ragged LightGlue batches (gim_sdpa_varlen, gim_lg_transpose_varlen,
gim_lg_assign_ragged, gim_lg_gather_pairs_ragged).  Every launch is compared with the uniform kernel called per sequence at that
sequence's own sizes: a sequence walks the same tiles with the same arithmetic, so the bar is bit equality on the rows that exist,
exact zeros (-1 for matches) on the rows that do not, and nothing written outside the batch.

Capacity 200 (no multiple of 64 or 128, two SDPA query blocks, 2 x 2 assignment tiles); lengths from {0, 1, 5, 63, 64, 65, 127, 128,
129, 199, 200}: both sides of every tile edge, an empty sequence, a full one."""
import functools

import pytest
import torch

import lightglue_oracle as O

pytestmark = pytest.mark.gpu
K = 200
KP = 256   # K rounded up to the 64-key tile
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
LEN_A = [200, 63, 129, 0, 65, 1]      # one table per side: every edge value appears in one of them
LEN_B = [199, 128, 5, 64, 0, 127]
GUARD = 3                             # guard rows in front of and behind every output


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=_dev())


def _guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), 7.0, dtype=dtype, device=_dev())
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf):
    return bool((buf[:GUARD] == 7).all() and (buf[-GUARD:] == 7).all())


# ------------------------------------------------------------------------------------------------ sdpa + transpose
def _sdpa_case(dt, D, cross, poison):
    """nb sequences of capacity K.  Self: q and k/v sequences share their lengths; cross: the stacked [2 B] layout with kv_shift = nb/2,
    sequence s attends to sequence (s + nb/2) % nb.  Returns nothing: asserts."""
    from gim_amd import ops
    dev, H = _dev(), 256 // D
    lens = LEN_A + LEN_B if cross else LEN_A        # cross: image-0 sequences first, then image-1
    nb = len(lens)
    shift = nb // 2 if cross else 0
    g = torch.Generator().manual_seed(11 + D + cross)
    qkv = torch.randn(nb * K, 768, generator=g).to(dev).to(dt)
    if poison:   # what lies behind a sequence's length must never be read: Q and K rows NaN there (V^T: as the varlen transpose wrote it)
        for s, n in enumerate(lens):
            qkv[s * K + n:(s + 1) * K, :512] = float("nan")
    q, k, v = qkv[:, :256], qkv[:, 256:512], qkv[:, 512:]
    ln = _i32(lens)
    vt = torch.full((nb, 256, KP), float("nan"), dtype=dt, device=dev)
    ops.lg_transpose(v, vt, nb, K, KP, 256, ln)
    for s, n in enumerate(lens):
        assert torch.equal(vt[s, :, :n], v[s * K:s * K + n].t()) and not vt[s, :, n:].any(), f"V^T of sequence {s} (len {n})"
    for out_dt in ({dt, torch.float32} if dt != torch.float32 else {dt}):
        buf, out = _guarded(nb * K, 256, out_dt)
        ops.sdpa(q, k, vt, out, nb, H, K, K, KP, kv_shift=shift, D=D, len_q=ln, len_k=ln)
        assert _guards_intact(buf), "rows outside [0, nb*L) were written"
        assert not torch.isnan(out.float()).any()
        for s, nq in enumerate(lens):
            kv = (s + shift) % nb
            nk = lens[kv]
            rows = out[s * K:(s + 1) * K]
            assert not rows[nq:].any(), f"sequence {s}: rows behind len_q={nq} are not zero"
            if nq == 0:
                continue
            if nk == 0:
                assert not rows.any(), f"sequence {s}: len_k = 0 must give zeros"
                continue
            # the uniform kernel on this sequence alone, at its own sizes
            nkp = (nk + 63) // 64 * 64
            q1 = q[s * K:s * K + nq].contiguous()
            k1 = k[kv * K:kv * K + nk].contiguous()
            vt1 = torch.empty(1, 256, nkp, dtype=dt, device=dev)
            ops.lg_transpose(v[kv * K:kv * K + nk].contiguous(), vt1, 1, nk, nkp, 256)
            ref = torch.empty(nq, 256, dtype=out_dt, device=dev)
            ops.sdpa(q1, k1, vt1, ref, 1, H, nq, nk, nkp, D=D)
            assert torch.equal(rows[:nq], ref), f"sequence {s} (len_q {nq}, len_k {nk}, {dt} -> {out_dt}): not gim_sdpa's bits"


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "nan-padding"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("precision", list(DTYPES))
def test_sdpa_varlen_is_sdpa_per_sequence(precision, cross, poison):
    _sdpa_case(DTYPES[precision], 64, cross, poison)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sdpa_varlen_head_dim_128(precision):
    _sdpa_case(DTYPES[precision], 128, True, True)


# ------------------------------------------------------------------------------------------------ assignment
@functools.lru_cache(maxsize=None)
def _assign_inputs():
    """B = 6 pairs of capacity K x K: descriptors and final_proj outputs of planted, match-rich pairs (CPU, never modified)"""
    g = torch.Generator().manual_seed(3)
    kp0, d0, kp1, d1 = O.planted_descriptors(len(LEN_A), K, seed=21)
    md0, md1 = 16.0 * d0 + 0.1 * torch.randn(d0.shape, generator=g), 16.0 * d1 + 0.1 * torch.randn(d1.shape, generator=g)
    return d0, d1, md0, md1, torch.randn(256, generator=g) / 16.0, torch.tensor([2.0])


def _assign(poison):
    from gim_amd import ops
    dev = _dev()
    d0, d1, md0, md1, mw, mb = (t.to(dev).clone() for t in _assign_inputs())
    B = len(LEN_A)
    if poison:
        for b in range(B):
            for t, n in ((d0, LEN_A[b]), (md0, LEN_A[b]), (d1, LEN_B[b]), (md1, LEN_B[b])):
                t[b, n:] = float("nan")
    r = ops.lg_assign(d0, d1, md0, md1, mw, mb, 0.1, _i32(LEN_A), _i32(LEN_B))
    counts = r.count.tolist()
    packed = ops.lg_emit_matches(r, sum(counts))
    return (d0, d1, md0, md1, mw, mb), r, counts, packed


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "nan-padding"])
def test_assign_ragged_is_assign_per_pair(poison):
    from gim_amd import ops
    (d0, d1, md0, md1, mw, mb), r, counts, packed = _assign(poison)
    off, matched = 0, 0
    for b, (n0, n1) in enumerate(zip(LEN_A, LEN_B)):
        assert (r.matches0[b, n0:] == -1).all() and not r.mscores0[b, n0:].any() and (r.pos[b, n0:] == -1).all(), b
        assert (r.matches1[b, n1:] == -1).all() and not r.mscores1[b, n1:].any(), b
        if n0 == 0 or n1 == 0:    # an empty side: nothing matches
            assert (r.matches0[b] == -1).all() and (r.matches1[b] == -1).all() and counts[b] == 0
            assert not r.mscores0[b].any() and not r.mscores1[b].any()
            continue
        u = ops.lg_assign(d0[b:b + 1, :n0].contiguous(), d1[b:b + 1, :n1].contiguous(), md0[b:b + 1, :n0].contiguous(),
                          md1[b:b + 1, :n1].contiguous(), mw, mb, 0.1)
        assert torch.equal(r.matches0[b, :n0], u.matches0[0]) and torch.equal(r.matches1[b, :n1], u.matches1[0]), (b, n0, n1)
        assert torch.equal(r.mscores0[b, :n0], u.mscores0[0]) and torch.equal(r.mscores1[b, :n1], u.mscores1[0]), (b, n0, n1)
        cu = int(u.count[0])
        assert counts[b] == cu
        pu = ops.lg_emit_matches(u, cu)
        assert torch.equal(packed[0][off:off + cu], pu[0]) and torch.equal(packed[1][off:off + cu], pu[1]), "compacted lists"
        off += cu
        matched += cu
    assert off == sum(counts) and matched > 100, "the planted pairs must produce matches"


def test_assign_ragged_ignores_what_the_padding_holds():
    _, a, ca, pa = _assign(False)
    _, b, cb, pb = _assign(True)
    assert ca == cb and torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    for k in ("matches0", "matches1", "mscores0", "mscores1", "pos"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("precision", list(DTYPES))
def test_gather_ragged_masks_by_count(precision, storage):
    from gim_amd import ops
    from gim_amd.lightglue import KeypointBank
    dev, dt = _dev(), DTYPES[precision]
    counts = [200, 129, 0, 64, 5]
    bank = KeypointBank(6, K, storage=storage, device=dev)
    for t in (bank.kpts, bank.desc, bank.enc):       # what an evicted image may have left behind
        t.fill_(float("nan"))
    wr = torch.randn(32, 2, generator=torch.Generator().manual_seed(2)).to(dev)
    bank._wr = wr
    g = torch.Generator().manual_seed(9)
    for i, n in enumerate(counts):
        bank.put(i, (torch.rand(n, 2, generator=g) * 400).to(dev), torch.randn(n, 256, generator=g).to(dev), torch.tensor([640.0, 480.0]))
    assert bank.slot_counts(bank.slots(range(5))) == counts
    for i, n in enumerate(counts):                   # and whatever else may sit behind an image's count
        s = bank.slots([i])[0]
        for t in (bank.kpts, bank.desc, bank.enc):
            t[s, n:] = float("nan")
    pairs = [(0, 1), (1, 0), (2, 3), (3, 4), (4, 4), (1, 2)]
    s0, s1 = bank.slot_tensor(bank.slots([p[0] for p in pairs])), bank.slot_tensor(bank.slots([p[1] for p in pairs]))
    B, R = len(pairs), 2 * len(pairs) * K
    alias = dt == torch.float32

    def run(ragged):
        cat = torch.full((R, 512), 7.0, dtype=dt, device=dev)
        x32 = cat[:, :256] if alias else torch.full((R, 256), 7.0, device=dev)
        enc = torch.full((R, 64), 7.0, device=dev)
        if ragged:
            lens = ops.lg_gather_pairs_ragged(bank.desc, bank.enc, bank.n, s0, s1, x32, None if alias else cat, enc)
        else:
            lens = None
            ops.lg_gather_pairs(bank.desc, bank.enc, s0, s1, x32, None if alias else cat, enc)
        return x32, cat[:, :256], enc, lens

    x, c, e, (l0, l1) = run(True)
    ux, uc, ue, _ = run(False)            # today's gather: every row of the slab
    assert l0.tolist() == [counts[p[0]] for p in pairs] and l1.tolist() == [counts[p[1]] for p in pairs]
    for side, ln in enumerate((l0.tolist(), l1.tolist())):
        for b, n in enumerate(ln):
            lo = (side * B + b) * K
            for name, got, want in (("x32", x, ux), ("cat", c, uc), ("enc", e, ue)):
                assert torch.equal(got[lo:lo + n], want[lo:lo + n]), f"{name}: valid rows of pair {b} side {side}"
                assert not got[lo + n:lo + K].any(), f"{name}: rows behind the count of pair {b} side {side} are not zero"
    assert not torch.isnan(x.float()).any() and not torch.isnan(e).any()
