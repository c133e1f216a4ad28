"""GPU tests of the batched sampler of the dense matchers: `ops.balanced_sample_pairs` (csrc/sample_pairs.hip), `DenseMatcher.sample_batch`
and `HlocDenseMatcher.match_pairs` on top of it.  Every comparison is `torch.equal` against the per-pair path (`balanced_sample`,
`ops.weighted_sample`, `ops.kde`) on the same device with the same seeds: no tolerances.  Intermediate results (keys, first-draw rows,
densities, per-pair counts) are read from the workspace, whose layout include/gim_hip.h documents."""
import numpy as np
import pytest
import torch

from test_gpu_dense_tail import _kde_points, _rows_of

pytestmark = pytest.mark.gpu

THRESH = 0.05


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _draw_seeds(seed, B):
    """the seeds B successive balanced_sample calls draw after torch.manual_seed(seed)"""
    torch.manual_seed(seed)
    return [torch.randint(0, 2 ** 31 - 1, (2,)).tolist() for _ in range(B)]


def _per_pair(matches, cert, num, seed, kde_half):
    """the per-pair path: B balanced_sample calls in order under torch.manual_seed(seed) -> [(rows, certainties)] on the CPU"""
    from gim_amd.dense import balanced_sample
    torch.manual_seed(seed)
    out = []
    for b in range(cert.shape[0]):
        sm, sc = balanced_sample(matches[b], cert[b], num, "threshold_balanced", THRESH, kde_half=kde_half)
        out.append((sm.cpu(), sc.cpu()))
    return out


def _batched(matches, cert, num, seed, kde_half):
    """ops.balanced_sample_pairs into outputs prefilled with NaN / -1 and a workspace prefilled with 0xff -> (sparse, mconf, count on the
    CPU, region(name) reading the workspace, the seeds)"""
    from gim_amd import ops
    B, n, dev = cert.shape[0], cert[0].numel(), cert.device
    seeds = _draw_seeds(seed, B)
    ws = torch.full((ops.balanced_sample_pairs_ws_bytes(B, n, num),), 0xff, dtype=torch.uint8, device=dev)
    out = (torch.full((B, num, 4), float("nan"), device=dev), torch.full((B, num), float("nan"), device=dev),
           torch.full((B,), -1, dtype=torch.int32, device=dev))
    ret = ops.balanced_sample_pairs(matches, cert, seeds, num, THRESH, kde_half, ws=ws, out=out)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(ret, out))
    return out[0].cpu(), out[1].cpu(), out[2].cpu(), (lambda name: ops.balanced_sample_pairs_region(ws, B, n, num, name).cpu()), seeds


def _check_against_per_pair(sparse, mconf, count, ref, what=""):
    """every element is written; pair b's first count[b] rows are the per-pair path's, the rest are zero"""
    assert not torch.isnan(sparse).any() and not torch.isnan(mconf).any() and (count >= 0).all(), f"{what}: outputs left unwritten"
    for b, (sm, sc) in enumerate(ref):
        k = int(count[b])
        assert k == sm.shape[0] == sc.shape[0], (what, b, k, sm.shape)
        assert torch.equal(sparse[b, :k], sm), f"{what}: pair {b}: rows differ from balanced_sample"
        assert torch.equal(mconf[b, :k], sc), f"{what}: pair {b}: certainties differ from balanced_sample"
        assert (sparse[b, k:] == 0).all() and (mconf[b, k:] == 0).all(), f"{what}: pair {b}: rows past its count are not zero"


def _check_workspace(region, matches, cert, seeds, count, num, kde_half, k1_want):
    """first-draw rows = the sorted set of ops.weighted_sample gathered, density = ops.kde of those rows, second-draw keys = the keys
    gim_weighted_sample computes for p -- bit for bit"""
    from gim_amd import ops
    B, n = cert.shape[0], cert[0].numel()
    state, rows, rowcert, density, keys2 = (region(k) for k in ("state", "rows", "rowcert", "density", "keys2"))
    for b in range(B):
        c = cert[b].reshape(-1)
        flat = matches[b].reshape(-1, 4)
        w = torch.where(c > THRESH, torch.ones_like(c), c)
        n_pos = int((w > 0).sum())
        assert int(state[b, 0]) == n_pos
        if n_pos == 0:
            w, n_pos = w + 1e-8, n
        k1 = int(state[b, 1])
        assert k1 == k1_want[b] == min(rows.shape[1], n_pos), (b, k1, k1_want[b])
        assert int(state[b, 2]) == int(count[b]) == min(num, k1)
        good = ops.weighted_sample(w.contiguous(), k1, seeds[b][0]).sort().values
        gm = flat[good].contiguous()
        assert torch.equal(rows[b, :k1], gm.cpu()), f"pair {b}: first-draw rows"
        assert torch.equal(rowcert[b, :k1], c[good].cpu()), f"pair {b}: first-draw certainties (un-thresholded)"
        d = ops.kde(gm, 0.1, half=kde_half)
        assert torch.equal(density[b, :k1], d.cpu()), f"pair {b}: density differs from ops.kde by up to {(density[b, :k1] - d.cpu()).abs().max()}"
        p = torch.where(d < 10, torch.full_like(d, 1e-7), 1 / (d + 1)).contiguous()
        wsp = torch.zeros(ops.weighted_sample_ws_bytes(k1), dtype=torch.uint8, device=p.device)
        ops.weighted_sample(p, int(count[b]), seeds[b][1], ws=wsp)
        assert torch.equal(keys2[b, :k1], wsp[:4 * k1].view(torch.int32).cpu()), f"pair {b}: second-draw keys"


# ------------------------------------------------------------------------------------------------ 1. every branch in one batch
def _branch_batch():
    """B = 5 maps of 24 x 40: 600 / 120 / 30 / 0 positive certainties, pair 4 = pair 0's maps"""
    g = torch.Generator().manual_seed(200)
    H, W2, n = 24, 40, 960
    matches = torch.rand(5, n, 4, generator=g) * 2 - 1
    matches[:, :400] = torch.tensor([0.3, -0.2, 0.25, -0.15]) + 0.05 * torch.randn(5, 400, 4, generator=g)   # a dense region: densities > 10
    cert = torch.zeros(5, n)
    for b, npos in ((0, 600), (1, 120), (2, 30)):
        where = torch.randperm(n, generator=g)[:npos]
        cert[b, where] = torch.cat((torch.rand(npos // 2, generator=g) * 0.04 + 0.005, torch.rand(npos - npos // 2, generator=g) * 0.9 + 0.06))
        assert int((cert[b] > 0).sum()) == npos and (cert[b][where] < THRESH).any() and (cert[b][where] > THRESH).any()
    matches[4], cert[4] = matches[0], cert[0]
    for b in range(5):
        assert matches[b].unique(dim=0).shape[0] == n                    # rows are distinct: _rows_of recovers the flat index
    return matches.reshape(5, H, W2, 4).contiguous(), cert.reshape(5, H, W2).contiguous()


@pytest.mark.parametrize("kde_half", [False, True], ids=["fp32", "half"])
def test_every_branch_in_one_batch(kde_half):
    dev = _dev()
    matches, cert = _branch_batch()
    md, cd = matches.to(dev), cert.to(dev)
    num, seed = 50, 31
    sparse, mconf, count, region, seeds = _batched(md, cd, num, seed, kde_half)
    print(f"count {count.tolist()}, state {region('state')[:, :3].tolist()}")
    assert count.tolist() == [50, 50, 30, 50, 50]
    _check_against_per_pair(sparse, mconf, count, _per_pair(md, cd, num, seed, kde_half), "branches")
    _check_workspace(region, md, cd, seeds, count, num, kde_half, k1_want=[200, 120, 30, 200, 200])
    assert (region("density")[0, :200] > 10).any() and (region("density")[0, :200] < 10).any()       # both sides of the cut
    assert (mconf[3] == 0).all() and (sparse[2, 30:] == 0).all() and (mconf[2, 30:] == 0).all()
    assert (mconf[:2] > 0).all() and (mconf[1] < THRESH).any() and (mconf[1] > THRESH).any()          # the un-thresholded certainty
    idx = []
    for b in range(5):
        r = _rows_of(sparse[b, :int(count[b])], matches[b].reshape(-1, 4))
        assert (r[1:] > r[:-1]).all(), f"pair {b}: rows are not in ascending flat index"
        assert torch.equal(mconf[b, :int(count[b])], cert[b].reshape(-1)[r])
        idx.append(r.tolist())
    assert len(set(idx[3])) == 50                                        # the `+ 1e-8` path: 50 distinct rows
    assert idx[4] != idx[0]                                              # the same maps, other seeds


# ------------------------------------------------------------------------------------------------ 2. threshold ties across workgroups
def test_threshold_ties_across_workgroups_take_the_smallest_indices():
    """all certainties 1.0: with 23-bit clocks 300 000 keys hold ~5000 duplicated values.  A `num` whose first-draw threshold key is
    duplicated, with the tied indices in different workgroups, must take the tied keys by ascending index.  n >= 256 * 1024: the
    grid-stride launch of the key and histogram kernels.  Column 0 of the matches is the flat index, so sets are read off the rows."""
    dev = _dev()
    B, n, seed = 2, 300_000, 77
    g = torch.Generator().manual_seed(201)
    matches = torch.rand(B, n, 4, generator=g) * 2 - 1
    matches[:, :, 0] = torch.arange(n, dtype=torch.float32)
    md, cd = matches.to(dev), torch.ones(B, n, device=dev)
    _, _, _, region, seeds = _batched(md, cd, 1, seed, False)
    keys = region("keys1")[0, :n].numpy().view(np.uint32)
    assert (keys > 0).all()
    # candidates: duplicated values among the 4000 largest keys (the KDE of the first draw is quadratic in 4 * num)
    top = np.sort(keys)[::-1][:4000]
    vals, counts = np.unique(top[top > top[-1]], return_counts=True)
    best = None
    for v, m in zip(vals[counts >= 2], counts[counts >= 2]):
        tied = np.flatnonzero(keys == v)
        above = int((keys > v).sum())
        for take in range(1, int(m)):
            if (above + take) % 4 == 0 and (best is None or np.ptp(tied) > best[0]):
                best = (int(np.ptp(tied)), int(v), tied, above, take)
    assert best is not None, "no duplicated threshold key with 4 | k1 among the top 4000 keys"
    spread, v, tied, above_n, take = best
    print(f"[measured] threshold key {v:#x} x{tied.size} at {tied.tolist()} (spread {spread}), {above_n} keys above, take {take}")
    assert spread >= 8 * 2048, spread                                    # condition on the input: the ties lie workgroups apart
    num = (above_n + take) // 4
    sparse, mconf, count, region, seeds2 = _batched(md, cd, num, seed, False)
    assert seeds2 == seeds and np.array_equal(region("keys1")[0, :n].numpy().view(np.uint32), keys)
    assert region("state")[:, 1].tolist() == [4 * num, 4 * num] and count.tolist() == [num, num]
    first = region("rows")[0, :4 * num, 0].long().numpy()
    want = np.sort(np.concatenate((np.flatnonzero(keys > v), tied[:take])))
    assert np.array_equal(first, want), f"took {np.intersect1d(first, tied)} of the tied indices {tied}, want {tied[:take]}"
    _check_against_per_pair(sparse, mconf, count, _per_pair(md, cd, num, seed, False), "ties")


# ------------------------------------------------------------------------------------------------ 3. chunk edges of the KDE
@pytest.mark.parametrize("kde_half", [False, True], ids=["fp32", "half"])
def test_kde_chunk_edges_across_one_batch(kde_half):
    """k1 = 63, 64, 65, 256, 257 in one batch (num = 65: 4 * num = 260): one 64-point chunk, one chunk +- 1, a full round of the four
    waves + 1; the rows that can be drawn are clustered points, so densities fall on both sides of 10"""
    from gim_amd import ops
    dev = _dev()
    k1s, n, num = [63, 64, 65, 256, 257], 600, 65
    g = torch.Generator().manual_seed(202)
    matches = torch.rand(5, n, 4, generator=g) * 2 - 1
    cert = torch.zeros(5, n)
    for b, k1 in enumerate(k1s):
        where = torch.randperm(n, generator=g)[:k1].sort().values
        matches[b, where] = _kde_points(k1)
        cert[b, where] = torch.rand(k1, generator=g) * 0.9 + 0.06
    md, cd = matches.to(dev), cert.to(dev)
    sparse, mconf, count, region, seeds = _batched(md, cd, num, 41, kde_half)
    assert region("state")[:, 1].tolist() == k1s and count.tolist() == [63, 64, 65, 65, 65]
    density, rows = region("density"), region("rows")
    for b, k1 in enumerate(k1s):
        assert torch.equal(rows[b, :k1], matches[b][cert[b] > 0])        # every positive row, in index order
        ref = ops.kde(rows[b, :k1].contiguous().to(dev), 0.1, half=kde_half).cpu()
        assert torch.equal(density[b, :k1], ref), (b, k1, (density[b, :k1] - ref).abs().max().item())
        if k1 >= 256:
            assert (ref < 10).any() and (ref > 100).any(), (ref.min().item(), ref.max().item())
    _check_against_per_pair(sparse, mconf, count, _per_pair(md, cd, num, 41, kde_half), "kde edges")


# ------------------------------------------------------------------------------------------------ 4. tiny weights
def test_tiny_weights_are_drawn_and_every_output_is_written():
    """certainties down to the smallest subnormal, k1 = every positive weight (4 * num = 2800 >= the ~2730 positives): a key that
    rounded to 0 would leave first-draw rows unwritten; the floor at 1 keeps them drawable and they tie by ascending index"""
    dev = _dev()
    n, num = 4096, 700
    g = torch.Generator().manual_seed(83)
    cert = torch.tensor([1.4e-45, 1e-42, 1e-38, 1e-30])[torch.randint(0, 4, (2, n), generator=g)]
    cert[:, ::3] = 0.0
    assert (cert[cert != 0] > 0).all() and (cert == 1.4e-45).sum() > 200  # the subnormal survives the host side
    matches = torch.rand(2, n, 4, generator=g) * 2 - 1
    matches[:, :, 0] = torch.arange(n, dtype=torch.float32)
    md, cd = matches.to(dev), cert.to(dev)
    sparse, mconf, count, region, seeds = _batched(md, cd, num, 2024, False)
    n_pos = (cert > 0).sum(1).tolist()
    assert max(n_pos) <= 4 * num and region("state")[:, 0].tolist() == n_pos and region("state")[:, 1].tolist() == n_pos
    assert count.tolist() == [num, num]
    for b in range(2):
        keys = region("keys1")[b, :n]
        assert ((keys != 0) == (cert[b] > 0)).all(), "a positive weight got key 0"
        assert np.array_equal(region("rows")[b, :n_pos[b], 0].long().numpy(), np.flatnonzero(cert[b].numpy() > 0))
    _check_against_per_pair(sparse, mconf, count, _per_pair(md, cd, num, 2024, False), "tiny weights")
    assert (mconf > 0).all()


# ------------------------------------------------------------------------------------------------ 5. sample_batch
def _matcher():
    from gim_amd.dkm import DKMv3
    return DKMv3(None, 128, 160, upsample_preds=True, precision="bf16")


def test_sample_batch_follows_torch_manual_seed():
    dev = _dev()
    net = _matcher()
    g = torch.Generator().manual_seed(203)
    B, H, W2, num = 3, 24, 40, 60
    matches = (torch.rand(B, H, W2, 4, generator=g) * 2 - 1).to(dev)
    cert = torch.rand(B, H, W2, generator=g).to(dev)
    cert[1].view(-1)[100:] = 0.0                                         # 100 positives: k1 = 100, k2 = 60
    cert[2].view(-1)[40:] = 0.0                                          # 40 positives: k2 = 40
    torch.manual_seed(5)
    a = net.sample_batch(matches, cert, num)
    state_batch = torch.get_rng_state()
    torch.manual_seed(5)
    b = net.sample_batch(matches, cert, num)
    torch.manual_seed(6)
    c = net.sample_batch(matches, cert, num)
    assert all(t.is_cuda for t in a) and a[0].shape == (B, num, 4) and a[1].shape == (B, num) and a[2].dtype == torch.int32
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])
    torch.manual_seed(5)
    ref = [net.sample(matches[i], cert[i], num) for i in range(B)]
    assert torch.equal(torch.get_rng_state(), state_batch)               # the generator is where B sample() calls leave it
    assert a[2].tolist() == [60, 60, 40]
    _check_against_per_pair(a[0].cpu(), a[1].cpu(), a[2].cpu(), [(m.cpu(), s.cpu()) for m, s in ref], "sample_batch")
    with pytest.raises(Exception, match="contiguous fp32"):
        net.sample_batch(matches.double(), cert.double(), num)
    with pytest.raises(Exception, match="contiguous fp32"):
        net.sample_batch(matches.transpose(1, 2), cert.transpose(1, 2), num)


def test_sample_batch_splits_more_than_16_pairs():
    dev = _dev()
    net = _matcher()
    g = torch.Generator().manual_seed(204)
    B, num = 18, 20
    matches = (torch.rand(B, 8, 12, 4, generator=g) * 2 - 1).to(dev)
    cert = torch.rand(B, 8, 12, generator=g).to(dev)
    torch.manual_seed(9)
    sparse, mconf, count = net.sample_batch(matches, cert, num)
    torch.manual_seed(9)
    ref = [net.sample(matches[i], cert[i], num) for i in range(B)]
    _check_against_per_pair(sparse.cpu(), mconf.cpu(), count.cpu(), [(m.cpu(), s.cpu()) for m, s in ref], "18 pairs")


# ------------------------------------------------------------------------------------------------ 6. match_pairs end to end
class _HostReads:
    """counts what makes the host wait for the device: torch.cuda.synchronize, and tolist / item / int() / float() / bool() of a device
    tensor"""

    NAMES = ("tolist", "item", "__int__", "__float__", "__bool__")

    def __init__(self, monkeypatch):
        self.n = 0
        for name in self.NAMES:
            monkeypatch.setattr(torch.Tensor, name, self._wrap(getattr(torch.Tensor, name)))
        sync = torch.cuda.synchronize

        def counted_sync(*a, **k):
            self.n += 1
            return sync(*a, **k)
        monkeypatch.setattr(torch.cuda, "synchronize", counted_sync)

    def _wrap(self, fn):
        def counted(t, *a, **k):
            if t.is_cuda and not self.inside:
                self.n += 1
                self.inside = True                  # item() inside tolist() is one read
                try:
                    return fn(t, *a, **k)
                finally:
                    self.inside = False
            return fn(t, *a, **k)
        return counted

    inside = False


def test_match_pairs_reads_the_device_once_per_batch(monkeypatch):
    from test_gpu_dense_pairs import _images, _net
    from gim_amd.adapters import HlocDenseMatcher
    from gim_amd.dense_bank import DenseFeatureBank
    dev = _dev()
    images = _images(dev)
    adapter = HlocDenseMatcher(_net(), 128, 160, num_samples=512)
    pairs = [("a.jpg", "b.jpg"), ("b.jpg", "a.jpg"), ("a.jpg", "c.jpg")]
    torch.manual_seed(11)
    ref = [adapter({"image0": images[n0], "image1": images[n1]}) for n0, n1 in pairs]
    bank = DenseFeatureBank(adapter.net, 3)
    for name in ("a.jpg", "b.jpg", "c.jpg"):
        adapter.bank_put(bank, name, images[name])
    adapter.match_pairs(bank, pairs[:2], batch_pairs=2)                  # buffers and workspaces exist before the counted run
    torch.manual_seed(11)
    with monkeypatch.context() as mp:
        reads = _HostReads(mp)
        got = adapter.match_pairs(bank, pairs, batch_pairs=2)
        n_reads = reads.n
    print(f"{n_reads} host reads for 3 pairs in 2 batches")
    assert n_reads == 2, f"{n_reads} host reads for two batches: want the count.tolist() of each batch and nothing else"
    for p, (gp, r) in enumerate(zip(got, ref)):
        assert r["scores"].shape[0] > 0
        for k in ("keypoints0", "keypoints1", "scores", "batch_indexes"):
            assert torch.equal(gp[k], r[k]), (p, k)
