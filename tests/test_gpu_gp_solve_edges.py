"""csrc/gp_solve.hip (gim_gp_solve, gim_gp_posterior_f64) at its block, pair-tree, layout and batch edges, against the fp64 references
of tests/gp_cases.py (judged on the host by tests/test_gp_cases_cpu.py).

Bound: max|got - float(ref)| <= 2^-23 max|ref| per batch entry -- derived in gp_cases.py (one rounding of an fp64 result to fp32 is
2^-24; the fp64 error of either side is ~1e-11 of scale at cond <= 1e5), never widened from a measurement.  Every comparison prints its
ratio (pytest -s).  Measured on an MI355X, fraction of scale (bound 1.192e-07) -- an fp64 result rounded once either IS the rounded
reference or sits one fp32 ulp of that element from it, so most ratios are exactly 0:
  gp_solve, n = 1 ... 577 (13 sizes), the 32 layout cases at n = 129, B = 16, the NaN workspaces, next to a failed entry: 0 in every
      case but n = 128 (1.3e-16: one ulp of one tiny element);
  gp_posterior_f64, 72 cases + the NaN workspaces + next to a failed direction: 0 in 73, 1.3e-11 (n=1 d=70 nrhs=65 B=2) and 1.8e-08 in
      the other two.  (Against a reference fed Python's 0.2 / 1e-6 / 0.1 instead of the C floats the ABI carries, the same outputs
      measure 3e-8 ... 1.13e-07: see gp_cases.py.)
Sanity check of this file: with the last pair's row count (mlast in chol_solve) forced to 0 in a scratch build, every gp_solve size
above 64 (65, 127, 128, 129, 192, 193, 320, 321, 577), the B = 16 case and the gp_posterior_f64 cases with n > 64 fail.
"""
import ctypes

import pytest
import torch

import gp_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.25


def _check(got, ref, what):
    """got fp32 [B, ...] (device), ref fp64 [B, ...]: the derived bound, per batch entry; prints the largest ratio"""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    B = ref.shape[0]
    err = (got.double() - ref.float().double()).abs().reshape(B, -1).amax(1)
    scale = ref.abs().reshape(B, -1).amax(1)
    ratio = (err / scale).max().item()
    print(f"[close] {what}: {ratio:.3e} of scale (bound 2^-23 = {C.TOL:.3e})")
    assert (err <= C.TOL * scale).all(), f"{what}: {ratio:.3e} of scale over the bound 2^-23 = {C.TOL:.3e}; per entry {(err / scale).tolist()}"
    return ratio


def _solve(K, F, ldk, npad):
    """ops.gp_solve on K [B,n,n] stored with row stride ldk, the columns beyond n holding NaN (they must not be read)"""
    from gim_amd import ops
    B, n, _ = K.shape
    Kp = torch.full((B, n, ldk), float("nan"))
    Kp[:, :, :n] = K
    Xt = ops.gp_solve(Kp.to(DEV), F.to(DEV).contiguous(), npad)
    assert Xt.shape == (B, F.shape[2], npad)
    return Xt


def _up(n, m):
    return (n + m - 1) // m * m


def _posterior(X, Y, F, sigma=0.1):
    """ops.gp_posterior_f64 into a row view with stride(0) = nrhs + 7 whose 7 trailing columns hold a sentinel -> (mu [B,n,nrhs], buffer)"""
    from gim_amd import ops
    B, n, _ = X.shape
    nrhs = F.shape[1]
    buf = torch.full((B * n, nrhs + 7), SENTINEL, device=DEV)
    out = buf[:, :nrhs]
    assert out.stride(0) == nrhs + 7
    ops.gp_posterior_f64(X.to(DEV), Y.to(DEV), F.to(DEV), out, 0.2, 1e-6, sigma)
    assert (buf[:, nrhs:] == SENTINEL).all(), "gp_posterior_f64 wrote beyond nrhs columns"
    return out.reshape(B, n, nrhs), buf


# ---------------------------------------------------------------------------------------- gp_solve: blocks and the pair tree
@pytest.mark.parametrize("n", C.SOLVE_NS)
def test_gp_solve_block_and_pair_tree_edges(n):
    """n <= 64: one block, no doubling level; 65 / 127 / 128 / 129: 1- and 63-row last block, one level with a ragged and a full last
    pair, a second level with a 1-row half; 192 / 193: 3 blocks (no second half at level 64); 320 / 321: 5 blocks; 577: 9 blocks + 1 row"""
    K, F = C.solve_case(n, 2)
    npad = _up(n, 32)
    Xt = _solve(K, F, _up(n, 64), npad)
    _check(Xt[:, :, :n].transpose(1, 2), C.solve_ref(n, 2), f"gp_solve n={n}")
    assert (Xt[:, :, n:] == 0).all()


@pytest.mark.parametrize("npad_kind", ["n", "n+1", "160", "n+100"])
@pytest.mark.parametrize("ldk_extra", [0, 5])
@pytest.mark.parametrize("nrhs", C.LAYOUT_NRHS)
def test_gp_solve_layout_edges(nrhs, ldk_extra, npad_kind):
    """nrhs against the 64-column tiles of the GEMM and of the transposing store, ldk > n (NaN beyond n), npad up to a whole 64-tile
    of pure padding (n + 100)"""
    n = C.LAYOUT_N
    npad = {"n": n, "n+1": n + 1, "160": 160, "n+100": n + 100}[npad_kind]
    K, F = C.solve_case(n, 2, nrhs)
    Xt = _solve(K, F, n + ldk_extra, npad)
    _check(Xt[:, :, :n].transpose(1, 2), C.solve_ref(n, 2, nrhs), f"gp_solve n={n} nrhs={nrhs} ldk=n+{ldk_extra} npad={npad_kind}")
    assert (Xt[:, :, n:] == 0).all()


# ---------------------------------------------------------------------------------------- the batch limit
def test_gp_solve_batch_16():
    """B = 16 distinct matrices: the dense matchers' max_batch = 8 pairs, and the whole 64-byte info area"""
    n, B = C.BATCH_N, C.MAX_B
    K, F = C.solve_case(n, B)
    Xt = _solve(K, F, _up(n, 64), _up(n, 32))
    _check(Xt[:, :, :n].transpose(1, 2), C.solve_ref(n, B), f"gp_solve n={n} B={B}")
    assert (Xt[:, :, n:] == 0).all()


def test_batch_17_is_refused():
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    n, B = 5, C.MAX_B + 1
    K = (torch.eye(n) * 1.1).expand(B, n, n).contiguous().to(DEV)
    F = torch.ones(B, n, 3, device=DEV)
    with pytest.raises(GimHipError, match="gp_solve"):
        ops.gp_solve(K, F, 32)
    X = torch.ones(B, n, 4, device=DEV)
    out = torch.full((B * n, 3), SENTINEL, device=DEV)
    with pytest.raises(GimHipError, match="gp_posterior_f64"):
        ops.gp_posterior_f64(X, X.clone(), F[0].contiguous(), out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("n", [C.BATCH_N, 193])
def test_batch_invariance(n):
    """entry b of a B = 16 call is the B = 1 call on the same matrix, bit for bit, through both entry points"""
    B = C.MAX_B
    K, F = C.solve_case(n, B)
    ldk, npad = _up(n, 64), _up(n, 32)
    Xt = _solve(K, F, ldk, npad).cpu()
    X, Y, Fp = C.posterior_case(n, B, 70, C.NRHS)
    mu = _posterior(X, Y, Fp)[0].cpu()
    for b in range(B):
        assert torch.equal(_solve(K[b:b + 1], F[b:b + 1], ldk, npad).cpu()[0], Xt[b]), f"gp_solve entry {b}"
        assert torch.equal(_posterior(X[b:b + 1], Y[b:b + 1], Fp)[0].cpu()[0], mu[b]), f"gp_posterior_f64 entry {b}"


# ---------------------------------------------------------------------------------------- the workspace contract
def _guarded(nbytes):
    """nbytes of workspace between two 4096-byte guards, everything 0xFF (NaN as doubles) -> (buffer, pointer to the workspace)"""
    buf = torch.full((nbytes + 2 * 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + 4096)


def _guards_intact(buf, nbytes):
    return bool((buf[:4096] == 0xFF).all()) and bool((buf[4096 + nbytes:] == 0xFF).all())


@pytest.mark.parametrize("n,B", [(193, 2), (C.BATCH_N, C.MAX_B)])
def test_gp_solve_workspace_contract(n, B):
    """no scratch is read before it is written (a workspace of NaN gives the same bits as any other), and gim_gp_solve_ws_bytes bounds
    the footprint (the guards on both sides keep their fill)"""
    from gim_amd import ops
    from gim_amd._lib import check, lib
    nrhs, ldk, npad = C.NRHS, _up(n, 64), _up(n, 32)
    K, F = C.solve_case(n, B)
    plain = _solve(K, F, ldk, npad)
    Kp = torch.zeros(B, n, ldk)
    Kp[:, :, :n] = K
    Kd, Fd = Kp.to(DEV), F.to(DEV).contiguous()
    nbytes = lib.gim_gp_solve_ws_bytes(B, n, nrhs)
    buf, ws = _guarded(nbytes)
    Xt = torch.full((B, nrhs, npad), SENTINEL, device=DEV)
    check(lib.gim_gp_solve(ops._p(Kd), ops._p(Fd), ops._p(Xt), ws, B, n, ldk, nrhs, npad, ops._stream()), "gim_gp_solve")
    torch.cuda.synchronize()
    assert torch.equal(Xt, plain)
    assert _guards_intact(buf, nbytes)
    _check(Xt[:, :, :n].transpose(1, 2), C.solve_ref(n, B), f"gp_solve n={n} B={B}, workspace of NaN")


@pytest.mark.parametrize("n,B", [(193, 2), (C.BATCH_N, C.MAX_B)])
def test_gp_posterior_workspace_contract(n, B):
    from gim_amd import ops
    from gim_amd._lib import check, lib
    d, nrhs = 70, C.NRHS
    X, Y, F = C.posterior_case(n, B, d, nrhs)
    plain, _ = _posterior(X, Y, F)
    Xd, Yd, Fd = X.to(DEV), Y.to(DEV), F.to(DEV)
    nbytes = lib.gim_gp_posterior_f64_ws_bytes(B, n, d, nrhs)
    buf, ws = _guarded(nbytes)
    mu = torch.full((B, n, nrhs), SENTINEL, device=DEV)
    check(lib.gim_gp_posterior_f64(ops._p(Xd), ops._p(Yd), ops._p(Fd), ops._p(mu), ws, B, n, d, d, nrhs, nrhs, 0.2, 1e-6, 0.1, ops._stream()),
          "gim_gp_posterior_f64")
    torch.cuda.synchronize()
    assert torch.equal(mu, plain)
    assert _guards_intact(buf, nbytes)
    _check(mu, C.posterior_ref(n, B, d, nrhs), f"gp_posterior_f64 n={n} B={B} d={d}, workspace of NaN")


# ---------------------------------------------------------------------------------------- gp_posterior_f64 directly
@pytest.mark.parametrize("B", C.POST_BS)
@pytest.mark.parametrize("nrhs", C.POST_NRHS)
@pytest.mark.parametrize("d", C.POST_DS)
@pytest.mark.parametrize("n", C.POST_NS)
def test_gp_posterior_f64(n, d, nrhs, B):
    """d = 70 leaves a ragged slab of the 32-wide K loop in all three operand orientations (Y Y^T, X Y^T: A rows / B transposed; the
    solve's L^-T product: A transposed); n as in the gp_solve sweep; the output is a strided row view"""
    X, Y, F = C.posterior_case(n, B, d, nrhs)
    mu, _ = _posterior(X, Y, F)
    _check(mu, C.posterior_ref(n, B, d, nrhs), f"gp_posterior_f64 n={n} d={d} nrhs={nrhs} B={B}")


# ---------------------------------------------------------------------------------------- a failed factorisation is visible
@pytest.mark.parametrize("kind", ["negdiag", "nan"])
def test_gp_solve_failed_entry_is_nan(kind):
    """a batch whose middle matrix is not positive definite (one negative diagonal entry in the ragged last block) / holds a NaN: all
    of Xt[1] is NaN, padding included; its neighbours are, bit for bit, what they are in a clean batch"""
    n, B, bad = C.BROKEN_N, C.BROKEN_B, C.BROKEN_AT
    K, F = C.broken_solve_case(kind)
    assert C.cholesky_rejects(K) == [b == bad for b in range(B)]
    ldk, npad = _up(n, 64), n + 100
    Xt = _solve(K, F, ldk, npad)
    assert torch.isnan(Xt[bad]).all(), f"{int(torch.isfinite(Xt[bad]).sum())} finite elements in the failed entry"
    good = [b for b in range(B) if b != bad]
    _check(Xt[good][:, :, :n].transpose(1, 2), C.solve_ref(n, B)[good], f"gp_solve next to a failed entry ({kind})")
    assert (Xt[good][:, :, n:] == 0).all()
    clean = _solve(*C.solve_case(n, B), ldk, npad)
    assert torch.equal(Xt[good], clean[good]) and torch.isfinite(clean).all()


def test_gp_posterior_failed_entry_is_nan():
    """one NaN support row in direction 1: K_yy of that direction fails to factor, all of mu[1] is NaN, the trailing columns keep the
    sentinel, the other directions are what they are in a clean batch"""
    n, B, bad = C.BROKEN_N, C.BROKEN_B, C.BROKEN_AT
    X, Y, F = C.broken_posterior_case()
    Kyy = C.cos_kernel64(Y.double(), Y.double()) + 0.1 * torch.eye(n, dtype=torch.float64)
    assert C.cholesky_rejects(Kyy) == [b == bad for b in range(B)]
    mu, _ = _posterior(X, Y, F)
    assert torch.isnan(mu[bad]).all(), f"{int(torch.isfinite(mu[bad]).sum())} finite elements in the failed direction"
    good = [b for b in range(B) if b != bad]
    _check(mu[good], C.posterior_ref(n, B, 32, C.NRHS)[good], "gp_posterior_f64 next to a failed direction")
    clean, _ = _posterior(*C.posterior_case(n, B, 32, C.NRHS))
    assert torch.equal(mu[good], clean[good]) and torch.isfinite(clean).all()


def test_gp_posterior_indefinite_is_nan():
    """The NaN row above also reaches mu through K_xy; this failure does not.  With sigma = -0.5 every K_yy + sigma I is finite and
    indefinite (C.INDEFINITE_SIGMA, rejected by the host's Cholesky too): only the info word stands between the substituted pivots'
    finite numbers and the output."""
    n, B = C.BROKEN_N, C.BROKEN_B
    X, Y, F = C.posterior_case(n, B, 3, C.NRHS)          # d = 3: K_yy has eigenvalues far below 0.5
    Kyy = C.cos_kernel64(Y.double(), Y.double()) + C.INDEFINITE_SIGMA * torch.eye(n, dtype=torch.float64)
    assert torch.isfinite(Kyy).all() and C.cholesky_rejects(Kyy) == [True] * B
    mu, _ = _posterior(X, Y, F, sigma=C.INDEFINITE_SIGMA)
    assert torch.isnan(mu).all(), f"{int(torch.isfinite(mu).sum())} finite elements behind failed factorisations"


@pytest.mark.parametrize("exact", [True, False], ids=["fp64-gp", "fp32-entries"])
def test_nan_feature_reaches_the_matchers_gp_output(exact):
    """dense.gp_posterior, the GP stage of gim_dkm / gim_roma, in both of its modes: one NaN feature row in image 1 makes the whole
    posterior of direction 0 (whose support is image 1) NaN -- not a finite number -- and, of direction 1, the row it queries"""
    from gim_amd import dense
    h, w, nb, dim = 7, 11, 2, 64
    n = h * w
    g = torch.Generator().manual_seed(31)
    a32 = torch.zeros(nb * n + 64, 512)
    a32[:nb * n] = torch.randn(nb * n, 512, generator=g)
    a32[n + 40] = float("nan")
    f = torch.randn(n, dim, generator=g)
    out = torch.full((nb * n, dim), SENTINEL, device=DEV)
    dense.gp_posterior(a32.to(DEV), nb, h, w, f.to(DEV), out, exact)
    out = out.cpu().view(nb, n, dim)
    assert torch.isnan(out[0]).all(), f"{int(torch.isfinite(out[0]).sum())} finite elements behind a failed factorisation"
    assert torch.isnan(out[1, 40]).all()
    rest = torch.cat((out[1, :40], out[1, 41:]))
    assert torch.isfinite(rest).all() and (rest != SENTINEL).all()
