"""The references and cases of tests/gp_cases.py, checked without a GPU: every matrix a GPU test of csrc/gp_solve.hip factors is
within the stated condition cap, two independent fp64 routes (LU, Cholesky) to the reference agree far below the GPU tests' bound, the
batch entries are distinct, and the inputs of the failed-factorisation tests are rejected by torch.linalg.cholesky in exactly the
entries the GPU tests expect as NaN."""
import pytest
import torch

import gp_cases as C


def _cond(K):
    s = torch.linalg.svdvals(K.double())
    return (s[..., 0] / s[..., -1]).max().item()


@pytest.mark.parametrize("n,B,nrhs", C.SOLVE_TABLE)
def test_solve_reference(n, B, nrhs):
    K, F = C.solve_case(n, B, nrhs)
    assert K.shape == (B, n, n) and F.shape == (B, n, nrhs) and K.dtype == F.dtype == torch.float32
    assert torch.equal(K, K.transpose(1, 2))
    if n > 1:
        assert all(not torch.equal(K[a], K[b]) for a in range(B) for b in range(a)), "every batch entry its own matrix"
    cond = _cond(K)
    ref, alt = C.solve_ref(n, B, nrhs), C.ref_solve_chol(K, F)
    agree = ((ref - alt).abs().amax((1, 2)) / ref.abs().amax((1, 2))).max().item()
    print(f"[gp case] solve n={n} B={B} nrhs={nrhs}: cond {cond:.3g} (cap {C.COND_CAP:g}), LU vs Cholesky {agree:.2e} of scale "
          f"(cap 2^-30 = {C.REF_AGREE:.2e})")
    assert cond <= C.COND_CAP and agree <= C.REF_AGREE
    assert C.cholesky_rejects(K) == [False] * B


@pytest.mark.parametrize("n,B,d,nrhs", [c for c in C.POST_TABLE if c[1] != 2 or c[0] == C.BROKEN_N])   # B = 2: the first two of the 16
def test_posterior_reference(n, B, d, nrhs):
    X, Y, F = C.posterior_case(n, B, d, nrhs)
    X2, Y2, F2 = C.posterior_case(n, 2, d, nrhs)
    assert torch.equal(X[:2], X2) and torch.equal(Y[:2], Y2) and torch.equal(F, F2)
    Kyy = C.cos_kernel64(Y.double(), Y.double(), C.ABI_T, C.ABI_EPS) + C.ABI_SIGMA * torch.eye(n, dtype=torch.float64)
    cond = _cond(Kyy)
    ref, alt = C.posterior_ref(n, B, d, nrhs), C.ref_posterior(X, Y, F, C.ABI_SIGMA, C.ABI_T, C.ABI_EPS, chol=True)
    assert ref.shape == (B, n, nrhs) and torch.isfinite(ref).all()
    agree = ((ref - alt).abs().amax((1, 2)) / ref.abs().amax((1, 2))).max().item()
    print(f"[gp case] posterior n={n} B={B} d={d} nrhs={nrhs}: cond {cond:.3g} (cap {C.COND_CAP:g}), LU vs Cholesky {agree:.2e} of scale "
          f"(cap 2^-30 = {C.REF_AGREE:.2e})")
    assert cond <= C.COND_CAP and agree <= C.REF_AGREE
    # the batched reference is the per-matrix one (tests/test_gpu_gp_pins.py calls it with [n, d] rows)
    assert (C.ref_posterior(X[B - 1], Y[B - 1], F, C.ABI_SIGMA, C.ABI_T, C.ABI_EPS) - ref[B - 1]).abs().max() <= C.REF_AGREE * ref[B - 1].abs().max()


@pytest.mark.parametrize("kind", ["negdiag", "nan"])
def test_broken_solve_cases_are_rejected_by_the_reference(kind):
    K, _ = C.broken_solve_case(kind)
    assert torch.equal(K.nan_to_num(7.0), K.transpose(1, 2).nan_to_num(7.0))
    assert C.cholesky_rejects(K) == [b == C.BROKEN_AT for b in range(C.BROKEN_B)]
    k0 = C.BROKEN_N // 64 * 64
    assert kind != "negdiag" or (K[C.BROKEN_AT].diagonal()[k0:] < 0).sum() == 1 and (K[C.BROKEN_AT].diagonal()[:k0] > 0).all()


def test_broken_posterior_case_is_rejected_by_the_reference():
    X, Y, F = C.broken_posterior_case()
    assert torch.isfinite(X).all() and torch.isfinite(F).all()
    assert torch.isnan(Y).any(-1).sum(-1).tolist() == [int(b == C.BROKEN_AT) for b in range(C.BROKEN_B)]
    Kyy = C.cos_kernel64(Y.double(), Y.double()) + 0.1 * torch.eye(C.BROKEN_N, dtype=torch.float64)
    assert C.cholesky_rejects(Kyy) == [b == C.BROKEN_AT for b in range(C.BROKEN_B)]


def test_indefinite_posterior_case_is_rejected_by_the_reference():
    _, Y, _ = C.posterior_case(C.BROKEN_N, C.BROKEN_B, 3, C.NRHS)
    Kyy = C.cos_kernel64(Y.double(), Y.double()) + C.INDEFINITE_SIGMA * torch.eye(C.BROKEN_N, dtype=torch.float64)
    assert torch.isfinite(Kyy).all() and (Kyy.diagonal(dim1=1, dim2=2) > 0).all()
    assert C.cholesky_rejects(Kyy) == [True] * C.BROKEN_B
