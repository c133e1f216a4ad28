"""Seeded inputs and fp64 references of the GP solver tests: shared by tests/test_gp_cases_cpu.py (which judges them with torch on the
host alone), tests/test_gpu_gp_solve_edges.py and tests/test_gpu_gp_pins.py.  Nothing here touches a device; every case is built once
and frozen (the tests clone before they modify).

The bound of the GPU tests, TOL = 2^-23 of max|reference|, is derived, not measured: csrc/gp_solve.hip computes in fp64 and rounds ONCE
to fp32, at most 2^-24 |x| per element; its own fp64 error is cond * 2^-53 ~ 1e-11 of scale for cond <= COND_CAP, as is the
reference's (test_gp_cases_cpu.py holds two independent fp64 solves to 2^-30 of scale of each other).  2^-23 is twice the rounding
term: one fp32 ulp of headroom.

gim_gp_posterior_f64 takes T, eps and sigma as C floats, so the kernel computes with float32(0.2) = 0.2 (1 + 1.5e-8) etc.; an fp64
reference fed Python's 0.2 / 1e-6 / 0.1 differs from it by up to 2.6e-8 of max|mu| on the cases here (measured on the host, n = 321,
d = 3) -- a difference of INPUTS, forty times the 2^-30 the bound's derivation allows for everything but the final rounding.
posterior_ref therefore hands ref_posterior the values the ABI carries (ABI_T, ABI_EPS, ABI_SIGMA), as ref_solve takes the fp32
matrix the kernel receives; ref_posterior's own defaults stay the reference formula's."""
import functools

import numpy as np
import torch

TOL = 2.0 ** -23
COND_CAP = 1e5
REF_AGREE = 2.0 ** -30
ABI_SIGMA, ABI_T, ABI_EPS = (float(np.float32(v)) for v in (0.1, 0.2, 1e-6))     # what a C float carries of the GP's constants
SPD_C = 8                                   # feature columns of spd_case
NRHS = 65
# gp_solve over the Cholesky blocks (64 rows) and the pair tree of the L^-1 doubling levels
SOLVE_NS = (1, 17, 63, 64, 65, 127, 128, 129, 192, 193, 320, 321, 577)
LAYOUT_N, LAYOUT_NRHS = 129, (1, 64, 65, 256)
BATCH_N, MAX_B = 65, 16
POST_NS, POST_DS, POST_NRHS, POST_BS = (1, 64, 65, 129, 193, 321), (3, 32, 70), (1, 65), (2, 16)
INDEFINITE_SIGMA = -0.5                     # K_yy + sigma I with this sigma: finite, symmetric, not positive definite
BROKEN_N, BROKEN_B, BROKEN_AT = 150, 3, 1   # blocks of 64 + 64 + 22 rows: the bad pivots sit in the ragged last block / the middle one

# every (n, B, nrhs) a gp_solve test runs, every (n, B, d, nrhs) a gp_posterior_f64 test runs: what the CPU test walks
SOLVE_TABLE = tuple(dict.fromkeys([(n, 2, NRHS) for n in SOLVE_NS] + [(LAYOUT_N, 2, r) for r in LAYOUT_NRHS] +
                                  [(BATCH_N, MAX_B, NRHS), (193, MAX_B, NRHS), (BROKEN_N, BROKEN_B, NRHS)]))
POST_TABLE = tuple(dict.fromkeys([(n, B, d, r) for n in POST_NS for d in POST_DS for r in POST_NRHS for B in POST_BS] +
                                 [(BROKEN_N, BROKEN_B, 32, NRHS)]))


def cos_kernel64(a, b, T=0.2, eps=1e-6):
    """exp((cos(a_i, b_j) - 1) / T) in fp64, rows [..., n, d] (CosKernel of dkm.py:135-144)"""
    c = a @ b.transpose(-1, -2) / (a.norm(dim=-1)[..., :, None] * b.norm(dim=-1)[..., None, :] + eps)
    return ((c - 1.0) / T).exp()


@functools.lru_cache(maxsize=None)
def spd_case(n, B, C, seed, nrhs=NRHS):
    """K [B,n,n] fp32: exp-cosine kernel of seeded rows [B,n,C] + 0.1 I, rounded to fp32 and made exactly symmetric by mirroring the
    lower triangle; a different matrix in every batch entry.  The rows scatter around one direction per matrix (cosines ~0.8), which
    puts the condition number at a few times n, the regime of the GP's own matrices (~2e4 at n = 2352).  F [B,n,nrhs] fp32."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(B, 1, C, generator=g, dtype=torch.float64) + 0.5 * torch.randn(B, n, C, generator=g, dtype=torch.float64)
    K = (cos_kernel64(rows, rows) + 0.1 * torch.eye(n, dtype=torch.float64)).float()
    K = torch.tril(K) + torch.tril(K, -1).transpose(1, 2)
    F = torch.randn(B, n, nrhs, generator=g)
    assert torch.equal(K, K.transpose(1, 2)) and (B == 1 or not torch.equal(K[0], K[1]) or n == 1)
    return K, F


def solve_case(n, B, nrhs=NRHS):
    return spd_case(n, B, SPD_C, 7000 + n, nrhs)


def ref_solve(K, F):
    """THE reference of gp_solve: the fp64 (LU) solve of the same fp32 matrix the kernel receives -> [B,n,nrhs] fp64"""
    return torch.linalg.solve(K.double(), F.double())


def ref_solve_chol(K, F):
    """an independent fp64 route to the same numbers (Cholesky factor + two substitutions)"""
    return torch.cholesky_solve(F.double(), torch.linalg.cholesky(K.double()))


@functools.lru_cache(maxsize=None)
def solve_ref(n, B, nrhs=NRHS):
    return ref_solve(*solve_case(n, B, nrhs))


def ref_posterior(xr, yr, fr, sigma=0.1, T=0.2, eps=1e-6, chol=False):
    """mu = K_xy (K_yy + sigma I)^-1 f in fp64 from fp32 feature rows [n, d] or [B, n, d] (cos kernel of dkm.py:135-144); fr [n, nrhs]
    is shared by the batch.  chol: solve through a Cholesky factor instead of LU (the CPU test's cross-check)."""
    x, y, f = xr.double(), yr.double(), fr.double()
    Kyy = cos_kernel64(y, y, T, eps) + sigma * torch.eye(y.shape[-2], dtype=torch.float64)
    f = f.expand(*y.shape[:-2], *f.shape)
    sol = torch.cholesky_solve(f, torch.linalg.cholesky(Kyy)) if chol else torch.linalg.solve(Kyy, f)
    return cos_kernel64(x, y, T, eps) @ sol


@functools.lru_cache(maxsize=None)
def posterior_case(n, B, d, nrhs):
    """X, Y [B,n,d] fp32 query / support rows, F [n,nrhs] fp32.  Every query row is a noisy copy of a support row (its neighbour's),
    so that K_xy has entries near 1 away from the diagonal, as between two views of one scene."""
    g = torch.Generator().manual_seed(9000 + 1000 * d + n)
    Y = torch.randn(MAX_B, n, d, generator=g)[:B].contiguous()          # drawn for MAX_B: entry b is the same matrix at every B
    X = (Y.roll(1, 1) + 0.3 * torch.randn(MAX_B, n, d, generator=g)[:B]).contiguous()
    F = torch.randn(n, nrhs, generator=torch.Generator().manual_seed(9500 + nrhs + n))
    return X, Y, F


@functools.lru_cache(maxsize=None)
def posterior_ref(n, B, d, nrhs):
    return ref_posterior(*posterior_case(n, B, d, nrhs), ABI_SIGMA, ABI_T, ABI_EPS)


# ---------------------------------------------------------------------------------------- inputs the reference rejects too
def broken_solve_case(kind):
    """solve_case(BROKEN_N, BROKEN_B) with entry BROKEN_AT spoilt.  'negdiag': one negative diagonal entry in the ragged last Cholesky
    block; 'nan': one NaN (mirrored) below the diagonal of the middle block row."""
    K, F = solve_case(BROKEN_N, BROKEN_B)
    K = K.clone()
    if kind == "negdiag":
        K[BROKEN_AT, 140, 140] = -1.0
    elif kind == "nan":
        K[BROKEN_AT, 70, 3] = K[BROKEN_AT, 3, 70] = float("nan")
    else:
        raise KeyError(kind)
    return K, F


def broken_posterior_case():
    """posterior_case(BROKEN_N, BROKEN_B, 32, NRHS) with one NaN support row in direction BROKEN_AT"""
    X, Y, F = posterior_case(BROKEN_N, BROKEN_B, 32, NRHS)
    Y = Y.clone()
    Y[BROKEN_AT, 77] = float("nan")
    return X, Y, F


def cholesky_rejects(K):
    """per batch entry: does torch.linalg.cholesky (fp64, host) raise?"""
    out = []
    for b in range(K.shape[0]):
        try:
            torch.linalg.cholesky(K[b].double())
            out.append(False)
        except torch.linalg.LinAlgError:
            out.append(True)
    return out
