"""The premise gemmul8_her2k rests on, pinned on the CPU oracle.  alpha A B^H + conj(alpha) B A^H is alpha W + (alpha W)^H with W = A B^H, ONE ordinary
GEMM -- (N, C) or (C, N) -- so the stored entry (i, j) follows from W_ij and W_ji by the contract formula (tests/her2k_util.py):
  * the formula is Hermitian by construction: with beta = 0 the uplo = U result equals (==, zero signs aside) the conjugate transpose of the L result,
    although W itself is not bitwise Hermitian-related to anything;
  * A and B keep their own shifts and the result has the accuracy class of the library's complex GEMM.

Error classes (accurate mode, A and B of comparable scale): against the exact A B^H + B A^H, relative to its largest entry, the issue that introduced the
routine set 1e-6 for complex64 with 7 moduli and 1e-14 for complex128 with 14; measured on the oracle at the shapes below: 1e-7 and 7e-16 at the most."""
import numpy as np
import pytest

import her2k_util as hu
import oracle_lib as ol

SHAPES = [(5, 1), (37, 65), (130, 129), (70, 300)]
CASES = [(np.complex64, 7, 1e-6), (np.complex128, 14, 1e-14)]


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-3, 4, shape)) + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-3, 4, shape))
    return a.astype(dt)


def _w(A, B, trans, N, fast=False):
    return np.asarray(ol.gemm(A, B, N, fastmode=fast, opA=trans, opB="C" if trans == "N" else "N"))


@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("dt,N,limit", CASES, ids=["complex64", "complex128"])
def test_upper_is_the_conjugate_transpose_of_lower(dt, N, limit, trans):
    rng = np.random.default_rng(31)
    for n, k in SHAPES:
        shape = (n, k) if trans == "N" else (k, n)
        A, B = _rand(rng, shape, dt), _rand(rng, shape, dt)
        for fast in (False, True):
            W = _w(A, B, trans, N, fast)
            for alpha in (1, -1j, 0.75 - 0.25j, 0.3 + 1.1j):
                R, _ = hu.model(W, alpha, 0)
                L = np.where(hu.tri_mask(n, "L"), R, 0)
                U = np.where(hu.tri_mask(n, "U"), R, 0)
                assert (U == L.conj().T).all(), (n, k, fast, alpha)
                assert not np.signbit(R.imag[np.diag_indices(n)]).any() and not R.imag[np.diag_indices(n)].any()


@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("dt,N,limit", CASES, ids=["complex64", "complex128"])
def test_accuracy_against_the_exact_product(dt, N, limit, trans):
    rng = np.random.default_rng(32)
    worst = 0.0
    for n, k in SHAPES:
        shape = (n, k) if trans == "N" else (k, n)
        A, B = _rand(rng, shape, dt), _rand(rng, shape, dt)
        R, _ = hu.model(_w(A, B, trans, N), 1, 0)
        Aw, Bw = A.astype(np.clongdouble), B.astype(np.clongdouble)
        ref = Aw @ Bw.conj().T + Bw @ Aw.conj().T if trans == "N" else Aw.conj().T @ Bw + Bw.conj().T @ Aw
        err = float(np.abs(R.astype(np.clongdouble) - ref).max() / np.abs(ref).max())
        worst = max(worst, err)
        assert err < limit, (n, k, err)
    print(f"her2k premise {np.dtype(dt).name} N={N} trans={trans}: worst relative error {worst:.3g}")
