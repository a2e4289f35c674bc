"""Helpers of the SYMM / HEMM tests: the materialised matrix Afull that BLAS defines from one stored triangle, and the equivalent GEMM of the contract
(include/gemmul8_c.h): side L = (N, N) Afull B, side R = (N, T) B Afull for SYMM and (N, C) for HEMM."""
import numpy as np


def is_cplx(dt):
    return np.dtype(dt).kind == "c"


def materialise(A, uplo, herm):
    """Afull from the triangle `uplo` ("L" / "U") of the square numpy matrix A: the mirrored entry is the stored one (herm: its conjugate), herm: the
    diagonal is the real part of the stored diagonal.  Nothing of the other strict triangle enters."""
    T = np.tril(A) if uplo == "L" else np.triu(A)
    S = np.tril(A, -1) if uplo == "L" else np.triu(A, 1)
    F = T + (S.conj().T if herm else S.T)
    if herm:
        F[np.diag_indices_from(F)] = np.diag(A).real
    return np.ascontiguousarray(F.astype(A.dtype))


def equivalent_ops(side, herm):
    """(opA, opB) of the equivalent GEMM"""
    return ("N", "N") if side == "L" else ("N", "C" if herm else "T")


def equivalent_operands(Afull, B, side):
    """(left, right) stored operands of the equivalent GEMM"""
    return (Afull, B) if side == "L" else (B, Afull)


def poison(A, uplo, herm):
    """A with NaN in everything SYMM / HEMM must not use: the other strict triangle and, herm, the diagonal's imaginary parts"""
    P = A.copy()
    other = np.triu(np.ones(A.shape, bool), 1) if uplo == "L" else np.tril(np.ones(A.shape, bool), -1)
    P[other] = np.nan + (1j * np.nan if is_cplx(A.dtype) else 0)
    if herm:
        P.imag[np.diag_indices_from(P)] = np.nan   # (the real parts stay: 1j * nan would be nan + nan j)
    return P
