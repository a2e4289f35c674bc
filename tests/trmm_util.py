"""Helpers of the TRMM tests: the materialised matrices of the contract (include/gemmul8_c.h, gemmul8_trmm) -- Atri, M = op(Atri) and its plain transpose
Mt --, the equivalent GEMM (side L = (N, N) M B, side R = (N, T) B Mt), the poisoned A, and a host mirror of the residue GEMM's per-tile K range
(tile_krange, csrc/oz2_gemm_common.hpp)."""
import numpy as np

from symm_util import is_cplx


def atri(A, uplo, diag):
    """the triangle `uplo` ("L" / "U") of the square numpy matrix A, exact zeros in the other strict triangle, ones on the diagonal under diag "U"
    (the stored diagonal does not enter then)"""
    T = (np.tril(A) if uplo == "L" else np.triu(A)).astype(A.dtype)
    if diag == "U":
        T[np.diag_indices_from(T)] = 1
    return T


def op(T, trans):
    return {"N": T, "T": T.T, "C": T.conj().T}[trans]


def materialise(A, uplo, trans, diag):
    """M = op(Atri)"""
    return np.ascontiguousarray(op(atri(A, uplo, diag), trans))


def equivalent_gemm(A, B, side, uplo, trans, diag):
    """(left, right, opA, opB) of the equivalent GEMM on stored operands"""
    M = materialise(A, uplo, trans, diag)
    return (M, B, "N", "N") if side == "L" else (B, np.ascontiguousarray(M.T), "N", "T")


def poison(A, uplo, diag):
    """A with NaN in everything TRMM must not read: the other strict triangle and, under diag "U", the diagonal"""
    P = A.copy()
    other = np.triu(np.ones(A.shape, bool), 1) if uplo == "L" else np.tril(np.ones(A.shape, bool), -1)
    nan = np.nan + (1j * np.nan if is_cplx(A.dtype) else 0)
    P[other] = nan
    if diag == "U":
        P[np.diag_indices_from(P)] = nan
    return P


# ---- the K-range rule.  KRange values and the function mirror csrc/oz2_gemm_common.hpp line by line.
KR_A_LOWER, KR_A_UPPER, KR_B_HIGH, KR_B_LOW = 1, 2, 3, 4


def m_is_lower(uplo, trans):
    """M = op(Atri) is lower triangular when the stored triangle is the lower one and op = N, or the upper one and op = T / C"""
    return (uplo == "L") == (trans == "N")


def krange_of(side, uplo, trans):
    """the driver's choice (trmm() in csrc/oz2_driver.hip)"""
    low = m_is_lower(uplo, trans)
    if side == "L":
        return KR_A_LOWER if low else KR_A_UPPER
    return KR_B_HIGH if low else KR_B_LOW


def tile_krange(krange, KT, tm, tn):
    t = tm if krange in (KR_A_LOWER, KR_A_UPPER) else tn
    k0, k1 = 0, KT
    if krange in (KR_A_LOWER, KR_B_LOW):
        k1 = min(2 * (t + 1), KT)
    elif krange != 0:
        k0 = 2 * t
    return k0, k1
