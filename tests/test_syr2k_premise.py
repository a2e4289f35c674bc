"""The premise gemmul8_syr2k rests on, pinned on the CPU oracle.  A B^T + B A^T = P Q^T with P = [A, Z, B, Z] and Q = [B, Z, A, Z] along k, Z = the zero
columns that bring k to kh = pad256(k) (trans = T: everything transposed, P^T Q).  In that GEMM -- (N, T) or (T, N), plain transpose for the complex types
too -- row i of P and row i of Q hold the same elements, so
  * the two sides have equal shifts;
  * Q's residue planes (and, accurate mode, its bound planes) are P's with the two K halves swapped;
  * the bound product is symmetric (rowmax == colmax) and C is bitwise symmetric.
The driver therefore computes one shift per row and writes every quantised element twice.  If a case fails here the contract is wrong.

Error classes: the float64 / complex128 product A B^T + B A^T is the reference, the error is taken relative to its largest entry.  The issue that introduced
the routine measured 1e-7 (S / C, 7 moduli) and 1e-15 (D / Z, 14 moduli) in accurate mode, 1e-4 and 1e-12 in fast mode; the assertions below allow one
decade above each class."""
import numpy as np
import pytest

import oracle_lib as ol

DTS = [np.float32, np.float64, np.complex64, np.complex128]
SHAPES = [(5, 1), (37, 65), (300, 129), (70, 300)]


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    if np.dtype(dt).kind == "c":
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    return a.astype(dt)


def concat(A, B, trans):
    """P = [A, Z, B, Z] and Q = [B, Z, A, Z] as stored for `trans` (N: n x 2 kh, T: 2 kh x n)"""
    n, k = A.shape if trans == "N" else A.shape[::-1]
    kh = (k + 255) // 256 * 256
    P, Q = (np.zeros((n, 2 * kh) if trans == "N" else (2 * kh, n), A.dtype) for _ in range(2))
    if trans == "N":
        P[:, :k], P[:, kh:kh + k], Q[:, :k], Q[:, kh:kh + k] = A, B, B, A
    else:
        P[:k], P[kh:kh + k], Q[:k], Q[kh:kh + k] = A, B, B, A
    return P, Q, kh


@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_q_side_is_the_p_side_with_swapped_halves(dt, trans, fast):
    rng = np.random.default_rng(23)
    single = np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4
    N = 7 if single else 14
    limit = 10 * ((1e-4 if single else 1e-12) if fast else (1e-7 if single else 1e-15))
    opB = "T" if trans == "N" else "N"
    for n, k in SHAPES:
        shape = (n, k) if trans == "N" else (k, n)
        A, B = _rand(rng, shape, dt), (8 * _rand(rng, shape, dt)).astype(dt)
        P, Q, kh = concat(A, B, trans)
        C, it = ol.gemm(P, Q, N, fastmode=fast, opA=trans, opB=opB, want_intermediates=True)
        assert np.array_equal(it["sftA"], it["sftB"]), (n, k)
        for lo, hi in ((slice(0, k), slice(kh, kh + k)), (slice(kh, kh + k), slice(0, k))):
            assert np.array_equal(it["A_lo"][..., lo], it["B_lo"][..., hi]), (n, k)
        assert not it["A_lo"][..., k:kh].any() and not it["A_lo"][..., kh + k:].any(), (n, k)
        Cb = np.ascontiguousarray(C).view(np.uint8).reshape(n, n, -1)
        assert np.array_equal(Cb, Cb.transpose(1, 0, 2)), (n, k)
        wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
        Aw, Bw = A.astype(wide), B.astype(wide)
        ref = Aw @ Bw.T + Bw @ Aw.T if trans == "N" else Aw.T @ Bw + Bw.T @ Aw
        err = np.abs(np.asarray(C).astype(wide) - ref).max() / np.abs(ref).max()
        assert err < limit, (n, k, err)
        if not fast:   # the bound planes, their preliminary shifts and the maxima of the bound product
            ba, s0a = ol.extract_bounds(P, trans, True)
            bb, s0b = ol.extract_bounds(Q, opB, False)
            assert np.array_equal(s0a, s0b), (n, k)
            assert np.array_equal(ba[..., :k], bb[..., kh:kh + k]) and np.array_equal(ba[..., kh:kh + k], bb[..., :k]), (n, k)
            rm, cm = ol.bound_maxima(ba, bb)
            assert np.array_equal(rm, cm), (n, k)
