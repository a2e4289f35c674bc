"""The premise gemmul8_herk rests on, pinned on the CPU oracle.  In the GEMM of a complex A with its own conjugate transpose -- (N, C) for A A^H,
(C, N) for A^H A -- the two sides share LESS than in SYRK (tests/test_syrk_premise.py):
  1. the shifts are equal, the bound planes and the maxima of the bound product are symmetric (the bounds take magnitudes), and plane set 0 (Re)
     is equal; plane set 1 of the conjugated side is the byte-wise negation (mod 256) of the other side's (for the modulus 256 the byte -128 maps
     to itself); plane set 2 of the conjugated side holds the residues of Re - Im, which no plane of the other side has.  One operand pass
     therefore writes FIVE plane sets, and the driver aliases shifts, bound planes and plane set 0 only.
  2. Re C is bitwise symmetric and the diagonal of Im C is exactly zero, but Im C is NOT bitwise antisymmetric: the CRT's reduction modulo P is not
     an odd function.  A stored entry is computed as the GEMM computes that entry, never mirrored or negated from the other triangle.
If a case fails here the contract of gemmul8_herk is wrong for it."""
import numpy as np
import pytest

import oracle_lib as ol

DTS = [np.complex64, np.complex128]
CASES = [(dt, N) for dt in DTS for N in ((2, 7, 13) if dt is np.complex64 else (2, 7, 13, 16, 20))]


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    return a.astype(dt)


def _neg_bytes(x):
    return ((256 - x.astype(np.int32)) & 255).astype(np.uint8)


def _not_antisymmetric(C):
    """number of (i, j), i != j, whose Im C[i, j] is not the negation of Im C[j, i] (magnitude bits compared; a zero counts as its own negation)"""
    im = np.ascontiguousarray(C.imag)
    return int((im != -im.T).sum())


@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("dt,N", CASES, ids=[f"{np.dtype(d).name}-N{N}" for d, N in CASES])
def test_what_the_two_sides_of_a_ah_share(dt, N, trans, fast):
    rng = np.random.default_rng(11)
    opB = "C" if trans == "N" else "N"
    for n in (5, 37, 300):
        for k in (1, 65, 700):
            A = _rand(rng, (n, k) if trans == "N" else (k, n), dt)
            C, it = ol.gemm(A, A, N, fastmode=fast, opA=trans, opB=opB, alpha=1.5, want_intermediates=True)
            what = (n, k)
            assert np.array_equal(it["sftA"], it["sftB"]), what
            plain, conj = (it["A_lo"], it["B_lo"]) if trans == "N" else (it["B_lo"], it["A_lo"])
            assert np.array_equal(plain[0], conj[0]), what                      # Re
            assert np.array_equal(conj[1], _neg_bytes(plain[1])), what          # -Im: the byte-wise negation
            assert np.array_equal(np.ascontiguousarray(C.real).view(np.uint8), np.ascontiguousarray(C.real.T).view(np.uint8)), what   # Re C: bitwise symmetric
            assert not np.diagonal(C).imag.any(), what                          # the diagonal of Im C: exactly zero
            if not fast:   # the bound planes and their preliminary shifts
                ba, s0a = ol.extract_bounds(A, trans, True)
                bb, s0b = ol.extract_bounds(A, opB, False)
                assert np.array_equal(ba, bb) and np.array_equal(s0a, s0b), what
                rm, cm = ol.bound_maxima(ba, bb)
                assert np.array_equal(rm, cm), what


def test_im_c_is_not_bitwise_antisymmetric_and_re_minus_im_is_a_plane_of_its_own():
    """Nothing above claims Im C[i, j] == -Im C[j, i], and this case shows why nobody may mirror: complex128, fast mode, 16 moduli, n = 300, k = 65.
    The same case shows the fifth plane set: the conjugated side's Re - Im planes are neither a plane set of the other side nor a negation of one."""
    rng = np.random.default_rng(11)
    A = _rand(rng, (300, 65), np.complex128)
    C, it = ol.gemm(A, A, 16, fastmode=True, opA="N", opB="C", alpha=1.5, want_intermediates=True)
    assert np.array_equal(C.real, C.real.T) and not np.diagonal(C).imag.any()
    assert _not_antisymmetric(C) > 0
    plain, conj = it["A_lo"], it["B_lo"]
    for p in range(3):
        assert not np.array_equal(conj[2], plain[p]) and not np.array_equal(conj[2], _neg_bytes(plain[p]))
