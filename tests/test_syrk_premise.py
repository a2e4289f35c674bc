"""The premise gemmul8_syrk rests on, pinned on the CPU oracle: in the GEMM of A with its own transpose -- (N, T) for A A^T, (T, N) for A^T A, plain
transpose for the complex types too -- the B side IS the A side: equal shifts, equal residue planes (which the bound planes are rounded from the same
way), and a bitwise symmetric C.  The driver therefore quantises A once and aliases B's planes and shifts to A's.  If a case fails here its contract
is wrong and the aliasing must not be used for it."""
import numpy as np
import pytest

import oracle_lib as ol

DTS = [np.float32, np.float64, np.complex64, np.complex128]


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    if np.dtype(dt).kind == "c":
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    return a.astype(dt)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("dt", DTS)
def test_b_side_of_a_at_is_the_a_side(dt, trans, fast):
    rng = np.random.default_rng(11)
    N = 7
    for n in (5, 37, 300):
        for k in (1, 65, 700):
            A = _rand(rng, (n, k) if trans == "N" else (k, n), dt)
            C, it = ol.gemm(A, A, N, fastmode=fast, opA=trans, opB="T" if trans == "N" else "N", want_intermediates=True)
            assert np.array_equal(it["sftA"], it["sftB"]), (n, k)
            assert np.array_equal(it["A_lo"], it["B_lo"]), (n, k)
            Cb = np.ascontiguousarray(C).view(np.uint8).reshape(n, n, -1)
            assert np.array_equal(Cb, Cb.transpose(1, 0, 2)), (n, k)
            if not fast:   # the bound planes and their preliminary shifts
                ba, s0a = ol.extract_bounds(A, trans, True)
                bb, s0b = ol.extract_bounds(A, "T" if trans == "N" else "N", False)
                assert np.array_equal(ba, bb) and np.array_equal(s0a, s0b), (n, k)
                rm, cm = ol.bound_maxima(ba, bb)
                assert np.array_equal(rm, cm), (n, k)
