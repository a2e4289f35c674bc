"""The premise the gemmul8_symm / gemmul8_hemm contract rests on, pinned on the CPU oracle.  The contract states the side = RIGHT product B * Afull as
the GEMM (N, T) -- HEMM: (N, C) -- of B with Afull, because the symmetric operand then enters the scaling kernels in the row-strided form on either side.
For a symmetric (Hermitian) Afull, op(Afull) = Afull, so that GEMM must be BLAS's B * Afull: in ACCURATE mode, where a row's shift comes from maxima and
every byte is a function of its element and the shift alone, (N, T) / (N, C) gives the same C bits and the same shifts as (N, N).  (The fast mode's
round-up sums depend on the lane an element lands in, which is why the contract names the form; it is not part of the premise.)  If a case fails here the
contract is wrong."""
import numpy as np
import pytest

import oracle_lib as ol
from symm_util import is_cplx, materialise

DTS = [np.float32, np.float64, np.complex64, np.complex128]
SHAPES = [(1, 1), (5, 3), (37, 5), (129, 33), (70, 130)]   # (ka, other dimension)


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    if is_cplx(dt):
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-6, 7, shape))
    return a.astype(dt)


ROUTINES = [(dt, False) for dt in DTS] + [(np.complex64, True), (np.complex128, True)]   # SYMM: four types; HEMM: C / Z


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("dt,herm", ROUTINES, ids=[("hemm-" if h else "symm-") + np.dtype(d).name for d, h in ROUTINES])
def test_right_side_form_gives_the_bits_of_the_plain_product(dt, herm, uplo):
    rng = np.random.default_rng(41)
    single = np.dtype(dt).itemsize // (2 if is_cplx(dt) else 1) == 4
    N = 7 if single else 14
    for ka, other in SHAPES:
        Afull = materialise(_rand(rng, (ka, ka), dt), uplo, herm)
        assert np.array_equal(Afull, Afull.conj().T if herm else Afull.T)
        B = _rand(rng, (other, ka), dt)
        Cn, itn = ol.gemm(B, Afull, N, opA="N", opB="N", want_intermediates=True)
        Ct, itt = ol.gemm(B, Afull, N, opA="N", opB="C" if herm else "T", want_intermediates=True)
        assert np.array_equal(itn["sftA"], itt["sftA"]) and np.array_equal(itn["sftB"], itt["sftB"]), (ka, other)
        assert np.array_equal(np.ascontiguousarray(Cn).view(np.uint8), np.ascontiguousarray(Ct).view(np.uint8)), (ka, other)
