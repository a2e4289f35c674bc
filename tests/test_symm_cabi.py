"""gemmul8_symm / gemmul8_hemm at the boundary, without a GPU: declared, exported, bound by the Python package, and their argument errors and
degenerate cases are answered before any HIP call (include/gemmul8_c.h)."""
import os
import re

import numpy as np
import pytest

import gemmul8_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NUM, E_ARG, E_UNSUP = -1, -2, -3


def _call(fn="gemmul8_symm", dtype=g.D, backend=g.INT8, side=0, uplo=0, m=4, n=4, alpha=True, A=True, B=True, beta=True, Cm=True, work=True, N=14):
    a = np.zeros(64)
    p = a.ctypes.data
    if fn == "gemmul8_hemm" and dtype == g.D:
        dtype = g.Z
    return getattr(g.lib(), fn)(None, dtype, backend, side, uplo, m, n, p if alpha else None, p if A else None, 4, p if B else None, 4,
                                p if beta else None, p if Cm else None, 4, N, 0, p if work else None, None)


FNS = ["gemmul8_symm", "gemmul8_hemm"]


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gemmul8_c.h")).read()
    for fn in FNS:
        assert re.search(r"GEMMUL8_API\s+int\s+" + fn + r"\s*\(", hdr)
        assert hasattr(g.lib(), fn) and fn in g.EXPORTS
        assert len(getattr(g.lib(), fn).argtypes) == 19
    assert re.search(r"GEMMUL8_LEFT\s*=\s*0\s*,\s*GEMMUL8_RIGHT\s*=\s*1", hdr)
    assert re.search(r"#define GEMMUL8_ABI_VERSION 7\b", hdr) and g.ABI_VERSION == 7   # no struct or existing signature changed
    assert g.lib().gemmul8_abi_version() == 7
    assert callable(g.symm) and callable(g.hemm) and callable(g.symm_work_size)


@pytest.mark.parametrize("fn", FNS)
def test_argument_errors_without_gpu(fn):
    assert _call(fn, side=2) == E_ARG and _call(fn, side=-1) == E_ARG and _call(fn, side=143) == E_ARG and _call(fn, side=140) == E_ARG
    assert _call(fn, uplo=2) == E_ARG and _call(fn, uplo=123) == E_ARG and _call(fn, uplo=-1) == E_ARG
    for name in ("alpha", "A", "B", "beta", "Cm", "work"):
        assert _call(fn, **{name: False}) == E_ARG, name
    big = (1 << 17) + 1
    assert _call(fn, side=0, m=big) == E_ARG and _call(fn, side=141, m=big) == E_ARG      # the order of A is m on the left ...
    assert _call(fn, side=1, n=big) == E_ARG and _call(fn, side=142, n=big) == E_ARG      # ... and n on the right
    assert _call(fn, side=0, m=big, n=0) == E_ARG and _call(fn, side=1, n=big, m=0) == E_ARG
    assert _call(fn, side=0, m=0, n=big) == 0 and _call(fn, side=1, n=0, m=big) == 0      # the other dimension has no such limit
    assert _call(fn, side=0, m=1 << 17, n=0) == 0
    assert _call(fn, dtype=4) == E_ARG and _call(fn, dtype=-1) == E_ARG and _call(fn, backend=2) == E_ARG and _call(fn, backend=-1) == E_ARG
    assert _call(fn, N=1) == E_NUM and _call(fn, N=21) == E_NUM and _call(fn, dtype=g.Cx, N=14) == E_NUM
    for dt in ((g.S, g.D, g.Cx, g.Z) if fn == "gemmul8_symm" else (g.Cx, g.Z)):
        assert _call(fn, dtype=dt, backend=g.FP8, N=8) == E_UNSUP


def test_symm_takes_four_types_and_hemm_the_complex_ones():
    assert _call("gemmul8_symm", dtype=g.S, N=14) == E_NUM     # (a type's moduli range is checked: the type was accepted)
    for dt in (g.S, g.D, g.Cx, g.Z):
        assert _call("gemmul8_symm", dtype=dt, N=7, m=0) == 0
    lib = g.lib()
    a = np.zeros(64)
    p = a.ctypes.data
    for dt in (g.S, g.D):   # BLAS has no real HEMM
        for m in (0, 4):
            assert lib.gemmul8_hemm(None, dt, g.INT8, 0, 0, m, 4, p, p, 4, p, 4, p, p, 4, 7, 0, p, None) == E_ARG
    for dt in (g.Cx, g.Z):
        assert lib.gemmul8_hemm(None, dt, g.INT8, 0, 0, 0, 4, p, p, 4, p, 4, p, p, 4, 7, 0, p, None) == 0


@pytest.mark.parametrize("fn", FNS)
def test_empty_products_succeed_and_accept_both_enum_spellings(fn):
    for side in (0, 1, 141, 142):
        for uplo in (0, 1, 121, 122):
            assert _call(fn, side=side, uplo=uplo, m=0) == 0
            assert _call(fn, side=side, uplo=uplo, n=0) == 0
            assert _call(fn, side=side, uplo=uplo, m=0, n=0) == 0


def test_timers_are_zeroed_by_a_call_that_does_nothing():
    import ctypes as C
    a = np.zeros(64)
    p = a.ctypes.data
    tm = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert g.lib().gemmul8_symm(None, g.D, g.INT8, 0, 0, 0, 4, p, p, 4, p, 4, p, p, 4, 14, 0, p, tm) == 0
    assert list(tm) == [0.0, 0.0, 0.0, 0.0]


def test_workspace_is_the_equivalent_gemms():
    for cplx in (False, True):
        for m, n in ((1, 1), (300, 257), (700, 64), (64, 1100)):
            assert g.symm_work_size(cplx, m, n, "L", 7) == g.work_size(cplx, g.INT8, m, n, m, 7)[0]
            assert g.symm_work_size(cplx, m, n, "R", 7) == g.work_size(cplx, g.INT8, m, n, n, 7)[0]
