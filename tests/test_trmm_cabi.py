"""gemmul8_trmm at the boundary, without a GPU: declared, exported, bound by the Python package, and its argument errors and degenerate cases are
answered before any HIP call (include/gemmul8_c.h)."""
import ctypes as C
import os
import re

import numpy as np

import gemmul8_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NUM, E_ARG, E_UNSUP = -1, -2, -3


def _call(dtype=g.D, backend=g.INT8, side=0, uplo=0, trans=0, diag=0, m=4, n=4, alpha=True, A=True, B=True, Cm=True, work=True, N=14, tm=None):
    a = np.zeros(64)
    p = a.ctypes.data
    return g.lib().gemmul8_trmm(None, dtype, backend, side, uplo, trans, diag, m, n, p if alpha else None, p if A else None, 4, p if B else None, 4,
                                p if Cm else None, 4, N, 0, p if work else None, tm)


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gemmul8_c.h")).read()
    assert re.search(r"GEMMUL8_API\s+int\s+gemmul8_trmm\s*\(", hdr)
    assert hasattr(g.lib(), "gemmul8_trmm") and "gemmul8_trmm" in g.EXPORTS
    assert len(g.lib().gemmul8_trmm.argtypes) == 20
    assert re.search(r"GEMMUL8_NON_UNIT\s*=\s*0\s*,\s*GEMMUL8_UNIT\s*=\s*1", hdr)
    assert re.search(r"#define GEMMUL8_ABI_VERSION 7\b", hdr) and g.lib().gemmul8_abi_version() == 7   # no struct or existing signature changed
    assert callable(g.trmm) and callable(g.trmm_work_size) and g.DIAG == {"N": 0, "U": 1}


def test_argument_errors_without_gpu():
    assert _call(side=2) == E_ARG and _call(side=-1) == E_ARG and _call(side=143) == E_ARG and _call(side=140) == E_ARG
    assert _call(uplo=2) == E_ARG and _call(uplo=123) == E_ARG and _call(uplo=-1) == E_ARG
    assert _call(trans=3) == E_ARG and _call(trans=-1) == E_ARG and _call(trans=110) == E_ARG and _call(trans=114) == E_ARG
    assert _call(diag=2) == E_ARG and _call(diag=-1) == E_ARG and _call(diag=130) == E_ARG and _call(diag=133) == E_ARG
    for name in ("alpha", "A", "B", "Cm", "work"):
        assert _call(**{name: False}) == E_ARG, name
    big = (1 << 17) + 1
    assert _call(side=0, m=big) == E_ARG and _call(side=141, m=big) == E_ARG      # the order of A is m on the left ...
    assert _call(side=1, n=big) == E_ARG and _call(side=142, n=big) == E_ARG      # ... and n on the right
    assert _call(side=0, m=big, n=0) == E_ARG and _call(side=1, n=big, m=0) == E_ARG
    assert _call(side=0, m=0, n=big) == 0 and _call(side=1, n=0, m=big) == 0      # the other dimension has no such limit
    assert _call(side=0, m=1 << 17, n=0) == 0
    assert _call(dtype=4) == E_ARG and _call(dtype=-1) == E_ARG and _call(backend=2) == E_ARG and _call(backend=-1) == E_ARG
    assert _call(N=1) == E_NUM and _call(N=21) == E_NUM and _call(dtype=g.Cx, N=14) == E_NUM and _call(dtype=g.S, N=14) == E_NUM
    for dt in (g.S, g.D, g.Cx, g.Z):
        assert _call(dtype=dt, backend=g.FP8, N=8) == E_UNSUP
    # the order of the answers: an argument error before the moduli range, the moduli range before the backend
    assert _call(side=2, N=1) == E_ARG and _call(N=1, backend=g.FP8) == E_NUM


def test_empty_products_succeed_with_every_enum_spelling_and_all_four_types():
    for side in (0, 1, 141, 142):
        for uplo in (0, 1, 121, 122):
            for trans in (0, 1, 2, 111, 112, 113):
                for diag in (0, 1, 131, 132):
                    assert _call(side=side, uplo=uplo, trans=trans, diag=diag, m=0) == 0
                    assert _call(side=side, uplo=uplo, trans=trans, diag=diag, n=0) == 0
    for dt in (g.S, g.D, g.Cx, g.Z):
        assert _call(dtype=dt, N=7, m=0, n=0) == 0


def test_timers_are_zeroed_by_a_call_that_does_nothing():
    tm = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert _call(m=0, tm=tm) == 0
    assert list(tm) == [0.0, 0.0, 0.0, 0.0]


def test_workspace_is_the_equivalent_gemms():
    for cplx in (False, True):
        for m, n in ((1, 1), (300, 257), (700, 64), (64, 1100)):
            assert g.trmm_work_size(cplx, m, n, "L", 7) == g.work_size(cplx, g.INT8, m, n, m, 7)[0]
            assert g.trmm_work_size(cplx, m, n, "R", 7) == g.work_size(cplx, g.INT8, m, n, n, 7)[0]
            assert g.trmm_work_size(cplx, m, n, "L", 7) == g.lib().gemmul8_work_size(int(cplx), g.INT8, m, n, m, 7, 0, 0, None, None)
