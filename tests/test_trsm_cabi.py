"""gemmul8_trsm at the boundary, without a GPU: declared, exported, bound by the Python package; its argument errors and degenerate cases are answered
before any HIP call; the workspace rule and the leaf order (include/gemmul8_c.h)."""
import ctypes as C
import os
import re

import numpy as np

import gemmul8_amd as g
import trsm_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NUM, E_ARG, E_UNSUP = -1, -2, -3


def _call(dtype=g.D, backend=g.INT8, side=0, uplo=0, trans=0, diag=0, m=4, n=4, alpha=True, A=True, B=True, work=True, N=14, tm=None):
    a = np.zeros(64)
    p = a.ctypes.data
    return g.lib().gemmul8_trsm(None, dtype, backend, side, uplo, trans, diag, m, n, p if alpha else None, p if A else None, 4, p if B else None, 4,
                                N, 0, p if work else None, tm)


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gemmul8_c.h")).read()
    assert re.search(r"GEMMUL8_API\s+int\s+gemmul8_trsm\s*\(", hdr)
    assert re.search(r"GEMMUL8_API\s+size_t\s+gemmul8_trsm_work_size\s*\(", hdr)
    assert re.search(r"GEMMUL8_API\s+int\s+gemmul8_trsm_leaf\s*\(\s*void\s*\)", hdr)
    for name in ("gemmul8_trsm", "gemmul8_trsm_work_size", "gemmul8_trsm_leaf"):
        assert hasattr(g.lib(), name) and name in g.EXPORTS
    assert len(g.lib().gemmul8_trsm.argtypes) == 18 and len(g.lib().gemmul8_trsm_work_size.argtypes) == 6
    assert re.search(r"#define GEMMUL8_ABI_VERSION 7\b", hdr) and g.lib().gemmul8_abi_version() == 7   # no struct or existing signature changed
    assert callable(g.trsm) and callable(g.trsm_work_size)


def test_the_leaf_order_is_read_from_the_library():
    assert g.lib().gemmul8_trsm_leaf() in (64, 128)
    assert g.TRSM_LEAF == g.lib().gemmul8_trsm_leaf()


def test_argument_errors_without_gpu():
    assert _call(side=2) == E_ARG and _call(side=-1) == E_ARG and _call(side=143) == E_ARG and _call(side=140) == E_ARG
    assert _call(uplo=2) == E_ARG and _call(uplo=123) == E_ARG and _call(uplo=-1) == E_ARG
    assert _call(trans=3) == E_ARG and _call(trans=-1) == E_ARG and _call(trans=110) == E_ARG and _call(trans=114) == E_ARG
    assert _call(diag=2) == E_ARG and _call(diag=-1) == E_ARG and _call(diag=130) == E_ARG and _call(diag=133) == E_ARG
    for name in ("alpha", "A", "B", "work"):
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
    # the order of the answers, as in gemmul8_trmm: an argument error before the moduli range, the moduli range before a null pointer, the order of A and
    # the backend; the order of A before the backend
    assert _call(side=2, N=1) == E_ARG and _call(N=1, backend=g.FP8) == E_NUM and _call(N=1, A=False) == E_NUM and _call(N=1, m=big) == E_NUM
    assert _call(A=False, backend=g.FP8, N=8) == E_ARG and _call(m=big, backend=g.FP8, N=8) == E_ARG


def test_empty_calls_succeed_with_every_enum_spelling_and_all_four_types():
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


def test_workspace_is_the_largest_gemms_plus_the_tail():
    L = g.TRSM_LEAF
    for cplx in (False, True):
        for m, n in ((1, 1), (L, 64), (L + 1, 33), (33, L + 1), (2 * L + 1, 40), (600, 300), (70, 1100), (1100, 70)):
            for side in "LR":
                shapes = su.gemm_shapes(m, n, side, L)
                assert bool(shapes) == ((m if side == "L" else n) > L)
                need = max([g.work_size(cplx, g.INT8, gm, gn, gk, 7)[0] for gm, gn, gk in shapes], default=0)
                want = (need + 63) // 64 * 64 + 64
                assert g.trsm_work_size(cplx, m, n, side, 7) == want, (cplx, m, n, side)
                assert g.lib().gemmul8_trsm_work_size(int(cplx), g.INT8, 141 + g.SIDE[side], m, n, 7) == want   # the hipBLAS spelling
