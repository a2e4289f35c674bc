"""gemmul8_her2k at the boundary, without a GPU: declared, exported, bound by the Python package, and its argument errors and degenerate
cases are answered before any HIP call, with a null stream (include/gemmul8_c.h)."""
import os
import re

import numpy as np

import gemmul8_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(dtype=g.Z, backend=g.INT8, uplo=0, trans=0, n=4, k=4, alpha=True, A=True, B=True, beta=True, Cm=True, work=True, N=14):
    a = np.zeros(64)
    p = a.ctypes.data
    return g.lib().gemmul8_her2k(None, dtype, backend, uplo, trans, n, k, p if alpha else None, p if A else None, 4, p if B else None, 4,
                                 p if beta else None, p if Cm else None, 4, N, 0, p if work else None, None)


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gemmul8_c.h")).read()
    assert re.search(r"GEMMUL8_API\s+int\s+gemmul8_her2k\s*\(", hdr)
    assert re.search(r"#define GEMMUL8_ABI_VERSION 7\b", hdr) and g.ABI_VERSION == 7   # no struct or existing signature changed
    assert g.lib().gemmul8_abi_version() == 7
    assert hasattr(g.lib(), "gemmul8_her2k") and "gemmul8_her2k" in g.EXPORTS and callable(g.her2k) and callable(g.her2k_work_size)
    assert len(g.lib().gemmul8_her2k.argtypes) == 19 and g.lib().gemmul8_her2k.argtypes == g.lib().gemmul8_syr2k.argtypes


def test_argument_errors_without_gpu():
    E_NUM, E_ARG, E_UNSUP = -1, -2, -3
    assert _call(dtype=g.S, N=7) == E_ARG and _call(dtype=g.D) == E_ARG   # BLAS has no real HER2K
    assert _call(uplo=2) == E_ARG and _call(uplo=123) == E_ARG and _call(uplo=-1) == E_ARG
    assert _call(trans=1) == E_ARG and _call(trans=112) == E_ARG and _call(trans=5) == E_ARG   # no plain transpose: HER2K, not SYR2K
    for name in ("alpha", "A", "B", "beta", "Cm", "work"):
        assert _call(**{name: False}) == E_ARG, name
    assert _call(k=(1 << 17) + 1) == E_ARG and _call(k=(1 << 17) + 1, n=0) == E_ARG
    assert _call(k=1 << 17, n=0) == 0   # the equivalent GEMM's limit, not SYR2K's 2^16
    assert _call(dtype=4) == E_ARG and _call(dtype=-1) == E_ARG and _call(backend=2) == E_ARG and _call(backend=-1) == E_ARG
    assert _call(N=1) == E_NUM and _call(N=21) == E_NUM and _call(dtype=g.Cx, N=14) == E_NUM
    for dt in (g.Cx, g.Z):
        assert _call(dtype=dt, backend=g.FP8, N=8) == E_UNSUP


def test_empty_products_succeed_and_accept_the_hipblas_enums():
    for dt, N in ((g.Cx, 7), (g.Z, 14)):
        for uplo in (0, 1, 121, 122):
            for trans in (0, 2, 111, 113):
                assert _call(dtype=dt, N=N, uplo=uplo, trans=trans, n=0) == 0
                assert _call(dtype=dt, N=N, uplo=uplo, trans=trans, k=0) == 0


def test_workspace_is_the_equivalent_gemms():
    for n, k in ((1, 1), (300, 257), (700, 1100)):
        assert g.her2k_work_size(n, k, 7) == g.work_size(True, g.INT8, n, n, k, 7)[0]
