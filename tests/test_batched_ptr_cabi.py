"""gemmul8_gemm_batched_ptr at the boundary, without a GPU: declared, exported, bound by the Python package; its argument errors and degenerate cases
are answered before any HIP call, in the order gemmul8_gemm_batched answers the same bad arguments (include/gemmul8_c.h)."""
import itertools
import os
import re
import subprocess

import numpy as np

import gemmul8_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NUM, E_ARG, OK = -1, -2, 0
BIG, BIG8 = (1 << 17) + 1, 65537


def _args(dtype=g.D, backend=g.INT8, opA=0, opB=0, m=4, n=4, k=4, alpha=True, A=True, B=True, beta=True, C=True, batch=3, N=14, work=True):
    a = np.zeros(64)
    p = a.ctypes.data
    return a, dict(dtype=dtype, backend=backend, opA=opA, opB=opB, m=m, n=n, k=k, alpha=p if alpha else None, A=p if A else None, B=p if B else None,
                   beta=p if beta else None, C=p if C else None, batch=batch, N=N, work=p if work else None)


def _ptr(**kw):
    keep, a = _args(**kw)
    return g.lib().gemmul8_gemm_batched_ptr(None, a["dtype"], a["backend"], a["opA"], a["opB"], a["m"], a["n"], a["k"], a["alpha"], a["A"], 4, a["B"], 4,
                                            a["beta"], a["C"], 4, a["batch"], a["N"], 0, a["work"])


def _strided(**kw):
    keep, a = _args(**kw)
    return g.lib().gemmul8_gemm_batched(None, a["dtype"], a["backend"], a["opA"], a["opB"], a["m"], a["n"], a["k"], a["alpha"], a["A"], 4, 16, a["B"], 4, 16,
                                        a["beta"], a["C"], 4, 16, a["batch"], a["N"], 0, a["work"])


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gemmul8_c.h")).read()
    m = re.search(r"GEMMUL8_API\s+int\s+gemmul8_gemm_batched_ptr\s*\(([^;]*)\)\s*;", hdr)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 20
    assert re.fullmatch(r"const void \*const \*A_array", params[9]) and re.fullmatch(r"const void \*const \*B_array", params[11])
    assert re.fullmatch(r"void \*const \*C_array", params[14])
    assert "gemmul8_gemm_batched_ptr" in g.EXPORTS and hasattr(g.lib(), "gemmul8_gemm_batched_ptr")
    assert len(g.lib().gemmul8_gemm_batched_ptr.argtypes) == 20
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r" T gemmul8_gemm_batched_ptr$", out, re.M)
    assert re.search(r"#define GEMMUL8_ABI_VERSION 7\b", hdr) and g.lib().gemmul8_abi_version() == 7   # no struct or existing signature changed
    assert callable(g.gemm_batched_ptr)
    # the contract is stated at the declaration
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    for phrase in ("bit-identical", "not validated", "never by the host", "REPLAY", "must not overlap", "alignment of its element type"):
        assert phrase.lower() in doc.lower(), phrase


def test_argument_errors_without_gpu():
    for name in ("A", "B", "C", "alpha", "beta", "work"):
        assert _ptr(**{name: False}) == E_ARG, name
    assert _ptr(dtype=4) == E_ARG and _ptr(dtype=-1) == E_ARG and _ptr(backend=2) == E_ARG and _ptr(backend=-1) == E_ARG
    assert _ptr(N=1) == E_NUM and _ptr(N=21) == E_NUM and _ptr(dtype=g.S, N=14) == E_NUM and _ptr(dtype=g.Cx, N=14) == E_NUM
    assert _ptr(k=BIG) == E_ARG and _ptr(k=BIG, m=0) == E_ARG
    assert _ptr(backend=g.FP8, N=8, k=BIG8) == E_ARG and _ptr(backend=g.FP8, N=8, k=BIG8, batch=0) == E_ARG


def test_degenerate_calls_succeed_and_touch_nothing():
    for zero in ("m", "n", "k", "batch"):
        for dt, N in ((g.S, 7), (g.D, 14), (g.Cx, 8), (g.Z, 15)):
            for backend in (g.INT8, g.FP8):
                assert _ptr(dtype=dt, N=min(N, 12), backend=backend, **{zero: 0}) == OK, (zero, dt, backend)
    assert _ptr(k=1 << 17, m=0) == OK and _ptr(backend=g.FP8, N=8, k=65536, n=0) == OK   # the limits themselves are inside


def test_the_order_of_checks_is_the_strided_forms():
    """Every combination of bad arguments gets the answer gemmul8_gemm_batched gives it (a null array where that one has a null matrix)."""
    bad = {"dtype": dict(dtype=4), "backend": dict(backend=2), "N": dict(N=1), "A": dict(A=False), "C": dict(C=False), "alpha": dict(alpha=False),
           "work": dict(work=False), "k": dict(k=BIG), "m0": dict(m=0), "batch0": dict(batch=0)}
    seen = set()
    for r in (1, 2, 3):
        for combo in itertools.combinations(sorted(bad), r):
            kw = {}
            for name in combo:
                kw.update(bad[name])
            want = _strided(**kw)
            assert want != OK or set(combo) <= {"m0", "batch0"}, combo
            assert _ptr(**kw) == want, (combo, want)
            seen.add(want)
    assert seen == {E_ARG, E_NUM, OK}
    # FP8's shorter k limit sits where the strided form has it: behind the null checks and the general limit, before the degenerate sizes
    for kw in (dict(backend=g.FP8, N=8, k=BIG8), dict(backend=g.FP8, N=8, k=BIG8, m=0), dict(backend=g.FP8, N=13, k=BIG8), dict(backend=g.FP8, N=8, k=BIG8, B=False)):
        assert _ptr(**kw) == _strided(**kw), kw
