"""The premise of gemmul8_trsm, on the CPU: the recipe of include/gemmul8_c.h as tests/trsm_util.py models it -- its split rule, its leaf in both
orientations, its four side / triangle cases -- and the quality of what it computes with the CPU oracle's emulated GEMM as the GEMM.

The residual condition.  Inputs: off-diagonal entries uniform in +-1/ka, diagonal magnitudes in [1, 2] with random sign, alpha = 0.75.  The componentwise
backward error max |M X - alpha B| / (|M||X| + |alpha||B|), taken in longdouble (float64 for the single-precision type), of the recipe with the emulated
GEMM (float64: 14 moduli, float32: 7) is at most 4 times that of the same recursion with its GEMMs done by a plain matmul in the element type.  The factor
is a condition, not a tuned tolerance: the emulated GEMM's own error at these moduli counts (2.5e-14 of |A||B| for float64 at 14 moduli, measured on the same
inputs) enters through the small off-diagonal mass only.  Measured with L = 64 on the cases below: ratios 0.92 .. 1.17, both legs 4.3e-16 .. 8.3e-16
(float64) and 2.5e-7 .. 4.6e-7 (float32)."""
import itertools

import numpy as np
import pytest

import gemmul8_amd as g
import oracle_lib as ol
import trsm_util as su


def _L():
    return g.TRSM_LEAF


# ---- the split rule
def test_split_rule_properties():
    for L in (64, 128):
        for r in list(range(L + 1, 4 * L + 3)) + [600, 1100, 5000, 8192, 1 << 17]:
            h = su.split(r, L)
            assert h % L == 0 and h < r <= 2 * h and (h // L) & (h // L - 1) == 0, (L, r, h)


@pytest.mark.parametrize("ka", [1, 63, 64, 65, 128, 129, 257, 600, 1100, 4097])
def test_the_blocks_tile_the_triangle(ka):
    L = _L()
    for side, lower_m in itertools.product("LR", (True, False)):
        steps = su.plan(ka, L, side, lower_m)
        cover = np.zeros((ka, ka), np.int32)   # [i, j] of M, counted once each over the live triangle
        solved = np.zeros(ka, bool)
        pending = np.ones(ka, bool)            # the scale has not reached these indices of B yet
        for st in steps:
            if st[0] == "leaf":
                _, d0, r, scaled = st
                assert 1 <= r <= L
                i, j = np.indices((r, r))
                cover[d0:d0 + r, d0:d0 + r] += (i >= j) if lower_m else (i <= j)
                assert not solved[d0:d0 + r].any()
                assert (pending[d0:d0 + r] == scaled).all()       # scaled exactly where the scale is still pending
                solved[d0:d0 + r] = True
                pending[d0:d0 + r] = False
            else:
                _, f0, fn, s0, sn, scaled = st
                assert solved[f0:f0 + fn].all() and not solved[s0:s0 + sn].any()    # the update uses final X and reaches unsolved rows only
                assert (pending[s0:s0 + sn] == scaled).all()
                pending[s0:s0 + sn] = False
                rows, cols = ((s0, sn), (f0, fn)) if side == "L" else ((f0, fn), (s0, sn))   # the block of M: [dst, src] left, [src, dst] right
                cover[rows[0]:rows[0] + rows[1], cols[0]:cols[0] + cols[1]] += 1
        i, j = np.indices((ka, ka))
        assert np.array_equal(cover, ((i >= j) if lower_m else (i <= j)).astype(np.int32)), (side, lower_m)
        assert solved.all() and not pending.any()
        assert sum(st[0] == "leaf" for st in steps) == -(-ka // L) and sum(st[0] == "gemm" for st in steps) == -(-ka // L) - 1


# ---- the leaf
TYPES = [np.float32, np.float64, np.complex64, np.complex128]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dt", TYPES, ids=[np.dtype(d).name for d in TYPES])
def test_row_and_column_oriented_leaf_give_the_same_bits(dt):
    rng = np.random.default_rng(5)
    for r, nrhs in ((1, 3), (7, 4), (33, 5)):
        A = su.well_conditioned(rng, r, dt)
        A = (A * 7).astype(dt)    # off-diagonal mass large enough for every subtraction to round
        for left, lower_m, unit, s in itertools.product((True, False), (True, False), (False, True), (None, 0.75 - 0.25j if np.dtype(dt).kind == "c" else -0.3)):
            Bm = su.rhs(rng, (r, nrhs) if left else (nrhs, r), dt)
            M = A.copy()
            dead = np.triu(np.ones((r, r), bool), 1) if lower_m else np.tril(np.ones((r, r), bool), -1)
            M[dead] = np.nan      # never read
            if unit:
                M[np.diag_indices(r)] = np.nan
            rows = su.leaf_rows(M, Bm, s, left, lower_m, unit)
            cols = su.leaf_columns(M, Bm, s, left, lower_m, unit)
            assert np.isfinite(rows).all()
            assert _bits(rows, cols), (r, left, lower_m, unit, s)


def test_leaf_torch_form_equals_numpy_form():
    import torch
    rng = np.random.default_rng(6)
    for dt in TYPES:
        A = (su.well_conditioned(rng, 19, dt) * 5).astype(dt)
        for left, lower_m, unit in itertools.product((True, False), (True, False), (False, True)):
            Bm = su.rhs(rng, (19, 6) if left else (6, 19), dt)
            want = su.leaf_columns(A, Bm, 0.75, left, lower_m, unit)
            got = su.leaf_columns(torch.from_numpy(A), torch.from_numpy(Bm), 0.75, left, lower_m, unit).numpy()
            assert _bits(want, got), (dt, left, lower_m, unit)


# ---- the recursion
def _exact_order_gemm(lhs, rhs, opL, opR, beta, Cm):
    """-op(lhs) op(rhs) + beta C with a fixed k-ascending order in longdouble (numpy's own loop: no BLAS), rounded once: transposing the problem transposes
    the result bit for bit"""
    ld = np.clongdouble if np.iscomplexobj(Cm) else np.longdouble
    P = su.op_block(lhs, opL).astype(ld) @ su.op_block(rhs, opR).astype(ld)
    return (-P + ld(beta) * Cm.astype(ld)).astype(Cm.dtype)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
def test_the_four_cases_are_consistent_under_transposition(dt):
    L = _L()
    rng = np.random.default_rng(8)
    ka, other = 2 * L + 9, 6
    A = su.well_conditioned(rng, ka, dt)
    Bm = su.rhs(rng, (ka, other), dt)
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(Bm.T)
    for uplo, diag in itertools.product("LU", "NU"):
        flip = "U" if uplo == "L" else "L"
        ref = su.solve(A, Bm, 0.75, "L", uplo, "N", diag, L, _exact_order_gemm)
        # op = T on the transposed storage is the same M
        assert _bits(ref, su.solve(At, Bm, 0.75, "L", flip, "T", diag, L, _exact_order_gemm)), (uplo, diag)
        # X M^T = B^T is the transposed problem: RIGHT with the other triangle
        assert _bits(ref, su.solve(At, Bt, 0.75, "R", flip, "N", diag, L, _exact_order_gemm).T), (uplo, diag)
        assert _bits(ref, su.solve(A, Bt, 0.75, "R", uplo, "T", diag, L, _exact_order_gemm).T), (uplo, diag)
        # and it solves the system
        M = np.tril(A) if uplo == "L" else np.triu(A)
        if diag == "U":
            M[np.diag_indices(ka)] = 1
        res = np.abs(M.astype(np.longdouble) @ ref.astype(np.longdouble) - np.longdouble(0.75) * Bm)
        assert res.max() <= 64 * np.finfo(dt).eps * (np.abs(M) @ np.abs(ref) + np.abs(Bm)).max()


# ---- the residual condition
def _backward_error(M, X, alpha, Bm, wide):
    Mw, Xw, Bw = M.astype(wide), X.astype(wide), Bm.astype(wide)
    num = np.abs(Mw @ Xw - wide(alpha) * Bw)
    den = np.abs(Mw) @ np.abs(Xw) + abs(wide(alpha)) * np.abs(Bw)
    return float((num / den).max())


@pytest.mark.parametrize("ka,other", [(65, 5), (257, 40), (600, 33)], ids=["65x5", "257x40", "600x33"])
@pytest.mark.parametrize("dt,N", [(np.float64, 14), (np.float32, 7)], ids=["float64-14", "float32-7"])
def test_residual_condition(dt, N, ka, other):
    L = _L()
    rng = np.random.default_rng(ka * 7 + other)
    wide = np.longdouble if dt == np.float64 else np.float64
    alpha = 0.75
    A = su.well_conditioned(rng, ka, dt)

    def emulated(lhs, rhs, opL, opR, beta, Cm):
        return np.asarray(ol.gemm(lhs, rhs, N, fastmode=False, opA=opL, opB=opR, alpha=-1.0, beta=beta, C0=Cm))

    def plain(lhs, rhs, opL, opR, beta, Cm):
        return (-(su.op_block(lhs, opL) @ su.op_block(rhs, opR)) + dt(beta) * Cm).astype(dt)
    for side, uplo, trans in (("L", "L", "N"), ("R", "U", "N"), ("L", "U", "T")):
        Bm = su.rhs(rng, (ka, other) if side == "L" else (other, ka), dt)
        M = su.op_block(np.tril(A) if uplo == "L" else np.triu(A), trans)
        errs = []
        for gemm in (emulated, plain):
            X = su.solve(A, Bm, alpha, side, uplo, trans, "N", L, gemm)
            errs.append(_backward_error(M, X, alpha, Bm, wide) if side == "L" else _backward_error(M.T, X.T, alpha, Bm.T, wide))
        print(f"{np.dtype(dt).name} {ka}x{other} {side}{uplo}{trans}: emulated {errs[0]:.3e}, plain matmul {errs[1]:.3e}, ratio {errs[0] / errs[1]:.3f}")
        assert errs[0] <= 4 * errs[1], (side, uplo, trans, errs)
