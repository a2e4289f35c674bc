"""The recipe of gemmul8_trsm (include/gemmul8_c.h) in Python: the split rule, the recursion -- with the GEMM as a callable -- and the leaf solve, on numpy
arrays or torch tensors alike.  Matrices are in the mathematical layout here, [row, col]; a device tensor of the (cols, rows) convention enters as its .T view.

The leaf model keeps complex numbers as separate real and imaginary arrays and works column-oriented with whole-array multiply / subtract / divide: one
ufunc or torch op is one rounding of the element type, and nothing can be contracted."""
import numpy as np

try:
    import torch
except Exception:  # the CPU tests need numpy only
    torch = None


def is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def m_is_lower(uplo, trans):
    """M = op(Atri) is lower triangular iff (uplo == LOWER) == (transA == N)"""
    return (uplo == "L") == (trans == "N")


def split(r, L):
    """h: the largest L * 2^j strictly below r (r > L)"""
    assert r > L
    h = L
    while 2 * h < r:
        h *= 2
    return h


def plan(ka, L, side, lower_m):
    """The recipe's steps in order: ("leaf", d0, r, scaled) and ("gemm", src0, nsrc, dst0, ndst, scaled), blocks as (first index, order) along the diagonal
    of M; scaled = the caller's alpha is still pending for the block's elements of B."""
    out = []
    first_is_1 = (side == "L") == lower_m   # the substitution runs forwards

    def rec(d0, r, scaled):
        if r <= L:
            out.append(("leaf", d0, r, scaled))
            return
        h = split(r, L)
        f0, fn, s0, sn = (d0, h, d0 + h, r - h) if first_is_1 else (d0 + h, r - h, d0, h)
        rec(f0, fn, scaled)
        out.append(("gemm", f0, fn, s0, sn, scaled))
        rec(s0, sn, False)
    if ka:
        rec(0, ka, True)
    return out


def gemm_shapes(m, n, side, L):
    """(m, n, k) of every GEMM the recipe can run for an m x n B on this side, over both orientations of M (the workspace rule does not know uplo / transA)"""
    ka, other = (m, n) if side == "L" else (n, m)
    out = []
    for lower_m in (True, False):
        for st in plan(ka, L, side, lower_m):
            if st[0] == "gemm":
                _, _, nsrc, _, ndst, _ = st
                out.append((ndst, other, nsrc) if side == "L" else (other, ndst, nsrc))
    return out


# ---- element arithmetic on (re, im) pairs of arrays; im is None for the real types
def _parts(x):
    cplx = x.is_complex() if is_torch(x) else np.iscomplexobj(x)
    if not cplx:
        return (x.clone() if is_torch(x) else x.copy()), None
    return (x.real.clone(), x.imag.clone()) if is_torch(x) else (x.real.copy(), x.imag.copy())


def _join(re, im, like):
    if im is None:
        return re
    if is_torch(re):
        return torch.complex(re.contiguous(), im.contiguous())
    out = np.empty(re.shape, like.dtype)
    out.real, out.imag = re, im
    return out


def _flip(x, axes):
    if x is None:
        return None
    return torch.flip(x, list(axes)) if is_torch(x) else np.flip(x, axes)


def _t(x):
    return None if x is None else x.T


def c_mul(a, b):
    """the textbook product: four products, two sums"""
    (ar, ai), (br, bi) = a, b
    if ai is None:
        return ar * br, None
    return ar * br - ai * bi, ar * bi + ai * br


def c_sub(a, b):
    (ar, ai), (br, bi) = a, b
    return ar - br, (None if ai is None else ai - bi)


def c_div(a, d):
    """the textbook quotient, not scaled"""
    (ar, ai), (dr, di) = a, d
    if ai is None:
        return ar / dr, None
    den = dr * dr + di * di
    return (ar * dr + ai * di) / den, (ai * dr - ar * di) / den


def _scalar_parts(s, like_re, cplx):
    """alpha as (re, im) scalars of the element type's real type"""
    s = complex(s)
    if is_torch(like_re):
        mk = lambda v: torch.tensor(v, dtype=like_re.dtype, device=like_re.device)
    else:
        mk = like_re.dtype.type
    return mk(s.real), (mk(s.imag) if cplx else None)


def _canonical(M, B, left, lower_m):
    """the leaf brought to ONE form: a lower triangle and right-hand-side columns, solved forwards.  RIGHT is the transposed problem (M^T X^T = B^T); an upper
    triangle is reversed in both indices.  Returns (Mre, Mim, Bre, Bim, undo)."""
    mr, mi = _parts(M)
    br, bi = _parts(B)
    if not left:
        mr, mi, br, bi, lower_m = _t(mr), _t(mi), _t(br), _t(bi), not lower_m
    if not lower_m:
        mr, mi, br, bi = _flip(mr, (0, 1)), _flip(mi, (0, 1)), _flip(br, (0,)), _flip(bi, (0,))
    rev = not lower_m

    def undo(xr, xi):
        if rev:
            xr, xi = _flip(xr, (0,)), _flip(xi, (0,))
        if not left:
            xr, xi = _t(xr), _t(xi)
        return xr, xi
    return mr, mi, br, bi, undo


def leaf_columns(M, B, s, left, lower_m, unit):
    """The leaf solve, column-oriented: once x_j is final, all later rows take their update.  M: the block of op(A) (only its live triangle -- under `unit`
    without the diagonal -- is read), B: the block's rows (left) or columns of B, s: the pending scale or None.  Returns X, an array like B."""
    mr, mi, xr, xi, undo = _canonical(M, B, left, lower_m)
    cplx = mi is not None
    xr, xi = (xr.clone(), None if xi is None else xi.clone()) if is_torch(xr) else (xr.copy(), None if xi is None else xi.copy())
    if s is not None:
        xr, xi = c_mul(_scalar_parts(s, xr, cplx), (xr, xi))
    r = mr.shape[0]
    for j in range(r):
        if not unit:
            qr, qi = c_div((xr[j], None if xi is None else xi[j]), (mr[j, j], None if mi is None else mi[j, j]))
            xr[j] = qr
            if cplx:
                xi[j] = qi
        if j + 1 < r:
            col = (mr[j + 1:, j:j + 1], None if mi is None else mi[j + 1:, j:j + 1])
            pr, pi = c_mul(col, (xr[j:j + 1], None if xi is None else xi[j:j + 1]))
            dr, di = c_sub((xr[j + 1:], None if xi is None else xi[j + 1:]), (pr, pi))
            xr[j + 1:] = dr
            if cplx:
                xi[j + 1:] = di
    xr, xi = undo(xr, xi)
    return _join(xr, xi, B)


def leaf_rows(M, B, s, left, lower_m, unit):
    """The leaf solve as include/gemmul8_c.h writes it: row-oriented scalar loops, each of the four cases in its own index order (numpy only)."""
    M, B = np.asarray(M), np.asarray(B)
    cplx = np.iscomplexobj(B)
    rt = B.real.dtype.type
    r = M.shape[0]
    X = B.copy()

    def el(v):
        return (rt(v.real), rt(v.imag)) if cplx else (rt(v), None)

    def back(p):
        return B.dtype.type(complex(p[0], p[1])) if cplx else p[0]
    sc = None if s is None else (el(np.asarray(s, B.dtype)[()]))
    fwd = left == lower_m
    order = range(r) if fwd else range(r - 1, -1, -1)
    for c in range(B.shape[1] if left else B.shape[0]):
        x = [None] * r
        for i in order:
            b = el(B[i, c] if left else B[c, i])
            acc = c_mul(sc, b) if sc is not None else b
            for j in (range(i) if fwd else range(r - 1, i, -1)):
                mij = el(M[i, j] if left else M[j, i])
                acc = c_sub(acc, c_mul(mij, x[j]) if left else c_mul(x[j], mij))
            x[i] = acc if unit else c_div(acc, el(M[i, i]))
            if left:
                X[i, c] = back(x[i])
            else:
                X[c, i] = back(x[i])
    return X


def op_block(Ablk, trans):
    """the block of M from the stored block of A"""
    if trans == "N":
        return Ablk
    return Ablk.T if trans == "T" else Ablk.conj().T


def solve(A, B, alpha, side, uplo, trans, diag, L, gemm, leaf=leaf_columns):
    """The whole recipe.  A: the stored ka x ka array (only the triangle `uplo` -- under diag "U" without its diagonal -- is read), B: m x n.  alpha: a number,
    or None for no scale at all (every leaf and GEMM then runs unscaled).  gemm(lhs, rhs, opL, opR, beta, C) returns -op(lhs) op(rhs) + beta C for the stored
    operands lhs, rhs.  Returns X; B is not modified."""
    left, lower_m, unit = side == "L", m_is_lower(uplo, trans), diag == "U"
    X = B.clone() if is_torch(B) else B.copy()
    ka = B.shape[0] if left else B.shape[1]
    for st in plan(ka, L, side, lower_m):
        scaled = st[-1] and alpha is not None
        if st[0] == "leaf":
            _, d0, r, _ = st
            blk = slice(d0, d0 + r)
            Mblk = op_block(A[blk, blk], trans)
            if left:
                X[blk, :] = leaf(Mblk, X[blk, :], alpha if scaled else None, left, lower_m, unit)
            else:
                X[:, blk] = leaf(Mblk, X[:, blk], alpha if scaled else None, left, lower_m, unit)
        else:
            _, f0, fn, s0, sn, _ = st
            src, dst = slice(f0, f0 + fn), slice(s0, s0 + sn)
            beta = alpha if scaled else 1
            if left:    # M[dst, src] lies at A[dst, src] (N) or A[src, dst] (T / C)
                Ablk = A[dst, src] if trans == "N" else A[src, dst]
                X[dst, :] = gemm(Ablk, X[src, :], trans, "N", beta, X[dst, :])
            else:       # M[src, dst]
                Ablk = A[src, dst] if trans == "N" else A[dst, src]
                X[:, dst] = gemm(X[:, src], Ablk, "N", trans, beta, X[:, dst])
    return X


# ---- data of the residual condition: off-diagonal entries uniform in +-1/ka, diagonal magnitudes in [1, 2] with random sign (complex: random phase)
def well_conditioned(rng, ka, dt):
    dt = np.dtype(dt)
    A = (rng.random((ka, ka)) * 2 - 1) / ka
    d = (1 + rng.random(ka)) * rng.choice([-1.0, 1.0], ka)
    if dt.kind == "c":
        A = A + 1j * (rng.random((ka, ka)) * 2 - 1) / ka
        d = d * np.exp(2j * np.pi * rng.random(ka))
    A[np.diag_indices(ka)] = d
    return A.astype(dt)


def rhs(rng, shape, dt):
    dt = np.dtype(dt)
    Bm = rng.random(shape) * 2 - 1
    if dt.kind == "c":
        Bm = Bm + 1j * (rng.random(shape) * 2 - 1)
    return Bm.astype(dt)
