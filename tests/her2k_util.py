"""A numpy model of the gemmul8_her2k contract (include/gemmul8_c.h).  With W = op(A) op(B)^H as gemmul8_gemm (or the oracle) writes it, W_ij = (x, y),
W_ji = (u, v), the old C_ij = (cx, cy) and alpha = (ar, ai), in the element type with one rounding each:

    p = x + u,  q = y - v,  r = y + v,  t = x - u
    Re = fma(beta, cx, fma(-ai, r, ar * p))
    Im = fma(beta, cy, fma( ai, t, ar * q))        (diagonal: cy counts as 0, Im = +0.0; beta == 0: cx = cy = 0, C unread)

numpy has no fused multiply-add, but a fused operation whose product is exact equals the product followed by the addition, signed zeros included.  With
alpha in {1, -1, i, -i} and beta in {0, 1} every product above is exact, so for these EXACT pairs the model gives the bits.  Elsewhere it is an exact
reference (longdouble where its epsilon is <= 2^-63, else fractions.Fraction) with the tolerance 6 u S,
    S = |ar| (|x| + |u|) + |ai| (|y| + |v|) + |beta| |cx|      (imaginary part: |ar| (|y| + |v|) + |ai| (|x| + |u|) + |beta| |cy|),
u = 2^-24 / 2^-53: the formula rounds at most five times on the way to a component (p or q, r or t, the product, two fused operations), each by at most
u times a partial sum that S bounds, and one more unit is the reference's own."""
import fractions

import numpy as np

EXACT_ALPHAS = (1, -1, 1j, -1j)
EXACT_BETAS = (0, 1)
EXACT_PAIRS = [(a, b) for a in EXACT_ALPHAS for b in EXACT_BETAS]
GENERAL_PAIRS = [(0.75 - 0.25j, -0.5), (0.3 + 1.1j, 1.5), (0, 2)]
LONGDOUBLE_OK = float(np.finfo(np.longdouble).eps) <= 2.0 ** -63


def is_exact_pair(alpha, beta):
    return complex(alpha) in [complex(a) for a in EXACT_ALPHAS] and float(beta) in (0.0, 1.0)


def real_type(dt):
    return np.float32 if np.dtype(dt) == np.complex64 else np.float64


def tri_mask(n, uplo):
    i, j = np.indices((n, n))
    return i >= j if uplo == "L" else i <= j


def _exact_sum(terms):
    """sum of products [(a, X), ...] of a scalar and an array, exactly (Fraction) or to 2^-64 (longdouble)"""
    if LONGDOUBLE_OK:
        out = np.zeros(terms[0][1].shape, np.longdouble)
        for a, X in terms:
            out = out + np.longdouble(a) * X.astype(np.longdouble)
        return out
    out = np.zeros(terms[0][1].shape, object)
    for a, X in terms:
        out = out + fractions.Fraction(float(a)) * np.vectorize(fractions.Fraction, otypes=[object])(X.astype(np.float64))
    return out


def _round_to(E, rt):
    if LONGDOUBLE_OK:
        return E.astype(rt)
    return np.array([[float(e) for e in row] for row in E], np.float64).astype(rt)   # (two roundings for float32: within the reference's unit)


def model(W, alpha, beta, C0=None):
    """The n x n matrix of the contract formula from W (every entry, as if stored; the caller masks the triangle) in W's dtype.
    Returns (R, None) for an exact scalar pair -- R carries the bits -- and (R, (tol_re, tol_im)) otherwise."""
    dt = W.dtype
    rt = real_type(dt)
    n = W.shape[0]
    ar, ai, be = rt(complex(alpha).real), rt(complex(alpha).imag), rt(beta)
    x, y, u, v = W.real, W.imag, W.T.real, W.T.imag
    if be == 0 or C0 is None:
        cx, cy = np.zeros((n, n), rt), np.zeros((n, n), rt)
    else:
        cx, cy = C0.real.astype(rt), C0.imag.astype(rt).copy()
        cy[np.diag_indices(n)] = 0
    R = np.empty((n, n), dt)
    with np.errstate(invalid="ignore"):
        p, q, r, t = x + u, y - v, y + v, x - u   # (bitwise symmetric / antisymmetric in (i, j): so is everything below)
        if is_exact_pair(alpha, beta):
            R.real = be * cx + ((-ai) * r + ar * p)
            R.imag = be * cy + (ai * t + ar * q)
            R.imag[np.diag_indices(n)] = 0.0
            return R, None
        re = _exact_sum([(ar, p), (-ai, r), (be, cx)])   # the formula's first step as it stands, the rest without rounding
        im = _exact_sum([(ar, q), (ai, t), (be, cy)])
        R.real, R.imag = _round_to(re, rt), _round_to(im, rt)
        R.imag[np.diag_indices(n)] = 0.0
    unit = 2.0 ** -24 if rt is np.float32 else 2.0 ** -53
    a64 = lambda z: np.abs(z.astype(np.float64))
    s_re = abs(float(ar)) * (a64(x) + a64(u)) + abs(float(ai)) * (a64(y) + a64(v)) + abs(float(be)) * a64(cx)
    s_im = abs(float(ar)) * (a64(y) + a64(v)) + abs(float(ai)) * (a64(x) + a64(u)) + abs(float(be)) * a64(cy)
    return R, (6 * unit * s_re, 6 * unit * s_im)


def mismatches(got, R, tol, mask):
    """number of entries of `mask` at which got (n x n, rows x cols) misses the model: bits for tol None, else |difference| <= tol per component"""
    if tol is None:
        it = np.uint32 if real_type(got.dtype) is np.float32 else np.uint64
        bad = (np.ascontiguousarray(got.real).view(it) != np.ascontiguousarray(R.real).view(it)) | \
              (np.ascontiguousarray(got.imag).view(it) != np.ascontiguousarray(R.imag).view(it))
    else:
        with np.errstate(invalid="ignore"):
            dre = np.abs(got.real.astype(np.float64) - R.real.astype(np.float64))
            dim = np.abs(got.imag.astype(np.float64) - R.imag.astype(np.float64))
            bad = ~(dre <= tol[0]) | ~(dim <= tol[1])
    return int((bad & mask).sum())
