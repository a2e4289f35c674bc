"""gemmul8_her2k on the GPU (include/gemmul8_c.h): the stored triangle carries the contract formula applied to W = op(A) op(B)^H as gemmul8_gemm writes it in
the same process -- bit for bit for the eight exact scalar pairs, within 6 u S for the general ones (tests/her2k_util.py) -- and, on a subset, to the
oracle's W computed with the device's shifts, as parity_case does; every byte of the enclosing C buffer outside the triangle keeps its sentinel; NaN
handling, device-resident scalars, A is B, sub-matrix views, HIP-graph replay, U against L.

(a) and (c) run over complex64 / complex128 x trans N / C x both modes x the moduli counts of the type x the shapes below, one test per (type, shape) and
one GEMM per (moduli, trans, mode); both uplo and all eleven scalar pairs at n <= 300, beyond that two pairs per GEMM and one uplo, rotating, so that
every pair and both uplo still occur at every shape; the ldc padding 1 / 7 / 64 rotates through the calls.  T = 64 is the CRT tile (crt_her2k_kernel): the
shapes (n, k) are (1, 1); (37, 65); (T - 1, 8), (T, T), (T + 1, 300): one tile short, exact, and a second tile row and column one entry thick; (256, 256);
(257, 255): a mirror tile pair one row thick behind four full ones; (300, 257); (513, 1024); (1031, 32): five GEMM tile rows, a LAPACK panel width.

(b) costs the CPU oracle about 4 n^2 k N / 1e9 seconds, so it runs once per type and shape, at most 5 s each, the other parameters rotating."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import her2k_util as hu
import oracle_lib as ol

pytestmark = pytest.mark.gpu

T = 64
DTS = [np.complex64, np.complex128]
SHAPES = [(1, 1), (37, 65), (T - 1, 8), (T, T), (T + 1, 300), (256, 256), (257, 255), (300, 257), (513, 1024), (1031, 32)]
PAIRS = hu.EXACT_PAIRS + hu.GENERAL_PAIRS
SENTINEL = 0xA5
LD_EXTRA = (1, 7, 64)


def _moduli(dt):
    return [2, 7, 13] if np.dtype(dt) == np.complex64 else [2, 7, 14, 20]


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape)) + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    return a.astype(dt)


def _pair(rng, n, k, trans, dt):
    """A and B as stored for `trans`; B eight times A's scale"""
    shape = (n, k) if trans == "N" else (k, n)
    return _rand(rng, shape, dt), (8 * _rand(rng, shape, dt)).astype(dt)


def _opb(trans):
    return "C" if trans == "N" else "N"


def _w_dev(dA, dB, trans, N, fast, work=None):
    """W = op(A) op(B)^H from gemmul8_gemm (alpha = 1, beta = 0) as a numpy n x n matrix"""
    W = g.gemm(dA, dB, N, fastmode=fast, opA=trans, opB=_opb(trans), work=work)[0]
    torch.cuda.synchronize()
    return gu.from_dev(W)


def _embedded(dA, dB, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0, scalars_dev=False, work=None, cache=None):
    """gemmul8_her2k on a C embedded with ldc = n + ld_extra in a sentinel-filled buffer whose triangle holds C0's.
    Returns (result as n x n numpy [row, col], bytes after, bytes before), the byte arrays as uint8 [n][ldc][esz]"""
    esz = np.dtype(dt).itemsize
    ldc = n + ld_extra
    key = (id(C0), uplo, ld_extra)
    if cache is not None and key in cache:
        buf = cache[key]
    else:
        buf = np.full((n, ldc, esz), SENTINEL, np.uint8)   # column j at buf[j]
        mk = hu.tri_mask(n, uplo)
        buf[:, :n, :][mk.T] = np.ascontiguousarray(C0.T).view(np.uint8).reshape(n, n, esz)[mk.T]
        if cache is not None:
            cache[key] = buf
    dC = torch.from_numpy(buf).cuda()
    if work is None:
        work = torch.full((g.her2k_work_size(n, k, N),), 0x3C, dtype=torch.uint8, device="cuda")
    al, be = np.array([alpha], dtype=dt), np.array([beta], dtype=hu.real_type(dt))
    if scalars_dev:
        dal, dbe = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
        pa, pb = dal.data_ptr(), dbe.data_ptr()
    else:
        pa, pb = al.ctypes.data, be.ctypes.data
    rc = g.lib().gemmul8_her2k(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.UPLO[uplo], g.OPS[trans], n, k, pa, dA.data_ptr(),
                               dA.stride(0), dB.data_ptr(), dB.stride(0), pb, dC.data_ptr(), ldc, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_her2k")
    torch.cuda.synchronize()
    out = dC.cpu().numpy()
    got = np.ascontiguousarray(out[:, :n, :]).view(dt).reshape(n, n).T
    return got, out, buf


def _check(got, out, buf, W, C0, alpha, beta, uplo, what):
    """(c) the bytes outside the triangle, then the triangle against the model of W"""
    n = W.shape[0]
    mk = hu.tri_mask(n, uplo)
    assert np.array_equal(out[:, n:], buf[:, n:]), "bytes of the ldc padding were written: " + what
    touched = (np.ascontiguousarray(out[:, :n]).view(np.uint64) != np.ascontiguousarray(buf[:, :n]).view(np.uint64)).any(axis=2)
    assert not (touched & ~mk.T).any(), "bytes of the other strict triangle were written: " + what
    R, tol = hu.model(W, alpha, beta, C0)
    bad = hu.mismatches(got, R, tol, mk)
    assert bad == 0, f"{bad} entries of the triangle miss the contract formula ({'bits' if tol is None else 'tolerance'}): " + what
    d = got.imag[np.diag_indices(n)]
    assert not d.any() and not np.signbit(d).any(), "diagonal imaginary parts are not +0.0: " + what


@pytest.mark.parametrize("n,k", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_grid_triangle_is_the_formula_of_the_gemms_w_and_the_rest_is_untouched(dt, n, k):
    """(a) and (c)"""
    rng = np.random.default_rng(n * 131 + k)
    dAB = {t: tuple(gu.to_dev(x) for x in _pair(rng, n, k, t, dt)) for t in "NC"}
    C0 = _rand(rng, (n, n), dt)
    work = torch.empty(g.her2k_work_size(n, k, max(_moduli(dt))), dtype=torch.uint8, device="cuda")
    small = n <= 300
    seen, call, cache = set(), 0, {}
    for gi, (N, trans, fast) in enumerate(itertools.product(_moduli(dt), "NC", (False, True))):
        W = _w_dev(*dAB[trans], trans, N, fast, work)
        pairs = range(len(PAIRS)) if small else [(2 * gi + j) % len(PAIRS) for j in range(2)]
        for pi in pairs:
            alpha, beta = PAIRS[pi]
            for uplo in ("LU" if small else "LU"[(gi + pi) % 2]):
                ld_extra = LD_EXTRA[call % 3]
                call += 1
                seen.add((pi, uplo))
                what = f"N={N} trans={trans} uplo={uplo} fast={fast} alpha={alpha} beta={beta} ldc={n + ld_extra}"
                got, out, buf = _embedded(*dAB[trans], dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0, work=work, cache=cache)
                _check(got, out, buf, W, C0, alpha, beta, uplo, what)
    assert {p for p, _ in seen} == set(range(len(PAIRS))) and {u for _, u in seen} == {"L", "U"}


def _oracle_cases():
    """(b): (type, n, k, trans, mode, scalar pair, moduli, ld_extra, uplo)"""
    out = []
    for si, (n, k) in enumerate(SHAPES):
        for di, dt in enumerate(DTS):
            mods = _moduli(dt)
            j = si * 3 + di * 5
            N = mods[(si + di) % len(mods)]
            while 4 * n * n * k * N / 1e9 > 5 and N > 2:
                N = mods[mods.index(N) - 1]
            out.append((dt, n, k, "NC"[(si + di) % 2], bool((si // 2 + di) % 2), j % len(PAIRS), N, LD_EXTRA[(si + di) % 3], "LU"[((si + di) % 2) ^ (si // 2 % 2)]))
    return out


ORACLE_CASES = _oracle_cases()


def test_the_oracle_subset_covers_every_type_at_every_shape():
    for dt in DTS:
        mine = [c for c in ORACLE_CASES if c[0] is dt]
        assert {(c[1], c[2]) for c in mine} == set(SHAPES)
        assert {c[3] for c in mine} == {"N", "C"} and {c[4] for c in mine} == {False, True} and {c[8] for c in mine} == {"L", "U"}
        assert len({c[6] for c in mine}) >= 3 and {c[7] for c in mine} == set(LD_EXTRA)
        assert any(hu.is_exact_pair(*PAIRS[c[5]]) for c in mine) and any(not hu.is_exact_pair(*PAIRS[c[5]]) for c in mine)
    assert all(4 * c[1] * c[1] * c[2] * c[6] / 1e9 <= 5 for c in ORACLE_CASES)


@pytest.mark.parametrize("dt,n,k,trans,fast,pi,N,ld_extra,uplo", ORACLE_CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1]}x{c[2]}-{c[3]}-{'fast' if c[4] else 'accu'}-s{c[5]}-N{c[6]}-ld{c[7]}-{c[8]}" for c in ORACLE_CASES])
def test_triangle_is_the_formula_of_the_oracles_w(dt, n, k, trans, fast, pi, N, ld_extra, uplo):
    """(b): the oracle's GEMM run with the device's shifts gives W; the device's own W must carry the same bits"""
    rng = np.random.default_rng(n * 131 + k)
    alpha, beta = PAIRS[pi]
    A, B = _pair(rng, n, k, trans, dt)
    C0 = _rand(rng, (n, n), dt)
    Wd, it = gu.hip_gemm(A, B, N, fastmode=fast, opA=trans, opB=_opb(trans), want_intermediates=True)
    Wo = np.asarray(ol.gemm(A, B, N, fastmode=fast, opA=trans, opB=_opb(trans), sftA_in=it["sftA"], sftB_in=it["sftB"]))
    assert gu.bits_equal(Wd, Wo)
    got, out, buf = _embedded(gu.to_dev(A), gu.to_dev(B), dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0)
    _check(got, out, buf, Wo, C0, alpha, beta, uplo, "against the oracle's W")


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_nan_in_c_reaches_only_what_the_contract_says(dt):
    """(c): beta == 0 over a NaN-filled C gives finite results and never reads C; with beta != 0 a NaN in a diagonal imaginary part reaches nothing"""
    rng = np.random.default_rng(5)
    n, k, N = 130, 77, 7
    A, B = _pair(rng, n, k, "N", dt)
    dA, dB = gu.to_dev(A), gu.to_dev(B)
    nan = np.full((n, n), np.nan + 1j * np.nan, dt)
    for uplo, fast, alpha in (("L", False, 0.75 - 0.25j), ("U", True, 1)):
        W = _w_dev(dA, dB, "N", N, fast)
        got, out, buf = _embedded(dA, dB, dt, n, k, uplo, "N", fast, alpha, 0.0, N, 7, nan)
        mk = hu.tri_mask(n, uplo)
        assert np.isfinite(got[mk]).all()
        _check(got, out, buf, W, None, alpha, 0.0, uplo, f"NaN-filled C, beta = 0, uplo {uplo}")
        C0 = _rand(rng, (n, n), dt)
        Cn = C0.copy()
        Cn.imag[np.diag_indices(n)] = np.nan
        got, out, buf = _embedded(dA, dB, dt, n, k, uplo, "N", fast, alpha, 1.0, N, 1, Cn)
        assert np.isfinite(got[mk]).all()
        _check(got, out, buf, W, C0, alpha, 1.0, uplo, f"NaN diagonal imaginary parts, beta = 1, uplo {uplo}")


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("uplo,trans", [("U", "C"), ("L", "N")])
def test_device_resident_scalars(dt, fast, uplo, trans):
    """(d)"""
    rng = np.random.default_rng(6)
    n, k, N = 130, 257, 7
    A, B = _pair(rng, n, k, trans, dt)
    dA, dB = gu.to_dev(A), gu.to_dev(B)
    C0 = _rand(rng, (n, n), dt)
    for alpha, beta in (PAIRS[8], PAIRS[3], PAIRS[10]):
        host = _embedded(dA, dB, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0)[1]
        dev = _embedded(dA, dB, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0, scalars_dev=True)[1]
        assert np.array_equal(host, dev), (alpha, beta)


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("trans", ["N", "C"])
def test_a_is_b(dt, trans):
    """(e): the same pointer for both operands"""
    rng = np.random.default_rng(9)
    n, k, N = 130, 257, 7
    dA = gu.to_dev(_pair(rng, n, k, trans, dt)[0])
    C0 = _rand(rng, (n, n), dt)
    for fast, (alpha, beta) in ((False, PAIRS[4]), (True, PAIRS[9])):
        W = _w_dev(dA, dA, trans, N, fast)
        got, out, buf = _embedded(dA, dA, dt, n, k, "L", trans, fast, alpha, beta, N, 1, C0)
        _check(got, out, buf, W, C0, alpha, beta, "L", f"A is B, trans {trans}")


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("trans", ["N", "C"])
def test_submatrix_views_with_different_leading_dimensions(dt, trans):
    """(f): A and B inside larger buffers, lda = rows + 7 and ldb = rows + 1, each base one element past a 16-byte boundary"""
    rng = np.random.default_rng(10)
    n, k, N = 257, 255, 7
    A, B = _pair(rng, n, k, trans, dt)
    dA, dB = gu.to_dev(A), gu.to_dev(B)
    cols, rows = dA.shape
    views = []
    for X, extra in ((dA, 7), (dB, 1)):
        store = torch.full((cols * (rows + extra) + 1,), 3.0, dtype=X.dtype, device="cuda")
        V = store.as_strided((cols, rows), (rows + extra, 1), 1)
        V.copy_(X)
        assert V.data_ptr() % 16 == X.element_size() % 16 and V.stride(0) == rows + extra
        views.append(V)
    C0 = _rand(rng, (n, n), dt)
    for fast, (alpha, beta) in ((False, PAIRS[7]), (True, PAIRS[8])):
        W = _w_dev(dA, dB, trans, N, fast)
        got, out, buf = _embedded(views[0], views[1], dt, n, k, "U", trans, fast, alpha, beta, N, 64, C0)
        _check(got, out, buf, W, C0, alpha, beta, "U", f"views, trans {trans}")
        Cd = g.her2k(views[0], views[1], N, uplo="U", trans=trans, fastmode=fast, alpha=alpha, beta=0.0)[0]   # the Python wrapper on the same views
        torch.cuda.synchronize()
        R, tol = hu.model(W, alpha, 0.0)
        assert hu.mismatches(gu.from_dev(Cd), R, tol, hu.tri_mask(n, "U")) == 0
        assert not gu.from_dev(Cd)[~hu.tri_mask(n, "U")].any()   # a fresh C_out is zero-filled: the other strict triangle stays so


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "C")])
def test_graph_capture_replays_to_the_same_bits(dt, uplo, trans):
    """(g): timers_ns null, one capture, replayed"""
    rng = np.random.default_rng(7)
    n, k, N = 257, 300, 7
    dA, dB = (gu.to_dev(x) for x in _pair(rng, n, k, trans, dt))
    fast = uplo == "U"
    alpha, beta = PAIRS[8][0], 0.0
    eager, _, work = g.her2k(dA, dB, N, uplo=uplo, trans=trans, fastmode=fast, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.her2k(dA, dB, N, uplo=uplo, trans=trans, fastmode=fast, alpha=alpha, beta=beta, C_out=out, work=work)   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        g.her2k(dA, dB, N, uplo=uplo, trans=trans, fastmode=fast, alpha=alpha, beta=beta, C_out=out, work=work)
    for _ in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert gu.bits_equal(out.cpu().numpy(), eager.cpu().numpy())


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("trans", ["N", "C"])
def test_upper_equals_the_conjugate_transpose_of_lower(dt, trans):
    """(h): beta = 0, numerically equal (==: zero signs aside)"""
    rng = np.random.default_rng(11)
    n, k = 300, 65
    dA, dB = (gu.to_dev(x) for x in _pair(rng, n, k, trans, dt))
    for N, fast, alpha in ((7, False, 0.3 + 1.1j), (_moduli(dt)[-1], True, -1j)):
        L = gu.from_dev(g.her2k(dA, dB, N, uplo="L", trans=trans, fastmode=fast, alpha=alpha)[0])
        U = gu.from_dev(g.her2k(dA, dB, N, uplo="U", trans=trans, fastmode=fast, alpha=alpha)[0])
        torch.cuda.synchronize()
        assert L[hu.tri_mask(n, "L")].any() and not L[~hu.tri_mask(n, "L")].any()
        assert (U == L.conj().T).all(), (N, fast, alpha)
