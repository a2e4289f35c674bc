"""gemmul8_syr2k on the GPU: the stored triangle carries the bits of the equivalent GEMM -- gemmul8_gemm on P = [A, Z, B, Z] and Q = [B, Z, A, Z]
materialised with the zero block (tests/test_syr2k_premise.py), run in the same process and, through the oracle with the device's shifts, as parity_case
does --, every byte of the enclosing C buffer outside the triangle keeps its sentinel; device-resident scalars, A is B, sub-matrix views, HIP-graph replay.

(a) and (c) run over the WHOLE grid: 4 types x 2 trans x 2 uplo x 2 modes x 4 scalar pairs x the moduli counts of the type x 8 shapes, one test per
(type, shape), buffers and comparisons on the device; the ldc padding 1 / 7 / 64 rotates through the calls of a test.  The shapes (n, k) are the smallest
at which each mechanism can fail: (1, 1); (37, 65); (256, 256): no zero block; (257, 255) and (300, 257): the pad edge on either side, a second tile-row of
one row; (513, 1024): the seam on a 1024-chunk boundary of the quantise kernels; (700, 1100): kh = 1280, the seam inside a 1024 chunk of the
concatenation; (1031, 300): 5 tile-rows, the triangular walk's group of 4 cut.

(b) costs the CPU oracle about n^2 2kh N (x 4 for complex) / 1e9 seconds per GEMM, so it runs on a subset: every type at every shape, both modes at the six
cheap shapes and one at the two largest (2 moduli there), both triangles compared with the one oracle GEMM of a case, the other parameters rotating."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol
from test_syr2k_premise import concat

pytestmark = pytest.mark.gpu

DTS = [np.float32, np.float64, np.complex64, np.complex128]
SHAPES = [(1, 1), (37, 65), (256, 256), (257, 255), (300, 257), (513, 1024), (700, 1100), (1031, 300)]
LARGE = [(700, 1100), (1031, 300)]
SCALARS = [(1, 0), (-1, 1), (0.75, -0.5), (0, 2)]
CSCALARS = [(1, 0), (-1, 1), (0.75 - 0.25j, -0.5 + 1.5j), (0, 2 - 1j)]
SENTINEL = 0xA5
LD_EXTRA = (1, 7, 64)


def _cplx(dt):
    return np.dtype(dt).kind == "c"


def _moduli(dt):
    return [2, 7, 13] if np.dtype(dt).itemsize // (2 if _cplx(dt) else 1) == 4 else [2, 7, 14, 20]


def _kh(k):
    return (k + 255) // 256 * 256


def _oracle_seconds(dt, n, k, N):
    return n * n * 2 * _kh(k) * N * (4 if _cplx(dt) else 1) / 1e9


def _oracle_cases():
    """(b): (type, n, k, trans, mode, scalar pair, moduli, ld_extra); both uplo are compared with the one oracle GEMM of a case"""
    out = []
    for si, (n, k) in enumerate(SHAPES):
        large = (n, k) in LARGE
        for di, dt in enumerate(DTS):
            mods = _moduli(dt)
            for r in range(1 if large else 2):
                j = si * 5 + di * 3 + r
                fast = bool((si + di) % 2) if large else bool(r)
                N = 2 if large else mods[(j + di) % len(mods)]
                while _oracle_seconds(dt, n, k, N) > 5 and N > 2:   # the next smaller count of the type
                    N = mods[mods.index(N) - 1]
                out.append((dt, n, k, "NT"[(j // 2 + di) % 2], fast, (j + si) % 4, N, LD_EXTRA[j % 3]))
    return out


ORACLE_CASES = _oracle_cases()


def test_the_oracle_subset_covers_every_type_at_every_shape_in_both_modes_and_trans():
    for dt in DTS:
        mine = [c for c in ORACLE_CASES if c[0] is dt]
        assert {(c[1], c[2]) for c in mine} == set(SHAPES)
        assert {c[3] for c in mine} == {"N", "T"} and {c[4] for c in mine} == {False, True}
        assert {c[5] for c in mine} == {0, 1, 2, 3} and {c[7] for c in mine} == set(LD_EXTRA)
        assert len({c[6] for c in mine}) >= 3 and {c[6] for c in mine} <= set(_moduli(dt))
        for n, k in SHAPES:
            if (n, k) not in LARGE:
                assert {c[4] for c in mine if (c[1], c[2]) == (n, k)} == {False, True}
    large = [c for c in ORACLE_CASES if (c[1], c[2]) in LARGE]
    assert {(c[0], c[1]) for c in large} == set(itertools.product(DTS, (700, 1031))) and {c[6] for c in large} == {2}
    assert {c[3] for c in large} == {"N", "T"} and {c[4] for c in large} == {False, True}
    for c in ORACLE_CASES:   # about 5 s per oracle GEMM; the complex types at the two largest shapes cost 9 to 10 s with the smallest count there is
        assert _oracle_seconds(c[0], c[1], c[2], c[6]) <= (5 if (c[1], c[2]) not in LARGE or not _cplx(c[0]) else 10.5), c


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    if _cplx(dt):
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    return a.astype(dt)


def _pair(rng, n, k, trans, dt):
    """A and B as stored for `trans`; B eight times A's scale"""
    shape = (n, k) if trans == "N" else (k, n)
    return _rand(rng, shape, dt), (8 * _rand(rng, shape, dt)).astype(dt)


def _tri_mask(n, uplo):
    i, j = np.indices((n, n))
    return i >= j if uplo == "L" else i <= j


def _concat_dev(dA, dB, trans):
    """P and Q of test_syr2k_premise.concat, built on the device from column-major tensors (cols, rows)"""
    k = dA.shape[0] if trans == "N" else dA.shape[1]
    kh = _kh(k)
    if trans == "N":
        P, Q = (torch.zeros((2 * kh, dA.shape[1]), dtype=dA.dtype, device="cuda") for _ in range(2))
        P[:k], P[kh:kh + k], Q[:k], Q[kh:kh + k] = dA, dB, dB, dA
    else:
        P, Q = (torch.zeros((dA.shape[0], 2 * kh), dtype=dA.dtype, device="cuda") for _ in range(2))
        P[:, :k], P[:, kh:kh + k], Q[:, :k], Q[:, kh:kh + k] = dA, dB, dB, dA
    return P, Q


def _gemm_dev(dA, dB, trans, N, fast, alpha=1.0, beta=0.0, C_out=None, work=None):
    P, Q = _concat_dev(dA, dB, trans)
    return g.gemm(P, Q, N, fastmode=fast, opA=trans, opB="T" if trans == "N" else "N", alpha=alpha, beta=beta, C_out=C_out, work=work)[0]


def _syr2k_embedded(A, B, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0, alpha_beta_dev=False):
    """gemmul8_syr2k on a C embedded with ldc = n + ld_extra in a sentinel-filled buffer whose triangle holds C0's; returns (result, buffer before) as uint8 [n][ldc][esz]"""
    esz = np.dtype(dt).itemsize
    ldc = n + ld_extra
    buf = np.full((n, ldc, esz), SENTINEL, np.uint8)   # column j at buf[j]
    mk = _tri_mask(n, uplo)
    win = buf[:, :n, :]
    win[mk.T] = np.ascontiguousarray(C0.T).view(np.uint8).reshape(n, n, esz)[mk.T]
    dC = torch.from_numpy(buf.copy()).cuda()
    dA, dB = gu.to_dev(A), gu.to_dev(B)
    work = torch.full((g.syr2k_work_size(_cplx(dt), n, k, N),), 0x3C, dtype=torch.uint8, device="cuda")
    al, be = np.array([alpha], dtype=dt), np.array([beta], dtype=dt)
    if alpha_beta_dev:
        dal, dbe = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
        pa, pb = dal.data_ptr(), dbe.data_ptr()
    else:
        pa, pb = al.ctypes.data, be.ctypes.data
    rc = g.lib().gemmul8_syr2k(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.UPLO[uplo], g.OPS[trans], n, k, pa, dA.data_ptr(),
                               dA.shape[1], dB.data_ptr(), dB.shape[1], pb, dC.data_ptr(), ldc, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_syr2k")
    torch.cuda.synchronize()
    return dC.cpu().numpy(), buf


def _words(x):
    """a (cols, ld) tensor of any of the four types as its int32 words, (cols, ld * words per element)"""
    if x.is_complex():
        x = torch.view_as_real(x).reshape(x.shape[0], -1)
    return x.view(torch.int32)


@pytest.mark.parametrize("n,k", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_whole_grid_triangle_is_the_gemms_and_the_rest_is_untouched(dt, n, k):
    """(a) and (c) for every trans x uplo x mode x scalar pair x moduli count of this type and shape: 32 x 3 or 4 SYR2K calls against 16 x 3 or 4 GEMMs"""
    rng = np.random.default_rng(n * 131 + k)
    cplx = _cplx(dt)
    w = np.dtype(dt).itemsize // 4
    dAB = {t: tuple(gu.to_dev(x) for x in _pair(rng, n, k, t, dt)) for t in "NT"}
    PQ = {t: _concat_dev(*dAB[t], t) for t in "NT"}
    C0 = gu.to_dev(_rand(rng, (n, n), dt))
    C0w = _words(C0)
    tri = {"L": torch.ones((n, n), dtype=torch.bool, device="cuda").triu(), "U": torch.ones((n, n), dtype=torch.bool, device="cuda").tril()}  # [col][row]
    triw = {u: m.repeat_interleave(w, dim=1) for u, m in tri.items()}
    work = torch.empty(g.syr2k_work_size(cplx, n, k, max(_moduli(dt))), dtype=torch.uint8, device="cuda")
    call = 0
    for N, trans, fast, sc in itertools.product(_moduli(dt), "NT", (False, True), range(4)):
        alpha, beta = (CSCALARS if cplx else SCALARS)[sc]
        Cg, _, _ = g.gemm(*PQ[trans], N, fastmode=fast, opA=trans, opB="T" if trans == "N" else "N", alpha=alpha, beta=beta, C_out=C0.clone(), work=work)
        Cgw = _words(Cg)
        for uplo in "LU":
            ldc = n + LD_EXTRA[call % 3]
            call += 1
            before = torch.full((n, ldc * w), int(np.array([SENTINEL] * 4, np.uint8).view(np.int32)[0]), dtype=torch.int32, device="cuda")
            before[:, :n * w] = torch.where(triw[uplo], C0w, before[:, :n * w])
            buf = before.clone()
            Cd = buf.view(torch.float32 if w == 1 else torch.float64) if not cplx else torch.view_as_complex(buf.view(torch.float32 if w == 2 else torch.float64).reshape(n, ldc, 2))
            assert Cd.shape == (n, ldc) and Cd.data_ptr() == buf.data_ptr()
            g.syr2k(*dAB[trans], N, uplo=uplo, trans=trans, fastmode=fast, alpha=alpha, beta=beta, C_out=Cd, work=work)
            torch.cuda.synchronize()
            what = f"N={N} trans={trans} uplo={uplo} fast={fast} scalars={sc} ldc={ldc}"
            diff = buf != before
            inside = torch.zeros((n, ldc * w), dtype=torch.bool, device="cuda")
            inside[:, :n * w] = triw[uplo]
            assert not bool((diff & ~inside).any()), "bytes outside the stored triangle were written: " + what                       # (c)
            bad = (buf[:, :n * w] != Cgw) & triw[uplo]
            assert not bool(bad.any()), f"{int(bad.sum())} words of the triangle differ from gemmul8_gemm(P, Q): " + what            # (a)


@pytest.mark.parametrize("dt,n,k,trans,fast,sc,N,ld_extra", ORACLE_CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1]}x{c[2]}-{c[3]}-{'fast' if c[4] else 'accu'}-s{c[5]}-N{c[6]}-ld{c[7]}" for c in ORACLE_CASES])
def test_triangle_bits_equal_the_oracles_gemm(dt, n, k, trans, fast, sc, N, ld_extra):
    """(b), with (a) and (c) on the host side: both triangles against ONE oracle GEMM run with the device's shifts"""
    rng = np.random.default_rng(n * 131 + k)
    alpha, beta = (CSCALARS if _cplx(dt) else SCALARS)[sc]
    A, B = _pair(rng, n, k, trans, dt)
    P, Q, _ = concat(A, B, trans)
    C0 = _rand(rng, (n, n), dt)
    esz = np.dtype(dt).itemsize
    opB = "T" if trans == "N" else "N"
    Cg, it = gu.hip_gemm(P, Q, N, fastmode=fast, opA=trans, opB=opB, alpha=alpha, beta=beta, C0=C0, want_intermediates=True)
    Co = ol.gemm(P, Q, N, fastmode=fast, opA=trans, opB=opB, alpha=alpha, beta=beta, C0=C0, sftA_in=it["sftA"], sftB_in=it["sftB"])
    ref = np.ascontiguousarray(Cg.T).view(np.uint8).reshape(n, n, esz)
    refo = np.ascontiguousarray(np.asarray(Co).T).view(np.uint8).reshape(n, n, esz)
    for uplo in "LU":
        out, buf = _syr2k_embedded(A, B, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0)
        mk = _tri_mask(n, uplo)
        keep = np.ones(out.shape[:2], bool)
        keep[:, :n] = ~mk.T
        assert np.array_equal(out[keep], buf[keep]), "bytes outside the stored triangle were written"
        got = out[:, :n, :]
        bad = (got != ref).any(axis=2) & mk.T
        assert not bad.any(), f"uplo {uplo}: {bad.sum()} entries of the triangle differ from gemmul8_gemm(P, Q); first at (col, row) {np.argwhere(bad)[:3].tolist()}"
        bad = (got != refo).any(axis=2) & mk.T
        assert not bad.any(), f"uplo {uplo}: {bad.sum()} entries of the triangle differ from the oracle's GEMM"


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_beta_zero_over_a_nan_triangle_gives_finite_results(dt):
    """beta == 0 (host scalars, general form: alpha = 0.75): a C full of NaN gives the finite result and the other triangle keeps its NaN"""
    rng = np.random.default_rng(5)
    n, k, N = 300, 77, 7
    A, B = _pair(rng, n, k, "N", dt)
    nan = np.full((n, n), np.nan, dt)
    for uplo, fast in (("L", False), ("U", True)):
        mk = _tri_mask(n, uplo)
        Cd, _, _ = g.syr2k(gu.to_dev(A), gu.to_dev(B), N, uplo=uplo, fastmode=fast, alpha=0.75, beta=0.0, C_out=gu.to_dev(nan.copy()))
        torch.cuda.synchronize()
        C = gu.from_dev(Cd)
        assert np.isfinite(C[mk]).all() and np.isnan(C[~mk]).all()


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("uplo,trans", [("U", "T"), ("L", "N")])
def test_device_resident_scalars(dt, fast, uplo, trans):
    rng = np.random.default_rng(6)
    n, k, N = 300, 257, 7
    alpha, beta = (CSCALARS if _cplx(dt) else SCALARS)[2]
    A, B = _pair(rng, n, k, trans, dt)
    C0 = _rand(rng, (n, n), dt)
    host, _ = _syr2k_embedded(A, B, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0)
    dev, _ = _syr2k_embedded(A, B, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0, alpha_beta_dev=True)
    assert np.array_equal(host, dev)


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("trans", ["N", "T"])
def test_a_is_b(dt, trans):
    """the same pointer for both operands: 2 A A^T as the GEMM on [A, Z, A, Z] gives it"""
    rng = np.random.default_rng(9)
    n, k, N = 300, 257, 7
    dA = gu.to_dev(_pair(rng, n, k, trans, dt)[0])
    low = torch.ones((n, n), dtype=torch.bool, device="cuda").triu()   # [col][row]: the lower triangle
    for fast in (False, True):
        Cd, _, _ = g.syr2k(dA, dA, N, uplo="L", trans=trans, fastmode=fast)
        Cg = _gemm_dev(dA, dA, trans, N, fast)
        torch.cuda.synchronize()
        assert gu.bits_equal(torch.where(low, Cd, torch.zeros_like(Cd)).cpu().numpy(), torch.where(low, Cg, torch.zeros_like(Cg)).cpu().numpy())
        assert not bool((Cd[~low] != 0).any())   # a fresh C_out is zero-filled: the other strict triangle stays so


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("trans", ["N", "T"])
def test_submatrix_views_with_different_leading_dimensions(dt, trans):
    """A and B inside larger buffers, lda = rows + 7 and ldb = rows + 1, each base one element past a 16-byte boundary"""
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
    up = torch.ones((n, n), dtype=torch.bool, device="cuda").tril()   # [col][row]: the upper triangle
    for fast in (False, True):
        Cd, _, _ = g.syr2k(views[0], views[1], N, uplo="U", trans=trans, fastmode=fast)
        Cg = _gemm_dev(dA, dB, trans, N, fast)
        torch.cuda.synchronize()
        assert gu.bits_equal(torch.where(up, Cd, torch.zeros_like(Cd)).cpu().numpy(), torch.where(up, Cg, torch.zeros_like(Cg)).cpu().numpy())


@pytest.mark.parametrize("dt", [np.float64, np.complex64], ids=["float64", "complex64"])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "T")])
def test_graph_capture_replays_to_the_same_bits(dt, uplo, trans):
    rng = np.random.default_rng(7)
    n, k, N = 513, 300, 7
    dA, dB = (gu.to_dev(x) for x in _pair(rng, n, k, trans, dt))
    for fast in (False, True):
        eager, _, work = g.syr2k(dA, dB, N, uplo=uplo, trans=trans, fastmode=fast)
        torch.cuda.synchronize()
        out = torch.zeros_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.syr2k(dA, dB, N, uplo=uplo, trans=trans, fastmode=fast, C_out=out, work=work)   # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        out.zero_()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            g.syr2k(dA, dB, N, uplo=uplo, trans=trans, fastmode=fast, C_out=out, work=work)
        for _ in range(2):
            out.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert gu.bits_equal(out.cpu().numpy(), eager.cpu().numpy())
