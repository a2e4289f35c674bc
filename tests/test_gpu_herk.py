"""gemmul8_herk on the GPU (include/gemmul8_c.h).  Off the diagonal the stored triangle carries the bits of the equivalent GEMM of A with its own
conjugate transpose, run in the same process with the real scalars widened to (alpha, 0), (beta, 0); a diagonal entry carries that GEMM's real
part and all-zero bits as its imaginary part, whatever the incoming imaginary part was (NaN in half the calls, a finite non-zero value in the
rest); every byte of the enclosing C buffer outside the triangle keeps its sentinel; with beta == 0 the triangle comes in full of NaN.

This is the first caller of the triangular tile walk whose left and right panels differ, and Im C is not antisymmetric, so a tile that took its
panels the wrong way round would conjugate its entries: the off-diagonal imaginary bits of both uplo against the ONE GEMM catch it, at one tile
(256), two tile-rows (257), a cut group of four (1031 = five tile-rows) and paired long and short groups (2304 = nine).

The whole grid runs per (type, shape) with buffers and comparisons on the device; the ldc padding 1 / 7 / 64 rotates through the calls.  The CPU
oracle costs about 4 n^2 k N / 1e9 seconds per complex GEMM, so oracle parity runs on a stated subset (ORACLE_CASES: every type x trans x mode at
the six shapes up to 1031 x 257, at moduli counts that keep one oracle GEMM under about 10 s); (2304, 512) is tied to the GEMM's bits by the
grid test, and tests/test_gpu_parity.py holds gemmul8_gemm against the oracle."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol

pytestmark = pytest.mark.gpu

DTS = [np.complex64, np.complex128]
SHAPES = [(1, 1), (37, 65), (256, 300), (257, 1024), (700, 129), (1031, 257), (2304, 512)]
SCALARS = [(1, 0), (-1, 1), (0.75, -0.5), (0, 2)]   # real (alpha, beta)
SENTINEL = 0xA5
LD_EXTRA = (1, 7, 64)


def _moduli(dt):
    return [2, 7, 13] if dt is np.complex64 else [2, 7, 14, 20]


def _oracle_cases():
    """(type, n, k, trans, mode, scalar pair, moduli, ld_extra); both uplo are compared with the one oracle GEMM of a case"""
    out = []
    j = 0
    for n, k in SHAPES[:6]:
        for dt, trans, fast in itertools.product(DTS, "NC", (False, True)):
            mods = [N for N in _moduli(dt) if 4 * n * n * k * N / 1e9 < 10.0]
            out.append((dt, n, k, trans, fast, j % 4, mods[j % len(mods)], LD_EXTRA[j % 3]))
            j += 1
    return out


ORACLE_CASES = _oracle_cases()


def test_the_oracle_subset_holds_every_type_trans_mode_and_uplo():
    for n, k in SHAPES[:6]:
        mine = [c for c in ORACLE_CASES if (c[1], c[2]) == (n, k)]
        assert {(c[0], c[3], c[4]) for c in mine} == set(itertools.product(DTS, "NC", (False, True)))
    assert {c[5] for c in ORACLE_CASES} == {0, 1, 2, 3} and {c[7] for c in ORACLE_CASES} == set(LD_EXTRA)
    for dt in DTS:
        assert {c[6] for c in ORACLE_CASES if c[0] is dt} == set(_moduli(dt))
    # (both uplo: test_triangle_bits_equal_the_oracles_gemm loops over "LU" inside every case)


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    return a.astype(dt)


def _rand_c(rng, n, dt):
    """a valid HERK input: the diagonal is real"""
    c = _rand(rng, (n, n), dt)
    c[np.arange(n), np.arange(n)] = c[np.arange(n), np.arange(n)].real
    return c


def _tri_mask(n, uplo):
    i, j = np.indices((n, n))
    return i >= j if uplo == "L" else i <= j


def _words(x):
    """a complex (cols, ld) tensor as its int32 words, (cols, ld * words per element)"""
    return torch.view_as_real(x).reshape(x.shape[0], -1).view(torch.int32)


def _as_complex(buf, n, ldc, w):
    return torch.view_as_complex(buf.view(torch.float32 if w == 2 else torch.float64).reshape(n, ldc, 2))


def _diag_imag(Cin, value):
    """Cin (device, complex, [col][row]) with the imaginary parts of its diagonal replaced"""
    out = Cin.clone()
    idx = torch.arange(out.shape[0], device=out.device)
    torch.view_as_real(out)[idx, idx, 1] = value
    return out


@pytest.mark.parametrize("n,k", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_whole_grid_against_the_equivalent_gemm(dt, n, k):
    """every trans x uplo x mode x scalar pair x moduli count of this type and shape: 32 x 3 or 4 HERK calls against 16 x 3 or 4 GEMMs"""
    rng = np.random.default_rng(n * 131 + k)
    w = np.dtype(dt).itemsize // 4          # int32 words per element; the first half is Re
    dAs = {"N": gu.to_dev(_rand(rng, (n, k), dt)), "C": gu.to_dev(_rand(rng, (k, n), dt))}
    C0 = gu.to_dev(_rand_c(rng, n, dt))
    ones = torch.ones((n, n), dtype=torch.bool, device="cuda")
    tri = {"L": ones.triu(), "U": ones.tril()}   # [col][row]
    triw = {u: m.repeat_interleave(w, dim=1) for u, m in tri.items()}
    imsel = torch.tensor(([False] * (w // 2) + [True] * (w // 2)) * n, device="cuda")[None, :].expand(n, -1)
    diag_im = torch.eye(n, dtype=torch.bool, device="cuda").repeat_interleave(w, dim=1) & imsel
    work = torch.empty(g.work_size(True, g.INT8, n, n, k, max(_moduli(dt)))[0], dtype=torch.uint8, device="cuda")
    sent = int(np.array([SENTINEL] * 4, np.uint8).view(np.int32)[0])
    call = 0
    for N, trans, fast, sc in itertools.product(_moduli(dt), "NC", (False, True), range(4)):
        alpha, beta = SCALARS[sc]
        Cg, _, _ = g.gemm(dAs[trans], dAs[trans], N, fastmode=fast, opA=trans, opB="C" if trans == "N" else "N", alpha=complex(alpha, 0), beta=complex(beta, 0),
                          C_out=C0.clone(), work=work)
        Cgw = _words(Cg)
        for uplo in "LU":
            ldc = n + LD_EXTRA[call % 3]
            nan_diag = call % 2 == 0 if uplo == "L" else (call // 2) % 2 == 0   # half the calls of either uplo
            call += 1
            Cin = torch.full_like(C0, complex(float("nan"), float("nan"))) if beta == 0 else _diag_imag(C0, float("nan") if nan_diag else 3.25)
            before = torch.full((n, ldc * w), sent, dtype=torch.int32, device="cuda")
            before[:, :n * w] = torch.where(triw[uplo], _words(Cin), before[:, :n * w])
            buf = before.clone()
            Cd = _as_complex(buf, n, ldc, w)
            assert Cd.shape == (n, ldc) and Cd.data_ptr() == buf.data_ptr()
            g.herk(dAs[trans], N, uplo=uplo, trans=trans, fastmode=fast, alpha=alpha, beta=beta, C_out=Cd, work=work)
            torch.cuda.synchronize()
            what = f"N={N} trans={trans} uplo={uplo} fast={fast} scalars={sc} ldc={ldc} nan_diag={nan_diag}"
            inside = torch.zeros((n, ldc * w), dtype=torch.bool, device="cuda")
            inside[:, :n * w] = triw[uplo]
            assert not bool(((buf != before) & ~inside).any()), "bytes outside the stored triangle were written: " + what
            got = buf[:, :n * w]
            bad = (got != Cgw) & triw[uplo] & ~diag_im
            assert not bool(bad.any()), f"{int(bad.sum())} words of the triangle (off the diagonal, and the diagonal's real parts) differ from gemmul8_gemm(A, A^H): " + what
            assert not bool(got[diag_im].any()), "a diagonal imaginary part is not +0.0: " + what


def _herk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0, scalars_dev=False):
    """gemmul8_herk on a C embedded with ldc = n + ld_extra in a sentinel-filled buffer whose triangle holds C0's; returns (result, buffer before) as uint8 [n][ldc][esz]"""
    esz = np.dtype(dt).itemsize
    ldc = n + ld_extra
    buf = np.full((n, ldc, esz), SENTINEL, np.uint8)   # column j at buf[j]
    mk = _tri_mask(n, uplo)
    buf[:, :n, :][mk.T] = np.ascontiguousarray(C0.T).view(np.uint8).reshape(n, n, esz)[mk.T]
    dC = torch.from_numpy(buf.copy()).cuda()
    dA = gu.to_dev(A)
    work = torch.full((g.work_size(True, g.INT8, n, n, k, N)[0],), 0x3C, dtype=torch.uint8, device="cuda")
    rdt = np.float32 if dt is np.complex64 else np.float64
    al, be = np.array([alpha], dtype=rdt), np.array([beta], dtype=rdt)
    if scalars_dev:
        dal, dbe = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
        pa, pb = dal.data_ptr(), dbe.data_ptr()
    else:
        pa, pb = al.ctypes.data, be.ctypes.data
    rc = g.lib().gemmul8_herk(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.UPLO[uplo], g.OPS[trans], n, k, pa, dA.data_ptr(),
                              dA.shape[1], pb, dC.data_ptr(), ldc, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_herk")
    torch.cuda.synchronize()
    return dC.cpu().numpy(), buf


@pytest.mark.parametrize("dt,n,k,trans,fast,sc,N,ld_extra", ORACLE_CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1]}x{c[2]}-{c[3]}-{'fast' if c[4] else 'accu'}-s{c[5]}-N{c[6]}-ld{c[7]}" for c in ORACLE_CASES])
def test_triangle_bits_equal_the_oracles_gemm(dt, n, k, trans, fast, sc, N, ld_extra):
    """both triangles against ONE oracle GEMM run with the device's shifts; the diagonal's incoming imaginary parts are NaN"""
    rng = np.random.default_rng(n * 131 + k)
    alpha, beta = SCALARS[sc]
    A = _rand(rng, (n, k) if trans == "N" else (k, n), dt)
    C0 = _rand_c(rng, n, dt)
    esz = np.dtype(dt).itemsize
    opB = "C" if trans == "N" else "N"
    _, it = gu.hip_gemm(A, A, N, fastmode=fast, opA=trans, opB=opB, alpha=alpha, beta=beta, C0=C0, want_intermediates=True)
    Co = np.asarray(ol.gemm(A, A, N, fastmode=fast, opA=trans, opB=opB, alpha=alpha, beta=beta, C0=C0, sftA_in=it["sftA"], sftB_in=it["sftB"]))
    assert not np.diagonal(Co).imag.any()
    refo = np.ascontiguousarray(Co.T).view(np.uint8).reshape(n, n, esz)
    Cin = C0.copy()
    Cin.imag[np.arange(n), np.arange(n)] = np.nan
    for uplo in "LU":
        out, buf = _herk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, Cin)
        mk = _tri_mask(n, uplo)
        keep = np.ones(out.shape[:2], bool)
        keep[:, :n] = ~mk.T
        assert np.array_equal(out[keep], buf[keep]), "bytes outside the stored triangle were written"
        got = out[:, :n, :]
        d = np.arange(n)
        assert not got[d, d, esz // 2:].any(), f"uplo {uplo}: a diagonal imaginary part is not +0.0"
        bad = (got != refo).any(axis=2) & mk.T
        assert not bad.any(), f"uplo {uplo}: {bad.sum()} entries of the triangle differ from the oracle's GEMM; first at (col, row) {np.argwhere(bad)[:3].tolist()}"


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("uplo,trans", [("U", "C"), ("L", "N")])
def test_device_resident_real_scalars(dt, fast, uplo, trans):
    rng = np.random.default_rng(6)
    n, k, N = 700, 129, 7
    alpha, beta = SCALARS[2]
    A = _rand(rng, (k, n) if trans == "C" else (n, k), dt)
    C0 = _rand_c(rng, n, dt)
    C0.imag[np.arange(n), np.arange(n)] = np.nan
    host, _ = _herk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0)
    dev, _ = _herk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0, scalars_dev=True)
    assert np.array_equal(host, dev)


@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "C")])
def test_graph_capture_replays_to_the_same_bits(dt, uplo, trans):
    rng = np.random.default_rng(7)
    n, k, N = 1031, 257, 7
    dA = gu.to_dev(_rand(rng, (n, k) if trans == "N" else (k, n), dt))
    for fast in (False, True):
        eager, _, work = g.herk(dA, N, uplo=uplo, trans=trans, fastmode=fast)
        torch.cuda.synchronize()
        out = torch.zeros_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.herk(dA, N, uplo=uplo, trans=trans, fastmode=fast, C_out=out, work=work)   # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        out.zero_()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            g.herk(dA, N, uplo=uplo, trans=trans, fastmode=fast, C_out=out, work=work)
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert gu.bits_equal(out.cpu().numpy(), eager.cpu().numpy())


@pytest.mark.parametrize("n,k", [(257, 1024), (37, 65)], ids=["257x1024", "37x65"])
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_one_operand_pass_leaves_the_gemms_planes(dt, trans, fast, n, k):
    """The five plane sets of the one pass, read through gemmul8_get_layout: A_lo parts 0 .. 2, B_lo parts 1 and 2 and sftA equal what the equivalent
    GEMM left in its own workspace; part 0 of B_lo is not written (the workspace comes in zeroed)."""
    rng = np.random.default_rng(9)
    N = 7
    A = _rand(rng, (n, k) if trans == "N" else (k, n), dt)
    _, ig = gu.hip_gemm(A, A, N, fastmode=fast, opA=trans, opB="C" if trans == "N" else "N", want_intermediates=True)
    work = torch.zeros(g.work_size(True, g.INT8, n, n, k, N)[0], dtype=torch.uint8, device="cuda")
    g.herk(gu.to_dev(A), N, uplo="L", trans=trans, fastmode=fast, work=work)
    torch.cuda.synchronize()
    ih = gu.read_intermediates(work, ol.DT[np.dtype(dt)], g.INT8, n, n, k, N)
    assert np.array_equal(ih["sftA"], ig["sftA"])
    assert np.array_equal(ih["A_lo"], ig["A_lo"]), "A_lo parts 0 .. 2"
    assert np.array_equal(ih["B_lo"][1:], ig["B_lo"][1:]), "B_lo parts 1 and 2: the conjugate twin's planes"
    assert np.array_equal(ig["B_lo"][0], ig["A_lo"][0]) and not ih["B_lo"][0].any()
    L = g.Layout()
    g.check(g.lib().gemmul8_get_layout(ol.DT[np.dtype(dt)], g.INT8, n, n, k, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    off = L.B_lo - work.data_ptr()
    assert not bool(work[off:off + L.part_strideB].any()), "part 0 of B_lo was written"
