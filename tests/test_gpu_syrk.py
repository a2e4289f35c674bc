"""gemmul8_syrk on the GPU: the stored triangle carries the bits of the equivalent GEMM of A with its transpose -- run in the same process
and, through the oracle with the device's shifts, as parity_case does --, every byte of the enclosing C buffer outside the triangle keeps its
sentinel, device-resident scalars, HIP-graph replay and the GEMMUL8_EPI_NT policies give the same bits.

(a) and (c) run over the WHOLE grid: 4 types x 2 trans x 2 uplo x 2 modes x 4 scalar pairs x every moduli count of the type x 8 shapes, one
test per (type, shape), buffers and comparisons on the device; the ldc padding 1 / 7 / 64 rotates through the calls of a test, so every padding
meets every type and shape.  (b) costs the CPU oracle about n^2 k N (x 4 for complex) / 1e9 seconds per GEMM, so it runs on a subset: for every
type and shape, one oracle GEMM per mode at the six small shapes and one at the two large ones (2 moduli there: 10 to 40 s each), both triangles
compared with it, the other parameters rotating deterministically.  Every case of (b)'s complement is tied to the same GEMM bits by (a), and
tests/test_gpu_parity.py holds gemmul8_gemm against the oracle."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol

pytestmark = pytest.mark.gpu

DTS = [np.float32, np.float64, np.complex64, np.complex128]
SHAPES = [(1, 1), (37, 65), (256, 300), (257, 1024), (700, 129), (1031, 257), (2304, 512), (4352, 256)]   # 2304 = 9 tile-rows, 4352 = 17
SCALARS = [(1, 0), (-1, 1), (0.75, -0.5), (0, 2)]
CSCALARS = [(1, 0), (-1, 1), (0.75 - 0.25j, -0.5 + 1.5j), (0, 2 - 1j)]
SENTINEL = 0xA5
LD_EXTRA = (1, 7, 64)


def _moduli(dt):
    return [2, 7, 13] if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4 else [2, 7, 14, 20]


def _oracle_cases():
    """(b): (type, n, k, trans, mode, scalar pair, moduli, ld_extra); both uplo are compared with the one oracle GEMM of a case"""
    out = []
    for si, (n, k) in enumerate(SHAPES):
        for di, dt in enumerate(DTS):
            mods = _moduli(dt)
            for r in range(2 if n <= 1031 else 1):
                j = si * 5 + di * 3 + r
                fast = bool(r) if n <= 1031 else bool((si + di) % 2)
                out.append((dt, n, k, "NT"[(j // 2 + di) % 2], fast, (j + si) % 4, mods[(j + di) % len(mods)] if n <= 1031 else 2, LD_EXTRA[j % 3]))
    return out


ORACLE_CASES = _oracle_cases()


def test_the_oracle_subset_covers_every_value_with_every_type():
    for dt in DTS:
        mine = [c for c in ORACLE_CASES if c[0] is dt]
        assert {c[3] for c in mine} == {"N", "T"} and {c[4] for c in mine} == {False, True}
        assert {c[5] for c in mine} == {0, 1, 2, 3} and {c[6] for c in mine} == set(_moduli(dt)) and {c[7] for c in mine} == set(LD_EXTRA)
        assert {(c[1], c[2]) for c in mine} == set(SHAPES)
        for n, k in SHAPES[:6]:
            assert {c[4] for c in mine if c[1] == n} == {False, True}
    large = [c for c in ORACLE_CASES if c[1] > 1031]
    assert {(c[0], c[1]) for c in large} == set(itertools.product(DTS, (2304, 4352)))
    assert {c[3] for c in large} == {"N", "T"} and {c[4] for c in large} == {False, True}


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    if np.dtype(dt).kind == "c":
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    return a.astype(dt)


def _tri_mask(n, uplo):
    i, j = np.indices((n, n))
    return i >= j if uplo == "L" else i <= j


def _syrk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0, alpha_beta_dev=False):
    """gemmul8_syrk on a C embedded with ldc = n + ld_extra in a sentinel-filled buffer whose triangle holds C0's; returns (result, buffer before) as uint8 [n][ldc][esz]"""
    esz = np.dtype(dt).itemsize
    ldc = n + ld_extra
    buf = np.full((n, ldc, esz), SENTINEL, np.uint8)   # column j at buf[j]
    mk = _tri_mask(n, uplo)
    win = buf[:, :n, :]
    win[mk.T] = np.ascontiguousarray(C0.T).view(np.uint8).reshape(n, n, esz)[mk.T]
    dC = torch.from_numpy(buf.copy()).cuda()
    dA = gu.to_dev(A)
    tot, _, _ = g.work_size(np.dtype(dt).kind == "c", g.INT8, n, n, k, N)
    work = torch.full((tot,), 0x3C, dtype=torch.uint8, device="cuda")
    al, be = np.array([alpha], dtype=dt), np.array([beta], dtype=dt)
    if alpha_beta_dev:
        dal, dbe = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
        pa, pb = dal.data_ptr(), dbe.data_ptr()
    else:
        pa, pb = al.ctypes.data, be.ctypes.data
    rc = g.lib().gemmul8_syrk(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.UPLO[uplo], g.OPS[trans], n, k, pa, dA.data_ptr(),
                              dA.shape[1], pb, dC.data_ptr(), ldc, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_syrk")
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
    """(a) and (c) for every trans x uplo x mode x scalar pair x moduli count of this type and shape: 32 x 3 or 4 SYRK calls against 16 x 3 or 4 GEMMs"""
    rng = np.random.default_rng(n * 131 + k)
    cplx = np.dtype(dt).kind == "c"
    w = np.dtype(dt).itemsize // 4
    dAs = {"N": gu.to_dev(_rand(rng, (n, k), dt)), "T": gu.to_dev(_rand(rng, (k, n), dt))}
    C0 = gu.to_dev(_rand(rng, (n, n), dt))
    C0w = _words(C0)
    tri = {"L": torch.ones((n, n), dtype=torch.bool, device="cuda").triu(), "U": torch.ones((n, n), dtype=torch.bool, device="cuda").tril()}  # [col][row]
    triw = {u: m.repeat_interleave(w, dim=1) for u, m in tri.items()}
    work = torch.empty(g.work_size(cplx, g.INT8, n, n, k, max(_moduli(dt)))[0], dtype=torch.uint8, device="cuda")
    call = 0
    for N, trans, fast, sc in itertools.product(_moduli(dt), "NT", (False, True), range(4)):
        alpha, beta = (CSCALARS if cplx else SCALARS)[sc]
        Cg, _, _ = g.gemm(dAs[trans], dAs[trans], N, fastmode=fast, opA=trans, opB="T" if trans == "N" else "N", alpha=alpha, beta=beta, C_out=C0.clone(), work=work)
        Cgw = _words(Cg)
        for uplo in "LU":
            ldc = n + LD_EXTRA[call % 3]
            call += 1
            before = torch.full((n, ldc * w), int(np.array([SENTINEL] * 4, np.uint8).view(np.int32)[0]), dtype=torch.int32, device="cuda")
            before[:, :n * w] = torch.where(triw[uplo], C0w, before[:, :n * w])
            buf = before.clone()
            Cd = buf.view(torch.float32 if w == 1 else torch.float64) if not cplx else torch.view_as_complex(buf.view(torch.float32 if w == 2 else torch.float64).reshape(n, ldc, 2))
            assert Cd.shape == (n, ldc) and Cd.data_ptr() == buf.data_ptr()
            g.syrk(dAs[trans], N, uplo=uplo, trans=trans, fastmode=fast, alpha=alpha, beta=beta, C_out=Cd, work=work)
            torch.cuda.synchronize()
            what = f"N={N} trans={trans} uplo={uplo} fast={fast} scalars={sc} ldc={ldc}"
            diff = buf != before
            inside = torch.zeros((n, ldc * w), dtype=torch.bool, device="cuda")
            inside[:, :n * w] = triw[uplo]
            assert not bool((diff & ~inside).any()), "bytes outside the stored triangle were written: " + what                       # (c)
            bad = (buf[:, :n * w] != Cgw) & triw[uplo]
            assert not bool(bad.any()), f"{int(bad.sum())} words of the triangle differ from gemmul8_gemm(A, A^T): " + what          # (a)


@pytest.mark.parametrize("dt,n,k,trans,fast,sc,N,ld_extra", ORACLE_CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1]}x{c[2]}-{c[3]}-{'fast' if c[4] else 'accu'}-s{c[5]}-N{c[6]}-ld{c[7]}" for c in ORACLE_CASES])
def test_triangle_bits_equal_the_oracles_gemm(dt, n, k, trans, fast, sc, N, ld_extra):
    """(b), with (a) and (c) on the host side: both triangles against ONE oracle GEMM run with the device's shifts"""
    rng = np.random.default_rng(n * 131 + k)
    cplx = np.dtype(dt).kind == "c"
    alpha, beta = (CSCALARS if cplx else SCALARS)[sc]
    A = _rand(rng, (n, k) if trans == "N" else (k, n), dt)
    C0 = _rand(rng, (n, n), dt)
    esz = np.dtype(dt).itemsize
    opB = "T" if trans == "N" else "N"
    Cg, it = gu.hip_gemm(A, A, N, fastmode=fast, opA=trans, opB=opB, alpha=alpha, beta=beta, C0=C0, want_intermediates=True)
    Co = ol.gemm(A, A, N, fastmode=fast, opA=trans, opB=opB, alpha=alpha, beta=beta, C0=C0, sftA_in=it["sftA"], sftB_in=it["sftB"])
    ref = np.ascontiguousarray(Cg.T).view(np.uint8).reshape(n, n, esz)
    refo = np.ascontiguousarray(np.asarray(Co).T).view(np.uint8).reshape(n, n, esz)
    for uplo in "LU":
        out, buf = _syrk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, ld_extra, C0)
        mk = _tri_mask(n, uplo)
        keep = np.ones(out.shape[:2], bool)
        keep[:, :n] = ~mk.T
        assert np.array_equal(out[keep], buf[keep]), "bytes outside the stored triangle were written"
        got = out[:, :n, :]
        bad = (got != ref).any(axis=2) & mk.T
        assert not bad.any(), f"uplo {uplo}: {bad.sum()} entries of the triangle differ from gemmul8_gemm(A, A^T); first at (col, row) {np.argwhere(bad)[:3].tolist()}"
        bad = (got != refo).any(axis=2) & mk.T
        assert not bad.any(), f"uplo {uplo}: {bad.sum()} entries of the triangle differ from the oracle's GEMM"


@pytest.mark.parametrize("dt", DTS)
def test_beta_zero_never_reads_c_and_nan_outside_is_not_read(dt):
    """beta == 0 (host scalars, general form: alpha = 0.75): a C full of NaN gives the finite result; beta != 0: NaN in the OTHER triangle stays out."""
    rng = np.random.default_rng(5)
    n, k, N = 300, 77, 7
    A = _rand(rng, (n, k), dt)
    nan = np.full((n, n), np.nan, dt)
    for uplo in "LU":
        mk = _tri_mask(n, uplo)
        Cd, _, _ = g.syrk(gu.to_dev(A), N, uplo=uplo, alpha=0.75, beta=0.0, C_out=gu.to_dev(nan.copy()))
        torch.cuda.synchronize()
        C = gu.from_dev(Cd)
        assert np.isfinite(C[mk]).all() and np.isnan(C[~mk]).all()
        C0 = _rand(rng, (n, n), dt)
        C0[~mk] = np.nan
        Cd, _, _ = g.syrk(gu.to_dev(A), N, uplo=uplo, alpha=0.75, beta=-0.5, C_out=gu.to_dev(C0.copy()))
        torch.cuda.synchronize()
        assert np.isfinite(gu.from_dev(Cd)[mk]).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("uplo,trans", [("U", "T"), ("L", "N")])
def test_device_resident_scalars(dt, fast, uplo, trans):
    rng = np.random.default_rng(6)
    n, k, N = 700, 129, 7
    cplx = np.dtype(dt).kind == "c"
    alpha, beta = (CSCALARS if cplx else SCALARS)[2]
    A = _rand(rng, (k, n) if trans == "T" else (n, k), dt)
    C0 = _rand(rng, (n, n), dt)
    host, _ = _syrk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0)
    dev, _ = _syrk_embedded(A, dt, n, k, uplo, trans, fast, alpha, beta, N, 7, C0, alpha_beta_dev=True)
    assert np.array_equal(host, dev)


@pytest.mark.parametrize("dt", [np.float64, np.complex64])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "T")])
def test_graph_capture_replays_to_the_same_bits(dt, uplo, trans):
    rng = np.random.default_rng(7)
    n, k, N = 1031, 257, 7
    A = _rand(rng, (n, k) if trans == "N" else (k, n), dt)
    dA = gu.to_dev(A)
    for fast in (False, True):
        eager, _, work = g.syrk(dA, N, uplo=uplo, trans=trans, fastmode=fast)
        torch.cuda.synchronize()
        out = torch.zeros_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.syrk(dA, N, uplo=uplo, trans=trans, fastmode=fast, C_out=out, work=work)   # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        out.zero_()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            g.syrk(dA, N, uplo=uplo, trans=trans, fastmode=fast, C_out=out, work=work)
        for _ in range(2):
            out.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert gu.bits_equal(out.cpu().numpy(), eager.cpu().numpy())


@pytest.mark.parametrize("dt", DTS)
def test_epi_nt_policies_give_the_same_bits(dt, monkeypatch):
    rng = np.random.default_rng(8)
    n, k, N = 2304, 300, 7
    A = _rand(rng, (n, k), dt)
    dA = gu.to_dev(A)
    res = []
    for nt in (None, 0, 1):
        gu.setknob(monkeypatch, "GEMMUL8_EPI_NT", nt)
        Cd, _, _ = g.syrk(dA, N, uplo="U", fastmode=True)
        torch.cuda.synchronize()
        res.append(Cd.cpu().numpy())
    assert gu.bits_equal(res[0], res[1]) and gu.bits_equal(res[0], res[2])
