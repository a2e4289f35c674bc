"""gemmul8_symm / gemmul8_hemm on the GPU (include/gemmul8_c.h): the m x n window of C carries the bits of the equivalent GEMM -- gemmul8_gemm, whose code
this feature does not touch, on the materialised Afull, run in the same process -- whatever the other strict triangle of A, its lda padding and (HEMM) the
diagonal's imaginary parts hold; the enclosing buffers of A, B and C keep every other byte; device-resident scalars; the CPU oracle; HIP-graph replay.

(a), (b) and (c) run over the WHOLE grid, one test per (routine and type, shape), buffers and comparisons on the device: 2 sides x 2 uplo x 2 modes x 4 scalar
pairs x the moduli counts of the type, each point once with a finite A and once with the unused parts of A poisoned with NaN; the ld padding 1 / 7 / 64 and
the element offset 0 / 1 of every base rotate through the calls (offset 1 and the odd paddings take the scalar-load paths, 64 with offset 0 the 16-byte ones).

Shapes (ka, other dimension), the smallest at which each mechanism can fail: (1, 1); (37, 5): one partial tile, all of it crossed by the diagonal;
(128, 64): exactly one k tile -- stored, mirrored and diagonal row tiles side by side; (129, 33): a k tile one column wide and a mirrored tile one row high;
(256, 256): no padding; (257, 40): the pad edge, kp = 512; (300, 257): the other dimension across a 256 block; (1100, 64): kp = 1280 past a 1024 chunk,
several k splits of the maxima pass.

(e) costs the CPU oracle about m n ka N (x 4 for complex) / 1e9 seconds per GEMM (at most 4.3 s here), so it runs on a subset: every routine and type at every
shape, sides, triangles, modes, scalar pairs and moduli counts rotating."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol
from symm_util import equivalent_ops, is_cplx, materialise, poison

pytestmark = pytest.mark.gpu

ROUTINES = [(np.float32, False), (np.float64, False), (np.complex64, False), (np.complex128, False), (np.complex64, True), (np.complex128, True)]
RIDS = [("hemm-" if h else "symm-") + np.dtype(d).name for d, h in ROUTINES]
SHAPES = [(1, 1), (37, 5), (128, 64), (129, 33), (256, 256), (257, 40), (300, 257), (1100, 64)]
SCALARS = [(1, 0), (-1, 1), (0.75, -0.5), (0, 2)]
CSCALARS = [(1, 0), (-1, 1), (0.75 - 0.25j, -0.5 + 1.5j), (0, 2 - 1j)]
SENTINEL = 0xA5
LD_EXTRA = (1, 7, 64)
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.complex64): torch.complex64,
            np.dtype(np.complex128): torch.complex128}


def _moduli(dt):
    return [2, 7, 13] if np.dtype(dt).itemsize // (2 if is_cplx(dt) else 1) == 4 else [2, 7, 14, 20]


def _rand(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    if is_cplx(dt):
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    return a.astype(dt)


def _dims(ka, other, side):
    """(m, n) of B and C"""
    return (ka, other) if side == "L" else (other, ka)


class Embedded:
    """a column-major matrix inside a larger device buffer: ld = rows + ld_extra, base `off` elements in, every other byte = `fill`"""

    def __init__(self, M, ld_extra, off, fill=SENTINEL):
        Md = gu.to_dev(M) if isinstance(M, np.ndarray) else M   # (a device tensor: already (cols, rows))
        dt = Md.dtype
        cols, rows = Md.shape
        self.rows, self.cols, self.ld, self.off = rows, cols, rows + ld_extra, off
        self.esz = Md.element_size()
        nelem = off + cols * self.ld + 3
        self.bytes = torch.full((nelem * self.esz,), fill, dtype=torch.uint8, device="cuda")
        if dt.is_complex:
            flat = torch.view_as_complex(self.bytes.view(torch.float32 if dt == torch.complex64 else torch.float64).reshape(nelem, 2))
        else:
            flat = self.bytes.view(dt)
        assert flat.data_ptr() == self.bytes.data_ptr() and flat.numel() == nelem
        self.view = flat.as_strided((cols, rows), (self.ld, 1), off)
        self.view.copy_(Md)
        inside = torch.zeros(nelem, dtype=torch.bool, device="cuda")
        inside.as_strided((cols, rows), (self.ld, 1), off).fill_(True)
        self.inside = inside.repeat_interleave(self.esz)
        self.before = self.bytes.clone()

    def ptr(self):
        return self.view.data_ptr()

    def window_words(self):
        return _words(self.view.contiguous())


def _words(x):
    """a contiguous (cols, rows) tensor of any of the four types as its int32 words"""
    if x.is_complex():
        x = torch.view_as_real(x).reshape(x.shape[0], -1)
    return x.contiguous().view(torch.int32)


def _symm_call(herm, dt, side, uplo, m, n, alpha, beta, A, B, Cm, N, fast, work, scalars_dev=False):
    al, be = np.array([alpha], dtype=dt), np.array([beta], dtype=dt)
    if scalars_dev:
        dal, dbe = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
        pa, pb = dal.data_ptr(), dbe.data_ptr()
    else:
        pa, pb = al.ctypes.data, be.ctypes.data
    fn = g.lib().gemmul8_hemm if herm else g.lib().gemmul8_symm
    rc = fn(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.SIDE[side], g.UPLO[uplo], m, n, pa, A.ptr(), A.ld, B.ptr(), B.ld, pb,
            Cm.ptr(), Cm.ld, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_hemm" if herm else "gemmul8_symm")
    torch.cuda.synchronize()


def _gemm_ref(Afull_d, B_d, side, herm, N, fast, alpha, beta, C0_d, work):
    opA, opB = equivalent_ops(side, herm)
    left, right = (Afull_d, B_d) if side == "L" else (B_d, Afull_d)
    return g.gemm(left, right, N, fastmode=fast, opA=opA, opB=opB, alpha=alpha, beta=beta, C_out=C0_d.clone(), work=work)[0]


def _poisoned(A, uplo, herm, ld_extra, off):
    """A's triangle `uplo` inside a buffer in which every other byte -- the other strict triangle, the ld padding, the surroundings and (herm) the
    diagonal's imaginary parts -- is 0xFF: NaN in all four types"""
    return Embedded(A if isinstance(A, torch.Tensor) else poison(A, uplo, herm), ld_extra, off, fill=0xFF)   # (a device tensor: poisoned by the caller)


@pytest.mark.parametrize("ka,other", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
@pytest.mark.parametrize("dt,herm", ROUTINES, ids=RIDS)
def test_whole_grid_window_is_the_gemms_and_nothing_else_is_touched(dt, herm, ka, other):
    """(a), (b), (c) for every side x uplo x mode x scalar pair x moduli count of this routine, type and shape"""
    rng = np.random.default_rng(ka * 131 + other)
    cplx = is_cplx(dt)
    A = _rand(rng, (ka, ka), dt)
    A_d, Apois_d = gu.to_dev(A), {u: gu.to_dev(poison(A, u, herm)) for u in "LU"}
    Afull_d = {u: gu.to_dev(materialise(A, u, herm)) for u in "LU"}
    Bs = {s: _rand(rng, _dims(ka, other, s), dt) for s in "LR"}
    B_d = {s: gu.to_dev(Bs[s]) for s in "LR"}
    C0 = {s: _rand(rng, _dims(ka, other, s), dt) for s in "LR"}
    C0_d = {s: gu.to_dev(C0[s]) for s in "LR"}
    nanC_d = {s: gu.to_dev(np.full(_dims(ka, other, s), np.nan, dt)) for s in "LR"}
    work = torch.empty(max(g.symm_work_size(cplx, *_dims(ka, other, s), s, max(_moduli(dt))) for s in "LR"), dtype=torch.uint8, device="cuda")
    call = 0
    for N, side, fast, sc in itertools.product(_moduli(dt), "LR", (False, True), range(4)):
        m, n = _dims(ka, other, side)
        alpha, beta = (CSCALARS if cplx else SCALARS)[sc]
        for uplo in "LU":
            ref = _words(_gemm_ref(Afull_d[uplo], B_d[side], side, herm, N, fast, alpha, beta, C0_d[side], work))
            for poisoned in (False, True):
                ex, off = [LD_EXTRA[(call + j) % 3] for j in range(3)], [(call >> j) & 1 for j in range(3)]
                call += 1
                EA = _poisoned(Apois_d[uplo], uplo, herm, ex[0], off[0]) if poisoned else Embedded(A_d, ex[0], off[0])
                EB = Embedded(B_d[side], ex[1], off[1])
                EC = Embedded(nanC_d[side] if beta == 0 else C0_d[side], ex[2], off[2])   # (c): beta == 0 over a NaN C
                _symm_call(herm, dt, side, uplo, m, n, alpha, beta, EA, EB, EC, N, fast, work)
                what = f"N={N} side={side} uplo={uplo} fast={fast} scalars={sc} poisoned={poisoned} ld+{ex} off={off}"
                assert torch.equal(EA.bytes, EA.before) and torch.equal(EB.bytes, EB.before), "A or B was written: " + what
                assert not bool(((EC.bytes != EC.before) & ~EC.inside).any()), "bytes outside the m x n window of C were written: " + what
                got = EC.window_words()
                bad = got != ref
                assert not bool(bad.any()), f"{int(bad.sum())} words of C differ from gemmul8_gemm on the materialised matrix: " + what   # (a), (b)
                if beta == 0:
                    out = EC.view.contiguous()
                    assert not bool(torch.isnan(torch.view_as_real(out) if cplx else out).any()), "beta == 0 read C: " + what            # (c)


def _oracle_cases():
    """(e): (routine index, ka, other, side, uplo, fast, scalar pair, moduli, (ld_extra, offset))"""
    out = []
    for si, (ka, other) in enumerate(SHAPES):
        for ri, (dt, herm) in enumerate(ROUTINES):
            mods = _moduli(dt)
            N = mods[(si + ri) % len(mods)]
            while _oracle_seconds(dt, ka, other, N) > 5 and N > 2:   # the next smaller count of the type
                N = mods[mods.index(N) - 1]
            out.append((ri, ka, other, "LR"[(si + ri) % 2], "LU"[(si // 4 + si + ri) % 2], bool((si // 2 + ri) % 2), (si + ri) % 4, N,
                        (LD_EXTRA[(si + ri) % 3], (si // 2 + ri) % 2)))
    return out


def _oracle_seconds(dt, ka, other, N):
    return ka * ka * other * N * (4 if is_cplx(dt) else 1) / 1e9


ORACLE_CASES = _oracle_cases()



def test_the_oracle_subset_covers_every_routine_at_every_shape_both_sides_and_modes():
    for ri in range(len(ROUTINES)):
        mine = [c for c in ORACLE_CASES if c[0] == ri]
        assert {(c[1], c[2]) for c in mine} == set(SHAPES)
        assert {c[3] for c in mine} == {"L", "R"} and {c[4] for c in mine} == {"L", "U"} and {c[5] for c in mine} == {False, True}
        assert {(c[3], c[5]) for c in mine} == set(itertools.product("LR", (False, True)))
        assert len({c[6] for c in mine}) >= 3 and len({c[7] for c in mine}) >= 2 and {c[7] for c in mine} <= set(_moduli(ROUTINES[ri][0]))
    for c in ORACLE_CASES:
        assert _oracle_seconds(ROUTINES[c[0]][0], c[1], c[2], c[7]) <= 5, c


@pytest.mark.parametrize("ri,ka,other,side,uplo,fast,sc,N,emb", ORACLE_CASES,
                         ids=[f"{RIDS[c[0]]}-{c[1]}x{c[2]}-{c[3]}{c[4]}-{'fast' if c[5] else 'accu'}-s{c[6]}-N{c[7]}-ld{c[8][0]}o{c[8][1]}" for c in ORACLE_CASES])
def test_window_bits_equal_the_oracles_gemm(ri, ka, other, side, uplo, fast, sc, N, emb):
    """(e): against the CPU oracle's equivalent GEMM run with the device's shifts, as gpu_util.parity_case does; A's unused parts are NaN"""
    dt, herm = ROUTINES[ri]
    rng = np.random.default_rng(ka * 131 + other + ri)
    cplx = is_cplx(dt)
    alpha, beta = (CSCALARS if cplx else SCALARS)[sc]
    m, n = _dims(ka, other, side)
    A, B, C0 = _rand(rng, (ka, ka), dt), _rand(rng, (m, n), dt), _rand(rng, (m, n), dt)
    Afull = materialise(A, uplo, herm)
    opA, opB = equivalent_ops(side, herm)
    left, right = (Afull, B) if side == "L" else (B, Afull)
    Cg, it = gu.hip_gemm(left, right, N, fastmode=fast, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0, want_intermediates=True)
    Co = ol.gemm(left, right, N, fastmode=fast, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0, sftA_in=it["sftA"], sftB_in=it["sftB"])
    EA, EB, EC = _poisoned(A, uplo, herm, emb[0], emb[1]), Embedded(B, emb[0], 1 - emb[1]), Embedded(C0, emb[0], emb[1])
    work = torch.full((g.symm_work_size(cplx, m, n, side, N),), 0x3C, dtype=torch.uint8, device="cuda")
    _symm_call(herm, dt, side, uplo, m, n, alpha, beta, EA, EB, EC, N, fast, work)
    got = gu.from_dev(EC.view.contiguous())
    assert gu.bits_equal(got, np.ascontiguousarray(Cg)), "differs from gemmul8_gemm on the materialised matrix"
    assert gu.bits_equal(got, np.ascontiguousarray(np.asarray(Co))), "differs from the oracle's GEMM"
    assert not bool(((EC.bytes != EC.before) & ~EC.inside).any())


@pytest.mark.parametrize("dt,herm", ROUTINES, ids=RIDS)
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("side,uplo", [("L", "U"), ("R", "L")])
def test_device_resident_scalars(dt, herm, fast, side, uplo):
    """(d)"""
    rng = np.random.default_rng(6)
    ka, other, N = 300, 257, 7
    m, n = _dims(ka, other, side)
    alpha, beta = (CSCALARS if is_cplx(dt) else SCALARS)[2]
    A, B, C0 = _rand(rng, (ka, ka), dt), _rand(rng, (m, n), dt), _rand(rng, (m, n), dt)
    work = torch.empty(g.symm_work_size(is_cplx(dt), m, n, side, N), dtype=torch.uint8, device="cuda")
    outs = []
    for dev in (False, True):
        EA, EB, EC = Embedded(A, 7, 0), Embedded(B, 1, 1), Embedded(C0, 64, 0)
        _symm_call(herm, dt, side, uplo, m, n, alpha, beta, EA, EB, EC, N, fast, work, scalars_dev=dev)
        outs.append(EC.bytes)
    assert torch.equal(outs[0], outs[1])
    ref = _words(_gemm_ref(gu.to_dev(materialise(A, uplo, herm)), gu.to_dev(B), side, herm, N, fast, alpha, beta, gu.to_dev(C0), work))
    assert torch.equal(EC.window_words(), ref)


@pytest.mark.parametrize("dt,herm", [(np.float64, False), (np.complex64, True)], ids=["symm-float64", "hemm-complex64"])
@pytest.mark.parametrize("side,uplo", [("L", "L"), ("R", "U")])
def test_graph_capture_replays_to_the_same_bits(dt, herm, side, uplo):
    """(f): a single-stream call with timers_ns == NULL, captured once and replayed"""
    rng = np.random.default_rng(7)
    ka, other, N = 300, 129, 7
    m, n = _dims(ka, other, side)
    dA, dB = gu.to_dev(_rand(rng, (ka, ka), dt)), gu.to_dev(_rand(rng, (m, n), dt))
    fn = g.hemm if herm else g.symm
    for fast in (False, True):
        eager, _, work = fn(dA, dB, N, side=side, uplo=uplo, fastmode=fast)
        torch.cuda.synchronize()
        out = torch.zeros_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(dA, dB, N, side=side, uplo=uplo, fastmode=fast, C_out=out, work=work)   # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        out.zero_()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn(dA, dB, N, side=side, uplo=uplo, fastmode=fast, C_out=out, work=work)
        for _ in range(2):
            out.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert gu.bits_equal(out.cpu().numpy(), eager.cpu().numpy())


def test_python_wrapper_matches_the_gemm_and_takes_views():
    """g.symm / g.hemm: defaults, a fresh zero-filled C_out, and a sub-matrix view of A with a larger leading dimension"""
    rng = np.random.default_rng(8)
    ka, other, N = 129, 33, 7
    for (dt, herm), side in zip(ROUTINES, "LRLRLR"):
        m, n = _dims(ka, other, side)
        A, B = _rand(rng, (ka, ka), dt), _rand(rng, (m, n), dt)
        EA = _poisoned(A, "U", herm, 7, 1)
        Cd, tm, _ = (g.hemm if herm else g.symm)(EA.view, gu.to_dev(B), N, side=side, uplo="U", timers=True)
        torch.cuda.synchronize()
        assert len(tm) == 4 and tm[0] > 0 and tm[1] > 0 and tm[3] > 0
        opA, opB = equivalent_ops(side, herm)
        Af = gu.to_dev(materialise(A, "U", herm))
        left, right = (Af, gu.to_dev(B)) if side == "L" else (gu.to_dev(B), Af)
        Cg = g.gemm(left, right, N, opA=opA, opB=opB)[0]
        torch.cuda.synchronize()
        assert torch.equal(_words(Cd), _words(Cg))
