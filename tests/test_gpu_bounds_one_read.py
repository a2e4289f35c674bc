"""Accurate mode's one-read bound extract of a row-strided operand (csrc/oz2_scale.hip, stage_panel_body; GEMMUL8_BOUNDS_ONE_READ) against the
two-pass form (row-maxima launch, then extract): bound planes, preliminary shifts, bound maxima, final shifts and C must be byte-identical, at the
edges of the tiling (16 / 32 rows, 128 k) and on data that takes every arm of the kernel -- the provisional shift of a tile too large by
d = 1, 6, 7, 8, 40 (rescaled from the plane), falling maxima (nothing rewritten), zero tiles and rows, subnormal rows, rows whose range
makes ldexp inexact (recomputed from a second read), NaN / +-Inf rows in both non-finite modes.  Unaligned operands walk tile by tile through guarded
loads; 16-byte aligned ones take the pipelined walk of the default path, so the grids run both ways.  One case runs with the knob unset (the default rule,
one operand above it and one below), one grid is also checked against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu

pytestmark = pytest.mark.gpu

KNOB = "GEMMUL8_BOUNDS_ONE_READ"
N_MOD = 8
NN = 16
MS = [1, 15, 16, 17, 33]
KS = [1, 127, 128, 129, 384, 1000]
RATIOS = [1, 6, 7, 8, 40]


def operand(rows, k, dtype, rng, shift, wide_rows=True):
    """Logical rows x k matrix of the row-strided operand; row r takes pattern (r + shift) % 8 (wide_rows=False: pattern 5 stays plain data)."""
    f32 = dtype == np.float32
    R = rng.uniform(-1.0, 1.0, (rows, k))
    nt = (k + 127) // 128
    tile = np.arange(k) // 128
    for r in range(rows):
        kind = (r + shift) % 8
        if kind == 0:    # maxima rising tile by tile: tile t is written with a shift too large by the sum of the later ratios
            e = np.cumsum([0] + [RATIOS[(r + shift + i) % 5] for i in range(nt - 1)])
            R[r] *= np.ldexp(1.0, (e - (60 if f32 else 200))[tile])
            R[r, 0::128] = np.ldexp(1.0, e - (60 if f32 else 200))  # exact powers of two as well
        elif kind == 1:  # falling maxima: the first tile holds the row maximum
            R[r] *= np.ldexp(1.0, -3 * tile)
        elif kind == 2:  # all-zero row
            R[r] = 0.0
        elif kind == 3:  # all-zero tiles in front of and between the others
            R[r, tile % 2 == 0] = 0.0
            R[r] *= np.ldexp(1.0, 9 * tile)
        elif kind == 4:  # subnormal row
            R[r] *= np.ldexp(1.0, -140 if f32 else -1050)
        elif kind == 5 and wide_rows:  # 1e-300 ... 1e300 in one row: ldexp of the small elements underflows (double)
            R[r] *= 10.0 ** rng.uniform(-37 if f32 else -300, 37 if f32 else 300, k)
            R[r, k // 2] = 1e37 if f32 else 1e300
            R[r, 0] = 1e-37 if f32 else 1e-300
        elif kind == 6:  # one late maximum far above the rest (d >= 8 everywhere before it), a subnormal among the rest
            R[r] *= 2.0 ** -30
            R[r, k - 1] = 3.0
            R[r, k // 3] = 2.0 ** -148 if f32 else 5e-324
        # kind 7: plain uniform data
    return R.astype(dtype)


def embed_cm(M, ld_extra, base_off, rng):
    """Column-major M inside a larger device buffer: base `base_off` elements in (element-aligned only), ld = rows + ld_extra."""
    buf, ld = gu.embed(M, ld_extra, base_off, rng)
    d = torch.from_numpy(buf).cuda()
    return d, d.data_ptr() + base_off * buf.dtype.itemsize, ld


def run(monkeypatch, knob, A, B, opA, opB, rng_seed, nf_mode=0, whole=True, aligned=False):
    """Bounds phase, then the whole call, with the knob forced to `knob` (None: unset, the default rule); everything the phase and the call leave behind
    as bytes.  aligned=False: lda > rows and a base that is only element-aligned (the kernel's guarded tile-by-tile walk); aligned=True: 16-byte aligned base
    and leading dimensions (lda = rows + 4), where full panels take the pipelined walk with unguarded loads."""
    gu.setknob(monkeypatch, KNOB, knob)
    rng = np.random.default_rng(rng_seed)
    m, k = (A.shape if opA == "N" else A.shape[::-1])
    n = B.shape[1] if opB == "N" else B.shape[0]
    if aligned:
        assert A.shape[0] % 4 == 0 and B.shape[0] % 4 == 0
        dA, pA, lda = embed_cm(A, 4, 0, rng)
        dB, pB, ldb = embed_cm(B, 4, 0, rng)
        assert pA % 16 == 0 and pB % 16 == 0
    else:
        dA, pA, lda = embed_cm(A, 3, 1, rng)   # lda > rows, base not 16-byte aligned
        dB, pB, ldb = embed_cm(B, 5, 1, rng)
    tdt = gu.NP2T[A.dtype]
    code = g._dtype_code(tdt)
    lib = g.lib()
    tot, _, _ = g.work_size(False, g.INT8, m, n, k, N_MOD)
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    work = torch.full((tot,), 0x5A, dtype=torch.uint8, device="cuda")
    L = g.Layout()
    g.check(lib.gemmul8_get_layout(code, g.INT8, m, n, k, N_MOD, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    g.check(lib.gemmul8_scale_bounds(st, code, g.INT8, g.OPS[opA], g.OPS[opB], m, n, k, pA, lda, pB, ldb, N_MOD, 0, n, C.byref(L), 0, 0))
    torch.cuda.synchronize()
    w = work.cpu().numpy()
    base = work.data_ptr()
    np_ = (n + 255) // 256 * 256
    out["A_bound"] = w[L.A_bound - base:L.A_bound - base + L.mp * L.kp].reshape(L.mp, L.kp)[:m].copy()
    out["B_bound"] = w[L.B_bound - base:L.B_bound - base + n * L.kp].reshape(n, L.kp).copy()
    out["sft0A"] = w[L.sftA - base:L.sftA - base + 2 * m].copy()
    out["sft0B"] = w[L.sftB - base:L.sftB - base + 2 * n].copy()
    mx = w[L.scratch - base:L.scratch - base + 4 * (L.mp + np_)]
    out["rowmax"], out["colmax"] = mx[:4 * m].copy(), mx[4 * L.mp:4 * L.mp + 4 * n].copy()
    assert not out["A_bound"][:, k:].any() and not out["B_bound"][:, k:].any(), "k-padding of a bound plane must be zero"
    if whole:
        prev = g.set_nonfinite_mode(nf_mode)
        try:
            work = torch.full((tot,), 0x5A, dtype=torch.uint8, device="cuda")
            Cd = torch.zeros((n, m), dtype=tdt, device="cuda")
            al, be = np.array([1.0], dtype=A.dtype), np.array([0.0], dtype=A.dtype)
            g.check(lib.gemmul8_gemm(st, code, g.INT8, g.OPS[opA], g.OPS[opB], m, n, k, al.ctypes.data, pA, lda, pB, ldb, be.ctypes.data,
                                     Cd.data_ptr(), m, N_MOD, 0, work.data_ptr(), None, None, 0, 0, 0, 0, None))
            torch.cuda.synchronize()
        finally:
            g.set_nonfinite_mode(prev)
        it = gu.read_intermediates(work, code, g.INT8, m, n, k, N_MOD)
        out["C"] = Cd.cpu().numpy().view(np.uint8)
        out["sftA"], out["sftB"] = it["sftA"].view(np.uint8), it["sftB"].view(np.uint8)
        out["A_lo"], out["B_lo"] = it["A_lo"], it["B_lo"]
    return out


def same(monkeypatch, A, B, opA, opB, seed, what, nf_mode=0, aligned=False, knob=1):
    on = run(monkeypatch, knob, A, B, opA, opB, seed, nf_mode, aligned=aligned)
    off = run(monkeypatch, 0, A, B, opA, opB, seed, nf_mode, aligned=aligned)
    for key in off:
        assert np.array_equal(on[key], off[key]), f"{what}: {key} differs in {int(np.sum(on[key] != off[key]))} bytes"


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("ops", [("N", "N"), ("T", "T"), ("N", "T")], ids=["A-strided", "B-strided", "both-strided"])
def test_one_read_equals_two_pass_at_the_tiling_edges(dtype, ops, monkeypatch):
    opA, opB = ops
    rng = np.random.default_rng(17)
    case = 0
    for m in MS:
        for k in KS:
            case += 1
            Ra = operand(m, k, dtype, rng, case)        # logical m x k
            Rb = operand(NN, k, dtype, rng, case + 3)   # logical n x k
            A = Ra if opA == "N" else np.ascontiguousarray(Ra.T)   # stored m x k (N) / k x m (T)
            B = Rb if opB == "T" else np.ascontiguousarray(Rb.T)   # stored n x k (T) / k x n (N)
            same(monkeypatch, A, B, opA, opB, case, f"m={m} k={k} {dtype.__name__} {opA}{opB}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("ops", [("N", "N"), ("T", "T"), ("N", "T")], ids=["A-strided", "B-strided", "both-strided"])
def test_one_read_equals_two_pass_on_the_pipelined_walk(dtype, ops, monkeypatch):
    """16-byte aligned operands, so that full panels (16 rows of double, 32 of float) take the unguarded, pipelined loads -- the walk of the default path:
    48 rows = full panels only (double) / one full and one ragged panel (float), 80 rows = two full panels and a ragged one (float); k = 384 (fewer full
    tiles than the ring of 4 holds), 640 and 768 (the ring wraps, with a partial last group), 700 and 1000 (a partial tile behind the pipelined ones)."""
    opA, opB = ops
    rng = np.random.default_rng(19)
    case = 0
    for m, n in ((48, 48), (80, 32)):
        for k in (384, 640, 700, 768, 1000):
            case += 1
            Ra = operand(m, k, dtype, rng, case)
            Rb = operand(n, k, dtype, rng, case + 3)
            A = Ra if opA == "N" else np.ascontiguousarray(Ra.T)
            B = Rb if opB == "T" else np.ascontiguousarray(Rb.T)
            if (A.shape[0] % 4) or (B.shape[0] % 4):   # (a K-major operand is stored k x rows: its leading dimension k must stay a multiple of 16 bytes too)
                continue
            same(monkeypatch, A, B, opA, opB, case, f"aligned m={m} n={n} k={k} {dtype.__name__} {opA}{opB}", aligned=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
def test_default_rule_with_operands_of_both_forms(dtype, monkeypatch):
    """The knob UNSET: A (8192 rows, aligned) is above the default rule's row count and takes the one-read form, B (row-strided, 16 rows) is below it and
    keeps the row-maxima launch -- one call with both forms, the row-maxima launch for B alone.  Same bytes as with the form forced off."""
    rng = np.random.default_rng(31)
    m, k = 8192, 128
    Ra = rng.uniform(-1.0, 1.0, (m, k))
    Ra[:64] = operand(64, k, dtype, rng, 0)
    Ra[-64:] = operand(64, k, dtype, rng, 5)
    Rb = operand(NN, k, dtype, rng, 1)
    same(monkeypatch, Ra.astype(dtype), Rb, "N", "T", 3, f"default rule m={m} k={k} {dtype.__name__}", aligned=True, knob=None)


@pytest.mark.parametrize("aligned", [False, True], ids=["guarded", "pipelined"])
@pytest.mark.parametrize("nf_mode", [0, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
def test_non_finite_rows_in_both_modes(dtype, nf_mode, aligned, monkeypatch):
    """NaN, +Inf and -Inf in the first, middle and last tile of rows of both row-strided operands (mode 0: the reference's behaviour, whatever it is;
    mode 1: sentinel rows) -- the same bytes either way."""
    rng = np.random.default_rng(23)
    for m, k in (((80, 1000), (48, 640)) if aligned else ((33, 1000), (17, 129))):
        nb = 32 if aligned else NN
        Ra = operand(m, k, dtype, rng, 7)   # (shift 7: row 0 is plain data)
        Rb = operand(nb, k, dtype, rng, 7)
        vals = [np.nan, np.inf, -np.inf]
        pos = [0, k // 2, k - 1]
        i = 0
        for v in vals:
            for p in pos:
                Ra[(2 * i) % m, p] = v
                Rb[(i + 1) % nb, p] = v
                i += 1
        Ra[m - 1, 3] = np.nan          # a NaN below a finite maximum, an Inf next to a NaN
        Ra[m - 1, k - 1] = np.inf
        same(monkeypatch, Ra, Rb, "N", "T", m, f"non-finite mode {nf_mode} m={m} k={k}", nf_mode, aligned=aligned)


def test_one_read_against_the_oracle(monkeypatch):
    """The forced one-read form through the oracle helpers: bound planes, sft0 and bound maxima bit for bit, then the whole call."""
    gu.setknob(monkeypatch, KNOB, 1)
    rng = np.random.default_rng(29)
    m, k = 33, 1000
    Ra = operand(m, k, np.float64, rng, 0, wide_rows=False)  # (rows spanning 600 binades overflow the product: not an oracle case)
    Rb = operand(NN, k, np.float64, rng, 3, wide_rows=False)
    gu.parity_case(Ra, Rb, N_MOD, False, opA="N", opB="T")  # (bounds_case first, then the whole call)
