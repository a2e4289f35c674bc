"""gemmul8_syrk, gemmul8_herk and gemmul8_syr2k where their three suites do not go: edge data, every residue-GEMM schedule under the triangular tile
walk, the k limits, and the driver paths that only a knob or a large n selects.  Everything is bit equality, through gpu_util.rank_k_case:

  (a) every word of the stored triangle equals the equivalent GEMM run in the same process (SYRK: gemmul8_gemm(A, A^T); HERK: gemmul8_gemm(A, A^H) with
      scalars (alpha, 0), (beta, 0), the diagonal holding that GEMM's real part and +0.0 over an incoming NaN; SYR2K: gemmul8_gemm on the K-concatenated P
      and Q of tests/test_syr2k_premise.py);
  (b) the triangle equals the CPU oracle's GEMM fed with the device GEMM's shifts, and the oracle's C is finite in every entry;
  (c) every byte of the sentinel-filled C buffer outside the triangle is unchanged (the ldc padding rotates through 1 / 7 / 64);
  and the whole buffers of A and B are byte-identical after the call.

1. Edge data (EDGE_REAL / EDGE_CPLX).  Row i of op(A) takes pattern i % P, so every pattern meets every other in C; for SYR2K row i of op(B) takes pattern
   (i + 3) % P, and the patterns are ordered so that an all-zero row of A meets a -0.0 row of B, a zero row of A a large row of B and a large row of A a
   subnormal row of B (asserted below without a GPU).  Span 60 for the float types and 450 for the double types, as in test_extreme_exponents_bit_exact:
   the largest row is below 2^(span - 1) in magnitude, so a sum of k <= 257 squares stays below 2^(2 span + 7) -- inside both types' ranges.
2. The ping-pong kernel (padded inner k = 5632 > 5120) and the K-step-barrier kernel (513 ... 5120) over five tile-rows, and k at each routine's limit.
3. Forced paths: GEMMUL8_SCALE_FOLD=0, GEMMUL8_CPLX_CHUNK, GEMMUL8_BOUND_TILE, GEMMUL8_BOUNDS_ONE_READ, and the default rule of the one-read bound
   extract at n = 8192 (the production path of a large DSYRK: no row-maxima launch at all)."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
from test_gpu_bounds_one_read import operand

gpu = pytest.mark.gpu   # per test: test_the_pattern_tables_hold_what_the_file_promises needs no GPU

ROUTINE_DTS = [(r, dt) for r in gu.RANK_K for dt in ([np.float32, np.float64, np.complex64, np.complex128] if r != "herk" else [np.complex64, np.complex128])]
RD_IDS = [f"{r}-{np.dtype(dt).name}" for r, dt in ROUTINE_DTS]
# one real and one complex type per routine (HERK has complex types only)
TWO_DTS = [(r, dt) for r in gu.RANK_K for dt in ([np.float64, np.complex64] if r != "herk" else [np.complex64, np.complex128])]
TWO_IDS = [f"{r}-{np.dtype(dt).name}" for r, dt in TWO_DTS]

EDGE_REAL = ["subnormal", "zero", "third_zero", "last_column", "minus_zero", "plain", "small", "large", "wide", "pow2"]
EDGE_CPLX = ["pure_real", "zero", "third_zero", "last_column", "minus_zero", "plain", "small", "large", "wide", "pow2", "subnormal", "pure_imag",
             "re_subnormal_im_large", "re_large_im_subnormal"]


def _cplx(dt):
    return np.dtype(dt).kind == "c"


def _single(dt):
    return np.dtype(dt).itemsize // (2 if _cplx(dt) else 1) == 4


def _trans(routine, t):
    return "C" if routine == "herk" and t == "T" else t


def _scalars(routine, dt):
    """the pairs (1, 0) and (0.75, -0.5) -- the suites' complex pair for SYRK / SYR2K on the complex types"""
    return [(1, 0), (0.75 - 0.25j, -0.5 + 1.5j) if _cplx(dt) and routine != "herk" else (0.75, -0.5)]


def _plain(rng, shape, dt):
    a = (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    if _cplx(dt):
        a = a + 1j * (rng.random(shape) - 0.5) * np.exp2(rng.integers(-4, 5, shape))
    return a.astype(dt)


def _c0(rng, n, dt, routine):
    c = _plain(rng, (n, n), dt)
    if routine == "herk":
        c[np.arange(n), np.arange(n)] = c[np.arange(n), np.arange(n)].real
    return c


def _real_row(kind, k, rng, span, tiny):
    x = rng.random(k) - 0.5
    if kind == "zero":
        return np.zeros(k)
    if kind == "minus_zero":
        return np.full(k, -0.0)
    if kind == "third_zero":
        x[::3] = 0
    elif kind == "last_column":
        x[:k - 1] = 0
    elif kind == "subnormal":
        return rng.random(k) * tiny
    elif kind == "large":
        x *= 2.0 ** span
    elif kind == "small":
        x *= 2.0 ** -span
    elif kind == "wide":
        x *= np.exp2(rng.integers(-span, span + 1, k).astype(np.float64))
    elif kind == "pow2":
        return np.exp2(rng.integers(-20, 21, k).astype(np.float64)) * rng.choice([-1.0, 1.0], k)
    return x


def edge_operand(rows, k, dt, rng, shift=0):
    """logical rows x k matrix of op(X): row i takes pattern (i + shift) % P of the type's table"""
    cplx, single = _cplx(dt), _single(dt)
    span = 60 if single else 450
    tiny = float(np.finfo(np.float32 if single else np.float64).tiny)
    table = EDGE_CPLX if cplx else EDGE_REAL
    X = np.zeros((rows, k), np.complex128 if cplx else np.float64)
    for i in range(rows):
        kind = table[(i + shift) % len(table)]
        if not cplx:
            X[i] = _real_row(kind, k, rng, span, tiny)
        elif kind == "pure_real":
            X[i] = _real_row("plain", k, rng, span, tiny)
        elif kind == "pure_imag":
            X[i] = 1j * _real_row("plain", k, rng, span, tiny)
        elif kind == "re_subnormal_im_large":
            X[i] = _real_row("subnormal", k, rng, span, tiny) + 1j * _real_row("large", k, rng, span, tiny)
        elif kind == "re_large_im_subnormal":
            X[i] = _real_row("large", k, rng, span, tiny) + 1j * _real_row("subnormal", k, rng, span, tiny)
        else:
            X[i] = _real_row(kind, k, rng, span, tiny) + 1j * _real_row(kind, k, rng, span, tiny)
    return X.astype(dt)


def _stored(X, trans):
    return np.ascontiguousarray(X if trans == "N" else X.T)


def test_the_pattern_tables_hold_what_the_file_promises():
    """no GPU: the tables hold every pattern, and SYR2K's shift of 3 pairs the rows as the docstring says"""
    assert len(set(EDGE_REAL)) == 10 and set(EDGE_CPLX) == set(EDGE_REAL) | {"pure_real", "pure_imag", "re_subnormal_im_large", "re_large_im_subnormal"}
    zero = {"zero", "minus_zero"}
    for table in (EDGE_REAL, EDGE_CPLX):
        pairs = {(table[i], table[(i + 3) % len(table)]) for i in range(len(table))}
        assert any(a in zero and b in zero for a, b in pairs), "some rows are zero in both"
        assert any(a in zero | {"subnormal"} and b == "large" for a, b in pairs) and any(a == "large" and b in zero | {"subnormal"} for a, b in pairs)
    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64, np.complex64, np.complex128):
        X = edge_operand(len(EDGE_CPLX), 50, dt, rng)
        table = EDGE_CPLX if _cplx(dt) else EDGE_REAL
        assert np.isfinite(X).all()
        z = X[table.index("minus_zero")]
        assert not z.any() and np.signbit(z.real).all()
        s = X[table.index("subnormal")]
        tiny = np.finfo(np.float32 if _single(dt) else np.float64).tiny
        assert (np.abs(s.real) < tiny).all() and s.real.any()
        assert not X[table.index("last_column")][:-1].any() and X[table.index("last_column")][-1] != 0
        if _cplx(dt):
            assert not X[table.index("pure_real")].imag.any() and not X[table.index("pure_imag")].real.any()


# ---- 1. edge data

def _moduli(dt):
    return (7, 13) if _single(dt) else (8, 20)   # 20 takes the BIG arm of emit4_mod_float


def _edge_pair(routine, n, k, dt, rng, trans):
    A = _stored(edge_operand(n, k, dt, rng), trans)
    B = _stored(edge_operand(n, k, dt, rng, 3), trans) if routine == "syr2k" else None
    return A, B


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("routine,dt", ROUTINE_DTS, ids=RD_IDS)
def test_edge_rows_against_the_gemm_and_the_oracle(routine, dt, t, fast):
    """(70, 200): (a), (b) and (c) for both uplo x both scalar pairs x both moduli counts; and the planes the one operand pass leaves are the equivalent GEMM's
    -- C alone cannot tell SYR2K's two plane sets apart (with the K halves of both swapped, P Q^T becomes its own transpose, and C is bitwise symmetric), nor
    see a byte of HERK's conjugate twin that the GEMM's second pass would write differently unless it changes a residue"""
    rng = np.random.default_rng(4100)
    n, k, trans = 70, 200, _trans(routine, t)
    A, B = _edge_pair(routine, n, k, dt, rng, t)
    C0 = _c0(rng, n, dt, routine)
    for call, (N, (alpha, beta)) in enumerate(itertools.product(_moduli(dt), _scalars(routine, dt))):
        gu.rank_k_case(routine, A, B, C0, "LU", trans, N, fast, alpha, beta, ld_extra=(0, 0, gu.LDC_EXTRA[call % 3]), oracle=True, rng=rng, intermediates=True)


PLACEMENTS = {"contiguous": ((0, 0), (0, 0)), "a_aligned_b_off": ((4, 3), (0, 1)), "a_off_b_aligned": ((3, 4), (1, 0))}


@gpu
@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("routine,dt", ROUTINE_DTS, ids=RD_IDS)
def test_edge_rows_over_two_tile_rows_and_on_embedded_operands(routine, dt, t, fast, place):
    """(300, 257): two tile-rows and the pad edge on the k side, (a) and (c); contiguous, then A 16-byte aligned with lda = rows + 4 and B one element past
    its buffer's base with ldb = rows + 3, then the reverse (SYRK / HERK: A in either placement).  C's window starts one element in on the embedded runs."""
    rng = np.random.default_rng(4200)
    n, k, trans = 300, 257, _trans(routine, t)
    A, B = _edge_pair(routine, n, k, dt, rng, t)
    C0 = _c0(rng, n, dt, routine)
    (exa, exb), (offa, offb) = PLACEMENTS[place]
    offc = int(place != "contiguous")
    for call, (N, (alpha, beta)) in enumerate(itertools.product(_moduli(dt), _scalars(routine, dt))):
        gu.rank_k_case(routine, A, B, C0, "LU", trans, N, fast, alpha, beta, ld_extra=(exa, exb, gu.LDC_EXTRA[(call + 1) % 3]), base_off=(offa, offb, offc),
                       oracle=False, rng=rng)


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128], ids=lambda d: np.dtype(d).name)
def test_syr2k_with_a_zero_operand_and_with_a_is_b(dt, t, fast):
    """A = 0 with B plain, B = 0 with A plain, and A is B (the same pointer) on the edge operand: (a), (b), (c) at (70, 200), (a) and (c) at (300, 257)"""
    rng = np.random.default_rng(4300)
    for (n, k), oracle in (((70, 200), True), ((300, 257), False)):
        E = _stored(edge_operand(n, k, dt, rng), t)
        X = _plain(rng, E.shape, dt)
        Z = np.zeros_like(X)
        C0 = _c0(rng, n, dt, "syr2k")
        for call, (A, B) in enumerate(((Z, X), (X, Z), (E, E))):
            N = _moduli(dt)[call % 2]
            alpha, beta = _scalars("syr2k", dt)[(call + 1) % 2]
            gu.rank_k_case("syr2k", A, B, C0, "LU", t, N, fast, alpha, beta, ld_extra=(0, 0, gu.LDC_EXTRA[call % 3]), oracle=oracle, rng=rng)


# ---- 2. the schedules and the k limits under the triangular walk

def _long_k(routine, k):
    return k // 2 if routine == "syr2k" else k


def _plain_pair(routine, n, k, dt, rng, t):
    shape = (n, k) if t == "N" else (k, n)
    return _plain(rng, shape, dt), (_plain(rng, shape, dt) if routine == "syr2k" else None)


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("routine,dt", TWO_DTS, ids=TWO_IDS)
def test_ping_pong_schedule_over_five_tile_rows(routine, dt, t, fast):
    """padded inner k = 5632 (SYRK / HERK k = 5400, SYR2K k = 2700), n = 1031: five tile-rows, the walk's group of four cut; (a) and (c), both uplo"""
    rng = np.random.default_rng(4400)
    n, k = 1031, _long_k(routine, 5400)
    assert gu.pad256(gu.rank_k_inner(routine, k)) == 5632
    A, B = _plain_pair(routine, n, k, dt, rng, t)
    alpha, beta = _scalars(routine, dt)[1]
    gu.rank_k_case(routine, A, B, _c0(rng, n, dt, routine), "LU", _trans(routine, t), 3, fast, alpha, beta, ld_extra=(0, 0, 7), oracle=False, rng=rng)


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("routine,dt", TWO_DTS, ids=TWO_IDS)
def test_ping_pong_schedule_against_the_oracle(routine, dt, t, fast):
    """the same inner dimension at n = 257 (two tile-rows) with 2 moduli: (a), (b) and (c); about 0.75 s of oracle per real GEMM, 3 s per complex one"""
    rng = np.random.default_rng(4500)
    n, k = 257, _long_k(routine, 5400)
    A, B = _plain_pair(routine, n, k, dt, rng, t)
    alpha, beta = _scalars(routine, dt)[int(fast)]
    gu.rank_k_case(routine, A, B, _c0(rng, n, dt, routine), "LU", _trans(routine, t), 2, fast, alpha, beta, ld_extra=(0, 0, 64), oracle=True, rng=rng)


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("routine,dt", [x for x in TWO_DTS if x[0] != "syr2k"], ids=[i for i in TWO_IDS if not i.startswith("syr2k")])
def test_k_step_barrier_schedule_over_five_tile_rows(routine, dt, t, fast):
    """(1031, 2000): padded k = 2048, the K-step-barrier kernel beyond two tile-rows; (a) and (c).  (SYR2K has (1031, 300) in its own suite.)"""
    rng = np.random.default_rng(4600)
    n, k = 1031, 2000
    A, _ = _plain_pair(routine, n, k, dt, rng, t)
    alpha, beta = _scalars(routine, dt)[1]
    gu.rank_k_case(routine, A, None, _c0(rng, n, dt, routine), "LU", _trans(routine, t), 7, fast, alpha, beta, ld_extra=(0, 0, 1), oracle=False, rng=rng)


K_LIMIT_CASES = [(r, dt, t, fast) for r in gu.RANK_K
                 for dt, t, fast in ((np.float64, "N", False), (np.complex64, "T", True), (np.float64, "T", True), (np.complex64, "N", False))
                 if r != "herk" or dt is np.complex64]


@gpu
@pytest.mark.parametrize("routine,dt,t,fast", K_LIMIT_CASES, ids=[f"{r}-{np.dtype(d).name}-{t}-{'fast' if f else 'accu'}" for r, d, t, f in K_LIMIT_CASES])
def test_k_at_the_limit(routine, dt, t, fast):
    """n = 37 and k = 2^17 (SYRK, HERK) / 2^16 (SYR2K), 2 moduli: (a), (b) and (c); about 37^2 2^17 2 / 1e9 = 0.36 s of oracle, four times that complex"""
    rng = np.random.default_rng(4700)
    n, k = 37, 1 << (16 if routine == "syr2k" else 17)
    A, B = _plain_pair(routine, n, k, dt, rng, t)
    alpha, beta = _scalars(routine, dt)[1]
    gu.rank_k_case(routine, A, B, _c0(rng, n, dt, routine), "LU", _trans(routine, t), 2, fast, alpha, beta, ld_extra=(0, 0, 7), oracle=True, rng=rng)


# ---- 3. forced paths: each compared with the same call with the knob unset, and with (a)

def _same_triangle(x, y, what):
    for uplo in x["out"]:
        tri = x["tri"][uplo]
        assert np.array_equal(x["out"][uplo][tri], y["out"][uplo][tri]), f"{what}: the triangle {uplo} differs from the run with the knob unset"


@gpu
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("routine,dt", TWO_DTS, ids=TWO_IDS)
def test_scale_fold_off_gives_the_folded_forms_bytes(routine, dt, t, monkeypatch):
    """GEMMUL8_SCALE_FOLD=0, accurate mode, (300, 257): SYR2K's own branch of syr2k_scale (one finalize launch that writes sftA), and the GEMM's un-folded
    form for SYRK / HERK.  Triangle and sftA (read in the rank-k call's own layout: SYR2K's inner dimension is 2 pad256(k)) are the folded form's."""
    rng = np.random.default_rng(4800)
    n, k, N = 300, 257, 7
    A, B = _plain_pair(routine, n, k, dt, rng, t)
    C0 = _c0(rng, n, dt, routine)
    alpha, beta = _scalars(routine, dt)[1]
    runs = []
    for knob in (None, 0):
        gu.setknob(monkeypatch, "GEMMUL8_SCALE_FOLD", knob)
        runs.append(gu.rank_k_case(routine, A, B, C0, "LU", _trans(routine, t), N, False, alpha, beta, ld_extra=(0, 0, 7), oracle=False, rng=rng, intermediates=True))
    _same_triangle(runs[1], runs[0], "GEMMUL8_SCALE_FOLD=0")
    for uplo in "LU":
        assert runs[0]["it"][uplo]["sftA"].any()
        assert np.array_equal(runs[1]["it"][uplo]["sftA"], runs[0]["it"][uplo]["sftA"]), "sftA differs between the folded and the un-folded finalize"
        assert np.array_equal(runs[1]["it"][uplo]["A_lo"], runs[0]["it"][uplo]["A_lo"])


@gpu
@pytest.mark.parametrize("fast", [False, True], ids=["accu", "fast"])
@pytest.mark.parametrize("dt", [np.complex64, np.complex128], ids=["complex64", "complex128"])
@pytest.mark.parametrize("routine", gu.RANK_K)
def test_chunked_moduli_loop(routine, dt, fast, monkeypatch):
    """GEMMUL8_CPLX_CHUNK=1 and =3 with 7 moduli, (300, 257): the chunked loop of rank_k offsets every plane pointer -- the twin's by
    t0 * twin.plane_stride -- by chunks of 1 and of 3 (the last one cut to 1)"""
    rng = np.random.default_rng(4900)
    n, k, N = 300, 257, 7
    for t in "NT":
        A, B = _plain_pair(routine, n, k, dt, rng, t)
        C0 = _c0(rng, n, dt, routine)
        alpha, beta = _scalars(routine, dt)[1]
        runs = []
        for knob in (None, 1, 3):
            gu.setknob(monkeypatch, "GEMMUL8_CPLX_CHUNK", knob)
            runs.append(gu.rank_k_case(routine, A, B, C0, "LU", _trans(routine, t), N, fast, alpha, beta, ld_extra=(0, 0, 64), oracle=False, rng=rng))
        _same_triangle(runs[1], runs[0], "GEMMUL8_CPLX_CHUNK=1")
        _same_triangle(runs[2], runs[0], "GEMMUL8_CPLX_CHUNK=3")


@gpu
@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("dt", [np.complex64, np.complex128], ids=["complex64", "complex128"])
def test_chunked_moduli_loop_of_the_complex_gemm(dt, chunk, monkeypatch):
    """no test set GEMMUL8_CPLX_CHUNK for gemmul8_gemm either: full parity against the oracle, both modes"""
    gu.setknob(monkeypatch, "GEMMUL8_CPLX_CHUNK", chunk)
    rng = np.random.default_rng(5000)
    A, B = _plain(rng, (70, 200), dt), _plain(rng, (200, 45), dt)
    for fast in (False, True):
        gu.parity_case(A, B, 7, fast, alpha=0.75 - 0.25j, beta=-0.5 + 1.5j, C0=_plain(rng, (70, 45), dt))


@gpu
@pytest.mark.parametrize("t", ["N", "T"])
@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["float64", "complex128"])
@pytest.mark.parametrize("routine", gu.RANK_K)
def test_bound_tile_sizes(routine, dt, t, monkeypatch):
    """GEMMUL8_BOUND_TILE=128 and =256, accurate mode, (513, 300): the bound GEMM of a rank-k call stays the full square, in either tile size"""
    if routine == "herk" and dt is np.float64:
        dt = np.complex64   # HERK has no real type: its second type instead
    rng = np.random.default_rng(5100)
    n, k, N = 513, 300, 8
    A, B = _plain_pair(routine, n, k, dt, rng, t)
    C0 = _c0(rng, n, dt, routine)
    alpha, beta = _scalars(routine, dt)[1]
    runs = []
    for knob in (None, 128, 256):
        gu.setknob(monkeypatch, "GEMMUL8_BOUND_TILE", knob)
        runs.append(gu.rank_k_case(routine, A, B, C0, "LU", _trans(routine, t), N, False, alpha, beta, ld_extra=(0, 0, 1), oracle=False, rng=rng, intermediates=True))
    for i, knob in ((1, 128), (2, 256)):
        _same_triangle(runs[i], runs[0], f"GEMMUL8_BOUND_TILE={knob}")
        assert np.array_equal(runs[i]["it"]["L"]["sftA"], runs[0]["it"]["L"]["sftA"])


ONE_READ = "GEMMUL8_BOUNDS_ONE_READ"


@gpu
@pytest.mark.parametrize("place", ["aligned", "offset"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
def test_syrk_one_read_bound_extract_equals_the_two_pass_form(dt, place, monkeypatch):
    """SYRK, trans = N, real types: the only rank-k caller the one-read extract exists for (skipB: no row-maxima launch at all).  A from the one-read suite's
    operand() -- rising and falling tile maxima, zero tiles and rows, subnormal rows, a late maximum, rows spanning the whole exponent range (their products
    overflow: whatever comes out, it is the GEMM's bits) -- at n in (33, 257) and 80 (full panels of both types), k in (129, 1000); 16-byte aligned base with lda = n + 4 (80: the
    pipelined walk), and one element past the base with lda = n + 3.  =1 against =0: triangle, sftA and the A planes byte-identical; and (a)."""
    rng = np.random.default_rng(5200)
    exa, offa = (4, 0) if place == "aligned" else (3, 1)
    case = 0
    for n, k in itertools.product((33, 80, 257), (129, 1000)):
        case += 1
        A = operand(n, k, dt, rng, case)
        C0 = _c0(rng, n, dt, "syrk")
        runs = []
        for knob in (0, 1):
            gu.setknob(monkeypatch, ONE_READ, knob)
            runs.append(gu.rank_k_case("syrk", A, None, C0, "LU", "N", 8, False, 0.75, -0.5, ld_extra=(exa, 0, gu.LDC_EXTRA[case % 3]), base_off=(offa, 0, 0),
                                       oracle=False, rng=np.random.default_rng(case), intermediates=True))
        _same_triangle(runs[1], runs[0], f"{ONE_READ}=1 n={n} k={k}")
        for key in ("sftA", "A_lo"):
            assert np.array_equal(runs[1]["it"]["L"][key], runs[0]["it"]["L"][key]), f"{key} differs between the one-read and the two-pass form, n={n} k={k}"


@gpu
@pytest.mark.parametrize("routine,dt,t", [("syrk", np.float64, "T"), ("herk", np.complex128, "N"), ("syr2k", np.float64, "N")], ids=["syrk-T", "herk-N", "syr2k-N"])
def test_one_read_knob_changes_nothing_where_the_form_does_not_exist(routine, dt, t, monkeypatch):
    rng = np.random.default_rng(5300)
    n, k = 257, 1000
    A, B = _plain_pair(routine, n, k, dt, rng, t)
    C0 = _c0(rng, n, dt, routine)
    runs = []
    for knob in (0, 1):
        gu.setknob(monkeypatch, ONE_READ, knob)
        runs.append(gu.rank_k_case(routine, A, B, C0, "L", _trans(routine, t), 8, False, 0.75, -0.5, ld_extra=(4, 4, 7), oracle=False, rng=np.random.default_rng(3),
                                   intermediates=True))
    _same_triangle(runs[1], runs[0], f"{ONE_READ}=1")
    for key in ("sftA", "A_lo", "B_lo"):
        assert np.array_equal(runs[1]["it"]["L"][key], runs[0]["it"]["L"][key]), key


@gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
def test_default_rule_takes_the_one_read_extract_at_8192_rows(dt, monkeypatch):
    """SYRK trans = N, n = 8192, k = 200, 2 moduli, accurate mode, A contiguous and aligned, the knob UNSET: the default rule selects the one-read extract,
    and with skipB there is no row-maxima launch.  Against the knob = 0, on the device: the triangle byte-identical, nothing outside it written."""
    rng = np.random.default_rng(5400)
    n, k, N = 8192, 200, 2
    R = rng.uniform(-1.0, 1.0, (n, k))
    R[:64] = operand(64, k, dt, rng, 0)
    R[-64:] = operand(64, k, dt, rng, 5)
    dA = gu.to_dev(R.astype(dt))
    tdt = gu.NP2T[np.dtype(dt)]
    w = np.dtype(dt).itemsize // 4
    ldc = n + 1
    sent = int(np.array([gu.SENTINEL] * 4, np.uint8).view(np.int32)[0])
    tri = torch.ones((n, n), dtype=torch.bool, device="cuda").triu()   # [col][row]: the lower triangle
    work = torch.empty(gu.rank_k_work_size("syrk", False, n, k, N), dtype=torch.uint8, device="cuda")
    res = []
    for knob in (None, 0):
        gu.setknob(monkeypatch, ONE_READ, knob)
        buf = torch.full((n, ldc * w), sent, dtype=torch.int32, device="cuda")
        gu.rank_k_call("syrk", dt, n, k, "L", "N", N, False, 1.0, 0.0, dA, n, buf, ldc, work=work)   # beta == 0: C is not read
        torch.cuda.synchronize()
        res.append(buf)
    a, b = (x.view(tdt).view(torch.int32 if w == 1 else torch.int64) for x in res)
    assert a.shape == (n, ldc)
    outside = torch.ones((n, ldc), dtype=torch.bool, device="cuda")
    outside[:, :n] = ~tri
    sentv = int(np.array([gu.SENTINEL] * (4 * w), np.uint8).view(np.int32 if w == 1 else np.int64)[0])
    assert bool((a[outside] == sentv).all()) and bool((b[outside] == sentv).all()), "bytes outside the stored triangle were written"
    assert not bool((a[:, :n][tri] == sentv).any()), "an entry of the triangle was not written"
    assert bool((a[:, :n][tri] == b[:, :n][tri]).all()), "the default rule's triangle differs from the two-pass form's"
