"""gemmul8_trmm on the GPU (include/gemmul8_c.h): the m x n window of C carries the bits of the equivalent GEMM -- gemmul8_gemm, whose code path this
feature does not touch, on the materialised M = op(Atri) (side L) or its plain transpose Mt (side R), run in the same process -- whatever the other strict
triangle of A, its lda padding and, under UNIT, its diagonal hold; the enclosing buffers of A, B and C keep every other byte; C == B works in place; the CPU
oracle; HIP-graph replay.

(a) and (b) run over the whole grid, one test per (type, shape): 2 sides x 2 uplo x {N, T, C} x 2 diag x 2 modes, with alpha rotating over SYMM's scalar
sets (device-resident every other time a general alpha comes up), the type's moduli counts, the ld padding 1 / 7 / 64 and the element offsets 0 / 1.  Every
point runs twice: with a finite A into a separate, NaN-filled C (C is never read), and with every unused part of A poisoned with NaN IN PLACE (C == B).
Both must give the GEMM's bits, so in place equals out of place.

Shapes (ka, other dimension), the smallest at which each mechanism can fail: (1, 1); (37, 5): one partial tile, all of it diagonal; (128, 64): one K-step
holds data; (129, 33): a second K-step one column wide; (256, 256): no padding; (257, 40): two tile-rows with K ranges of 2 and 3 (of 4) K-steps; (600, 300):
3 x 2 tiles, ranges 2 / 4 / 5 of 6; (1100, 600) with 20 moduli: 300 tiles on 256 workgroups -- a workgroup crosses from a tile into one with another range,
the look-ahead fetch across the boundary; (5200, 64): kp = 5376, the ping-pong schedule, 21 tile-rows x 14 (13) moduli = more tiles than workgroups.
ka <= 512 is the SMALLK kernel.  The last two run on a reduced grid: both sides, both triangles, N and C, float64 and one complex type, diag and mode
rotating."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol
import trmm_util as tu
from symm_util import is_cplx
from test_gpu_symm import CSCALARS, LD_EXTRA, SCALARS, TORCH_DT, Embedded, _dims, _moduli, _rand, _words

pytestmark = pytest.mark.gpu

TYPES = [np.float32, np.float64, np.complex64, np.complex128]
SHAPES = [(1, 1), (37, 5), (128, 64), (129, 33), (256, 256), (257, 40), (600, 300)]
ALPHAS = [a for a, _ in SCALARS]
CALPHAS = [a for a, _ in CSCALARS]


def _rand_dev(shape, dt, seed):
    """a (cols, rows) device tensor of a rows x cols column-major matrix: uniform mantissas, exponents over 2^-4 .. 2^4, as test_gpu_symm._rand"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    tdt = TORCH_DT[np.dtype(dt)]
    rdt = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(tdt, tdt)

    def part():
        return ((torch.rand(shape[::-1], generator=gen, device="cuda", dtype=torch.float64) - 0.5)
                * torch.exp2(torch.randint(-4, 5, shape[::-1], generator=gen, device="cuda").double())).to(rdt)
    return torch.complex(part(), part()) if tdt.is_complex else part()


def _stored_tri(At, uplo, strict=False):
    """mask, in the (cols, rows) layout, of the triangle `uplo` of the matrix"""
    ones = torch.ones(At.shape, dtype=torch.bool, device=At.device)
    d = 1 if strict else 0
    return torch.triu(ones, d) if uplo == "L" else torch.tril(ones, -d)   # (the layout is the transpose)


def _materialise_dev(At, uplo, trans, diag, side):
    """device tensor, (cols, rows) layout, of the equivalent GEMM's triangular operand: M (side L) or Mt (side R)"""
    T = torch.where(_stored_tri(At, uplo), At, torch.zeros_like(At))
    if diag == "U":
        T.diagonal().fill_(1)
    # T holds Atri in the (cols, rows) layout, i.e. it is Atri^T as a tensor; M = op(Atri)
    M = {"N": T, "T": T.T, "C": T.T.conj()}[trans]
    return (M if side == "L" else M.T).resolve_conj().contiguous()


def _poison_dev(At, uplo, diag):
    P = At.clone()
    nan = complex(float("nan"), float("nan")) if At.is_complex() else float("nan")
    P[~_stored_tri(At, uplo)] = nan
    if diag == "U":
        P.diagonal().fill_(nan)
    return P


def _trmm_call(dt, side, uplo, trans, diag, m, n, alpha, A, B, Cm, N, fast, work, alpha_dev=False):
    al = np.array([alpha], dtype=dt)
    keep = torch.from_numpy(al).cuda() if alpha_dev else None
    pa = keep.data_ptr() if alpha_dev else al.ctypes.data
    rc = g.lib().gemmul8_trmm(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.SIDE[side], g.UPLO[uplo], g.OPS[trans], g.DIAG[diag],
                              m, n, pa, A.ptr(), A.ld, B.ptr(), B.ld, Cm.ptr(), Cm.ld, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_trmm")
    torch.cuda.synchronize()


def _gemm_ref(Mop_d, B_d, side, N, fast, alpha, work):
    left, right, opB = (Mop_d, B_d, "N") if side == "L" else (B_d, Mop_d, "T")
    return g.gemm(left, right, N, fastmode=fast, opA="N", opB=opB, alpha=alpha, beta=0.0, work=work)[0]


def _run_grid(dt, ka, other, points, moduli):
    cplx = is_cplx(dt)
    A_d = _rand_dev((ka, ka), dt, ka * 131 + other)
    B_d = {s: _rand_dev(_dims(ka, other, s), dt, ka * 137 + other + i) for i, s in enumerate("LR")}
    nanC_d = {s: torch.full_like(B_d[s], complex(float("nan"), float("nan")) if cplx else float("nan")) for s in "LR"}
    work = torch.empty(max(g.trmm_work_size(cplx, *_dims(ka, other, s), s, max(moduli)) for s in "LR"), dtype=torch.uint8, device="cuda")
    alphas = CALPHAS if cplx else ALPHAS
    for call, (side, uplo, trans, diag, fast) in enumerate(points):
        m, n = _dims(ka, other, side)
        N = moduli[call % len(moduli)]
        sc = (call // 2 + call // 7) % 4
        alpha = alphas[sc]
        alpha_dev = sc >= 2 and bool((call // 4) & 1)
        ref = _words(_gemm_ref(_materialise_dev(A_d, uplo, trans, diag, side), B_d[side], side, N, fast, alpha, work))
        for poisoned in (False, True):
            ex, off = [LD_EXTRA[(call + j + poisoned) % 3] for j in range(3)], [((call + poisoned) >> j) & 1 for j in range(3)]
            EA = Embedded(_poison_dev(A_d, uplo, diag), ex[0], off[0], fill=0xFF) if poisoned else Embedded(A_d, ex[0], off[0])
            EB = Embedded(B_d[side], ex[1], off[1])
            EC = EB if poisoned else Embedded(nanC_d[side], ex[2], off[2])   # poisoned: in place, C == B with ldc == ldb
            _trmm_call(dt, side, uplo, trans, diag, m, n, alpha, EA, EB, EC, N, fast, work, alpha_dev)
            what = f"N={N} side={side} uplo={uplo} trans={trans} diag={diag} fast={fast} alpha={alpha} dev={alpha_dev} poisoned/in-place={poisoned} ld+{ex} off={off}"
            assert torch.equal(EA.bytes, EA.before), "A was written: " + what
            if not poisoned:
                assert torch.equal(EB.bytes, EB.before), "B was written: " + what
            assert not bool(((EC.bytes != EC.before) & ~EC.inside).any()), "bytes outside the m x n window of C were written: " + what
            bad = EC.window_words() != ref
            assert not bool(bad.any()), f"{int(bad.sum())} words of C differ from gemmul8_gemm on the materialised matrix: " + what


FULL_GRID = list(itertools.product("LR", "LU", "NTC", "NU", (False, True)))


@pytest.mark.parametrize("ka,other", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
@pytest.mark.parametrize("dt", TYPES, ids=[np.dtype(d).name for d in TYPES])
def test_whole_grid_window_is_the_gemms_and_nothing_else_is_touched(dt, ka, other):
    """(a), (b) for every side x uplo x trans x diag x mode of this type and shape"""
    _run_grid(dt, ka, other, FULL_GRID, _moduli(dt))


def _reduced_grid():
    pts = list(itertools.product("LR", "LU", "NC"))
    return [(s, u, t, "NU"[(i + i // 2) % 2], bool((i + i // 4) % 2)) for i, (s, u, t) in enumerate(pts)]


def test_the_reduced_grid_keeps_sides_triangles_ops_and_rotates_diag_and_mode():
    pts = _reduced_grid()
    assert {p[:3] for p in pts} == set(itertools.product("LR", "LU", "NC")) and len(pts) == 8
    assert {p[3] for p in pts} == {"N", "U"} and {p[4] for p in pts} == {False, True}
    for s in "LR":   # both K-range cases of each side (M lower / upper), each in both modes or both diag values
        assert {tu.m_is_lower(p[1], p[2]) for p in pts if p[0] == s} == {True, False}


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["float64", "complex128"])
def test_more_tiles_than_workgroups_crossing_between_tiles_of_different_k_ranges(dt):
    """(1100, 600) with 20 moduli: 5 x 3 x 20 = 300 tiles on at most 256 workgroups (side R: 3 x 5 x 20)"""
    _run_grid(dt, 1100, 600, _reduced_grid(), [20])


@pytest.mark.parametrize("dt,N", [(np.float64, 14), (np.complex64, 13)], ids=["float64-14", "complex64-13"])
def test_ping_pong_schedule_with_k_ranges(dt, N):
    """(5200, 64): kp = 5376 > the K-step-barrier schedule's limit; 21 tile-rows (side R: tile-columns) x N planes > 256 workgroups"""
    _run_grid(dt, 5200, 64, _reduced_grid(), [N])


def test_device_materialisation_matches_the_numpy_definition():
    rng = np.random.default_rng(3)
    for dt in (np.float64, np.complex64):
        A = _rand(rng, (37, 37), dt)
        for side, uplo, trans, diag in itertools.product("LR", "LU", "NTC", "NU"):
            left, right, _, _ = tu.equivalent_gemm(A, np.zeros((37, 37), dt), side, uplo, trans, diag)
            want = left if side == "L" else right
            got = gu.from_dev(_materialise_dev(gu.to_dev(A), uplo, trans, diag, side))
            assert np.array_equal(got, want), (side, uplo, trans, diag)
        P = gu.from_dev(_poison_dev(gu.to_dev(A), "L", "U"))
        assert np.array_equal(np.isnan(P), np.isnan(tu.poison(A, "L", "U")))


# ---- (c) the CPU oracle, on a rotating subset: every type at every shape of the full grid; the oracle costs about m n ka N (x 4 complex) / 1e9 s per GEMM
def _oracle_seconds(dt, ka, other, N):
    return ka * ka * other * N * (4 if is_cplx(dt) else 1) / 1e9


def _oracle_cases():
    out = []
    for si, (ka, other) in enumerate(SHAPES):
        for ti, dt in enumerate(TYPES):
            mods = _moduli(dt)
            N = mods[(si + ti) % len(mods)]
            while _oracle_seconds(dt, ka, other, N) > 3 and N > 2:
                N = mods[mods.index(N) - 1]
            i = si + ti
            out.append((ti, ka, other, "LR"[i % 2], "LU"[(si // 4 + i) % 2], "NTC"[(si + 2 * ti) % 3], "NU"[(si // 2 + ti) % 2], bool((si // 2 + i) % 2), i % 4, N,
                        (LD_EXTRA[i % 3], (si // 2 + ti) % 2)))
    return out


ORACLE_CASES = _oracle_cases()


def test_the_oracle_subset_covers_every_type_at_every_shape_and_every_enum_value():
    for ti in range(len(TYPES)):
        mine = [c for c in ORACLE_CASES if c[0] == ti]
        assert {(c[1], c[2]) for c in mine} == set(SHAPES)
        assert {c[3] for c in mine} == {"L", "R"} and {c[4] for c in mine} == {"L", "U"} and {c[5] for c in mine} == {"N", "T", "C"}
        assert {c[6] for c in mine} == {"N", "U"} and {c[7] for c in mine} == {False, True}
    for c in ORACLE_CASES:
        assert _oracle_seconds(TYPES[c[0]], c[1], c[2], c[9]) <= 3, c


@pytest.mark.parametrize("ti,ka,other,side,uplo,trans,diag,fast,sc,N,emb", ORACLE_CASES,
                         ids=[f"{np.dtype(TYPES[c[0]]).name}-{c[1]}x{c[2]}-{c[3]}{c[4]}{c[5]}{c[6]}-{'fast' if c[7] else 'accu'}-s{c[8]}-N{c[9]}" for c in ORACLE_CASES])
def test_window_bits_equal_the_oracles_gemm(ti, ka, other, side, uplo, trans, diag, fast, sc, N, emb):
    """against the CPU oracle's equivalent GEMM run with the device's shifts, as gpu_util.parity_case does; A's unused parts are NaN"""
    dt = TYPES[ti]
    rng = np.random.default_rng(ka * 131 + other + ti)
    cplx = is_cplx(dt)
    alpha = (CALPHAS if cplx else ALPHAS)[sc]
    m, n = _dims(ka, other, side)
    A, B = _rand(rng, (ka, ka), dt), _rand(rng, (m, n), dt)
    left, right, opA, opB = tu.equivalent_gemm(A, B, side, uplo, trans, diag)
    C0 = np.zeros((m, n), dt)
    Cg, it = gu.hip_gemm(left, right, N, fastmode=fast, opA=opA, opB=opB, alpha=alpha, beta=0.0, C0=C0, want_intermediates=True)
    Co = ol.gemm(left, right, N, fastmode=fast, opA=opA, opB=opB, alpha=alpha, beta=0.0, C0=C0, sftA_in=it["sftA"], sftB_in=it["sftB"])
    EA, EB, EC = Embedded(tu.poison(A, uplo, diag), emb[0], emb[1], fill=0xFF), Embedded(B, emb[0], 1 - emb[1]), Embedded(np.full((m, n), np.nan, dt), emb[0], emb[1])
    work = torch.full((g.trmm_work_size(cplx, m, n, side, N),), 0x3C, dtype=torch.uint8, device="cuda")
    _trmm_call(dt, side, uplo, trans, diag, m, n, alpha, EA, EB, EC, N, fast, work)
    got = gu.from_dev(EC.view.contiguous())
    assert gu.bits_equal(got, np.ascontiguousarray(Cg)), "differs from gemmul8_gemm on the materialised matrix"
    assert gu.bits_equal(got, np.ascontiguousarray(np.asarray(Co))), "differs from the oracle's GEMM"
    assert not bool(((EC.bytes != EC.before) & ~EC.inside).any())


@pytest.mark.parametrize("dt,side,uplo,trans,diag", [(np.float64, "L", "L", "N", "N"), (np.complex64, "R", "U", "C", "U")], ids=["float64-LLNN", "complex64-RUCU"])
def test_graph_capture_replays_to_the_same_bits(dt, side, uplo, trans, diag):
    """(d): a single-stream call with timers_ns == NULL, captured once and replayed; alpha on the device in the complex case"""
    ka, other, N = 300, 129, 7
    m, n = _dims(ka, other, side)
    dA, dB = _rand_dev((ka, ka), dt, 7), _rand_dev((m, n), dt, 8)
    alpha = torch.tensor([0.75 - 0.25j], dtype=TORCH_DT[np.dtype(dt)], device="cuda") if is_cplx(dt) else -1
    kw = dict(side=side, uplo=uplo, trans=trans, diag=diag, alpha=alpha)
    for fast in (False, True):
        eager, _, work = g.trmm(dA, dB, N, fastmode=fast, **kw)
        torch.cuda.synchronize()
        ref = _gemm_ref(_materialise_dev(dA, uplo, trans, diag, side), dB, side, N, fast, 0.75 - 0.25j if is_cplx(dt) else -1, None)
        assert torch.equal(_words(eager), _words(ref))
        out = torch.zeros_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.trmm(dA, dB, N, fastmode=fast, C_out=out, work=work, **kw)   # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        out.zero_()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            g.trmm(dA, dB, N, fastmode=fast, C_out=out, work=work, **kw)
        for _ in range(2):
            out.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert gu.bits_equal(out.cpu().numpy(), eager.cpu().numpy())


def test_python_wrapper_in_place_views_and_timers():
    """g.trmm: defaults, C_out = B (in place), a view of A with a larger leading dimension, timers"""
    ka, other, N = 129, 33, 7
    for dt, side in zip(TYPES, "LRLR"):
        m, n = _dims(ka, other, side)
        dA, dB = _rand_dev((ka, ka), dt, 9), _rand_dev((m, n), dt, 10)
        EA = Embedded(_poison_dev(dA, "U", "N"), 7, 1, fill=0xFF)
        ref = _gemm_ref(_materialise_dev(dA, "U", "T", "N", side), dB, side, N, False, 1.0, None)
        Cd, tm, _ = g.trmm(EA.view, dB, N, side=side, uplo="U", trans="T", timers=True)
        torch.cuda.synchronize()
        assert len(tm) == 4 and tm[0] > 0 and tm[1] > 0 and tm[3] > 0
        assert torch.equal(_words(Cd), _words(ref))
        Bc = dB.clone()
        Cd2, _, _ = g.trmm(EA.view, Bc, N, side=side, uplo="U", trans="T", C_out=Bc)
        torch.cuda.synchronize()
        assert Cd2 is Bc and torch.equal(_words(Bc), _words(ref))
