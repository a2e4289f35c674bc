"""gemmul8_trsm on the GPU (include/gemmul8_c.h): the m x n window of B carries, bit for bit, what the recipe gives -- the model of tests/trsm_util.py run
in the same process, with g.gemm (a code path this feature does not touch) as its GEMM and the torch form of the leaf -- whatever the other strict triangle
of A, its lda padding and, under UNIT, its diagonal hold; the enclosing buffers of A and B keep every other byte.

The grid, one test per (type, shape): 2 sides x 2 uplo x {N, T, C} x 2 diag x 2 modes, with alpha rotating over SYMM's scalar sets (device-resident every
other time a general alpha comes up), the type's moduli counts, the ld padding 1 / 7 / 64 and the element offsets 0 / 1.  Every point runs with a finite A and
again with every unused part of A poisoned with NaN; both must give the model's bits.

Shapes (ka, other dimension) with L = gemmul8_trsm_leaf(), the smallest at which each mechanism can fail: (1, 1); (L-1, 5): one partial leaf; (L, 64): a
full leaf, no GEMM; (L+1, 33): h = L, remainder 1, a one-row GEMM; (2L+1, 40): h = 2L, two levels, the pending scale handed down and then dropped;
(600, 300): a ragged last block; (1100, 70): k = 1024 GEMMs on the long-K kernel beside k = L ones.  The last two run on a reduced grid: both sides, both
triangles, N and C, float64 and one complex type, diag and mode rotating.  The data are well conditioned (off-diagonal entries uniform in +-1/ka, diagonal
magnitudes in [1, 2]), so that no entry overflows."""
import itertools

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol
import trsm_util as su
from symm_util import is_cplx
from test_gpu_symm import LD_EXTRA, TORCH_DT, Embedded, _dims, _moduli, _words
from test_gpu_trmm import ALPHAS, CALPHAS, FULL_GRID, TYPES, _poison_dev, _reduced_grid

pytestmark = pytest.mark.gpu

L = g.TRSM_LEAF
SHAPES = [(1, 1), (L - 1, 5), (L, 64), (L + 1, 33), (2 * L + 1, 40)]


def _data(dt, ka, other, seed):
    rng = np.random.default_rng(seed)
    A_d = gu.to_dev(su.well_conditioned(rng, ka, dt))
    B_d = {s: gu.to_dev(su.rhs(rng, _dims(ka, other, s), dt)) for s in "LR"}
    return A_d, B_d


def _dev_gemm(N, fast, scalars_dev=False):
    """the model's GEMM: gemmul8_gemm on contiguous copies of the blocks (its bits do not depend on the leading dimensions: tests/test_gpu_ld.py) -- through
    g.gemm, or with scalars_dev through the C ABI with -1 and beta resident on the device, as the routine calls it beside a device-resident alpha (a zero
    beta is then tested on the device, and the signs of zeros it leaves differ from the host path's)"""
    def gemm(lhs, rhs, opL, opR, beta, Cm):
        out, dl, dr = Cm.T.contiguous(), lhs.T.contiguous(), rhs.T.contiguous()
        if not scalars_dev:
            g.gemm(dl, dr, N, fastmode=fast, opA=opL, opB=opR, alpha=-1.0, beta=beta, C_out=out)
            return out.T
        n, m = out.shape
        k = lhs.shape[1] if opL == "N" else lhs.shape[0]
        sc = torch.tensor([-1, beta], dtype=out.dtype, device="cuda")
        work = torch.empty(g.work_size(out.dtype.is_complex, g.INT8, m, n, k, N)[0], dtype=torch.uint8, device="cuda")
        rc = g.lib().gemmul8_gemm(torch.cuda.current_stream().cuda_stream, g._dtype_code(out.dtype), g.INT8, g.OPS[opL], g.OPS[opR], m, n, k, sc.data_ptr(),
                                  dl.data_ptr(), dl.shape[1], dr.data_ptr(), dr.shape[1], sc.data_ptr() + sc.element_size(), out.data_ptr(), out.shape[1], N,
                                  int(fast), work.data_ptr(), None, None, 0, 0, 0, 0, None)
        g.check(rc, "gemmul8_gemm")
        torch.cuda.synchronize()
        return out.T
    return gemm


def _model(A_d, B_d, alpha, side, uplo, trans, diag, N, fast, scalars_dev=False):
    """the recipe on device tensors of the (cols, rows) layout; returns the (cols, rows) tensor of X"""
    return su.solve(A_d.T, B_d.T, alpha, side, uplo, trans, diag, L, _dev_gemm(N, fast, scalars_dev)).T.contiguous()


def _trsm_call(dt, side, uplo, trans, diag, m, n, alpha, A, B, N, fast, work, alpha_dev=False, stream=None):
    al = np.array([alpha], dtype=dt)
    keep = torch.from_numpy(al).cuda() if alpha_dev else None
    pa = keep.data_ptr() if alpha_dev else al.ctypes.data
    rc = g.lib().gemmul8_trsm(torch.cuda.current_stream().cuda_stream, ol.DT[np.dtype(dt)], g.INT8, g.SIDE[side], g.UPLO[uplo], g.OPS[trans], g.DIAG[diag],
                              m, n, pa, A.ptr(), A.ld, B.ptr(), B.ld, N, int(fast), work.data_ptr(), None)
    g.check(rc, "gemmul8_trsm")
    torch.cuda.synchronize()


def _run_grid(dt, ka, other, points, moduli):
    cplx = is_cplx(dt)
    A_d, B_d = _data(dt, ka, other, ka * 131 + other)
    work = torch.empty(max(g.trsm_work_size(cplx, *_dims(ka, other, s), s, max(moduli)) for s in "LR"), dtype=torch.uint8, device="cuda")
    alphas = CALPHAS if cplx else ALPHAS
    for call, (side, uplo, trans, diag, fast) in enumerate(points):
        m, n = _dims(ka, other, side)
        N = moduli[call % len(moduli)]
        sc = (call // 2 + call // 7) % 4
        alpha = alphas[sc]
        alpha_dev = sc >= 2 and bool((call // 4) & 1)
        if alpha == 0 and not alpha_dev:   # a host zero: +0 over the window, A unread (its own test below); a device zero takes the recipe
            ref = _words(torch.zeros_like(B_d[side]))
        else:
            ref = _words(_model(A_d, B_d[side], alpha, side, uplo, trans, diag, N, fast, alpha_dev))
        for poisoned in (False, True):
            ex, off = [LD_EXTRA[(call + j + poisoned) % 3] for j in range(2)], [((call + poisoned) >> j) & 1 for j in range(2)]
            EA = Embedded(_poison_dev(A_d, uplo, diag), ex[0], off[0], fill=0xFF) if poisoned else Embedded(A_d, ex[0], off[0])
            EB = Embedded(B_d[side], ex[1], off[1])
            _trsm_call(dt, side, uplo, trans, diag, m, n, alpha, EA, EB, N, fast, work, alpha_dev)
            what = f"N={N} side={side} uplo={uplo} trans={trans} diag={diag} fast={fast} alpha={alpha} dev={alpha_dev} poisoned={poisoned} ld+{ex} off={off}"
            assert torch.equal(EA.bytes, EA.before), "A was written: " + what
            assert not bool(((EB.bytes != EB.before) & ~EB.inside).any()), "bytes outside the m x n window of B were written: " + what
            bad = EB.window_words() != ref
            assert not bool(bad.any()), f"{int(bad.sum())} words of X differ from the recipe's model: " + what


@pytest.mark.parametrize("ka,other", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
@pytest.mark.parametrize("dt", TYPES, ids=[np.dtype(d).name for d in TYPES])
def test_whole_grid_window_is_the_recipes_and_nothing_else_is_touched(dt, ka, other):
    _run_grid(dt, ka, other, FULL_GRID, _moduli(dt))


def test_the_reduced_grid_covers_sides_triangles_ops_and_rotates_diag_and_mode():
    pts = _reduced_grid()
    assert {p[:3] for p in pts} == set(itertools.product("LR", "LU", "NC")) and len(pts) == 8
    assert {p[3] for p in pts} == {"N", "U"} and {p[4] for p in pts} == {False, True}
    for s in "LR":   # both directions of the substitution on each side
        assert {su.m_is_lower(p[1], p[2]) for p in pts if p[0] == s} == {True, False}
    # and the two shapes do what they are there for: a ragged last block; k = 1024 GEMMs beside k = L ones
    assert 600 % L != 0 and su.plan(600, L, "L", True)[-1][2] == 600 % L
    ks = {st[2] for st in su.plan(1100, L, "L", True) if st[0] == "gemm"}
    assert 1024 in ks and L in ks


@pytest.mark.parametrize("dt,ka,other,N", [(np.float64, 600, 300, 14), (np.complex128, 600, 300, 7), (np.float64, 1100, 70, 20), (np.complex64, 1100, 70, 13)],
                         ids=["float64-600x300", "complex128-600x300", "float64-1100x70", "complex64-1100x70"])
def test_ragged_last_block_and_long_k_updates(dt, ka, other, N):
    _run_grid(dt, ka, other, _reduced_grid(), [N])


@pytest.mark.parametrize("dt", TYPES, ids=[np.dtype(d).name for d in TYPES])
def test_host_alpha_zero_fills_and_leaves_a_nan_filled_a_unread(dt):
    cplx = is_cplx(dt)
    for (ka, other), side in zip(((L + 1, 33), (2 * L + 1, 40)), "LR"):
        m, n = _dims(ka, other, side)
        _, B_d = _data(dt, ka, other, 3)
        A_nan = torch.full((ka, ka), complex(float("nan"), float("nan")) if cplx else float("nan"), dtype=TORCH_DT[np.dtype(dt)], device="cuda")
        EA, EB = Embedded(A_nan, 7, 1, fill=0xFF), Embedded(B_d[side], 1, 1)
        work = torch.empty(g.trsm_work_size(cplx, m, n, side, 7), dtype=torch.uint8, device="cuda")
        _trsm_call(dt, side, "L", "N", "N", m, n, 0, EA, EB, 7, False, work)
        assert torch.equal(EA.bytes, EA.before)
        assert not bool(((EB.bytes != EB.before) & ~EB.inside).any())
        assert not bool(EB.window_words().any()), "the window is not all +0"


@pytest.mark.parametrize("dt,fast", [(np.float64, False), (np.complex128, True)], ids=["float64-accu", "complex128-fast"])
def test_one_row_update_equals_the_model_with_the_cpu_oracles_gemm(dt, fast):
    """(L+1, 33): ONE GEMM, whose shifts the call leaves in its workspace; the CPU oracle's GEMM runs with them, as gpu_util.parity_case does"""
    ka, other, N = L + 1, 33, 14
    rng = np.random.default_rng(11)
    alpha = 0.75 - 0.25j if is_cplx(dt) else 0.75
    for side, uplo, trans, diag in (("L", "L", "N", "N"), ("R", "L", "C", "U"), ("L", "U", "T", "N")):
        m, n = _dims(ka, other, side)
        A, Bm = su.well_conditioned(rng, ka, dt), su.rhs(rng, (m, n), dt)
        dA, dB = gu.to_dev(A), gu.to_dev(Bm)
        _, _, work = g.trsm(dA, dB, N, side=side, uplo=uplo, trans=trans, diag=diag, alpha=alpha, fastmode=fast)
        torch.cuda.synchronize()
        (st,) = [st for st in su.plan(ka, L, side, su.m_is_lower(uplo, trans)) if st[0] == "gemm"]
        gm, gn, gk = (st[4], other, st[2]) if side == "L" else (other, st[4], st[2])
        sft = gu.work_vectors(work, ol.DT[np.dtype(dt)], g.INT8, gm, gn, gk, N)

        def oracle_gemm(lhs, rhs, opL, opR, beta, Cm):
            return np.asarray(ol.gemm(lhs, rhs, N, fastmode=fast, opA=opL, opB=opR, alpha=-1.0, beta=beta, C0=Cm, sftA_in=sft["sftA"], sftB_in=sft["sftB"]))
        want = su.solve(A, Bm, alpha, side, uplo, trans, diag, L, oracle_gemm)
        assert gu.bits_equal(gu.from_dev(dB), want), (side, uplo, trans, diag)


@pytest.mark.parametrize("dt,side,uplo,trans,diag", [(np.float64, "L", "L", "N", "N"), (np.complex64, "R", "U", "C", "U")], ids=["float64-LLNN", "complex64-RUCU"])
def test_graph_capture_replays_to_the_same_bits(dt, side, uplo, trans, diag):
    """a copy-in of B plus the call with timers_ns == NULL, captured once and replayed twice; alpha on the device in the complex case"""
    ka, other, N = 2 * L + 1, 40, 7
    m, n = _dims(ka, other, side)
    A_d, B_all = _data(dt, ka, other, 7)
    B0 = B_all[side]
    alpha = torch.tensor([0.75 - 0.25j], dtype=TORCH_DT[np.dtype(dt)], device="cuda") if is_cplx(dt) else -1
    kw = dict(side=side, uplo=uplo, trans=trans, diag=diag, alpha=alpha)
    for fast in (False, True):
        eager = B0.clone()
        _, _, work = g.trsm(A_d, eager, N, fastmode=fast, **kw)
        torch.cuda.synchronize()
        assert torch.equal(_words(eager), _words(_model(A_d, B0, 0.75 - 0.25j if is_cplx(dt) else -1, side, uplo, trans, diag, N, fast, is_cplx(dt))))
        X = torch.zeros_like(B0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):   # warm-up on the side stream
            X.copy_(B0)
            g.trsm(A_d, X, N, fastmode=fast, work=work, **kw)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            X.copy_(B0)
            g.trsm(A_d, X, N, fastmode=fast, work=work, **kw)
        for _ in range(2):
            X.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert gu.bits_equal(X.cpu().numpy(), eager.cpu().numpy())


def test_python_wrapper_views_and_timers():
    """g.trsm: in place on B, a view of A with a larger leading dimension, timers with the leaf share in slot 2"""
    ka, other, N = 2 * L + 1, 33, 7
    for dt, side in zip(TYPES, "LRLR"):
        A_d, B_all = _data(dt, ka, other, 9)
        EA = Embedded(_poison_dev(A_d, "U", "N"), 7, 1, fill=0xFF)
        ref = _model(A_d, B_all[side], 1, side, "U", "T", "N", N, False)
        Bc = B_all[side].clone()
        out, tm, _ = g.trsm(EA.view, Bc, N, side=side, uplo="U", trans="T", timers=True)
        torch.cuda.synchronize()
        assert out is Bc and len(tm) == 4 and all(t > 0 for t in tm)
        assert torch.equal(_words(Bc), _words(ref))
