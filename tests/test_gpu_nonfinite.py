"""-m gpu: non-finite mode 1 (gemmul8_set_nonfinite_mode(1), GEMMUL8_NONFINITE=ieee; contract at the declaration in include/gemmul8_c.h).

A row of op(A) / column of op(B) holding a NaN or an Inf is flagged.  Clean entries must be bit-identical to the mode-0 result on A' / B'
(the flagged rows / columns set to zero) -- checked against the oracle and against the library in mode 0 --, flagged entries must be
alpha * s + beta * C in their class (NaN / +Inf / -Inf), s the IEEE sum over k, evaluated here with NumPy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "gemmul8_amd", "lib", "libgemmul8_preload.so")
NMOD = {np.float32: 8, np.float64: 14, np.complex64: 8, np.complex128: 14}


@pytest.fixture(autouse=True)
def mode0_after():
    """The mode is process-wide: every test leaves mode 0 behind (and the FP8 bound mode on which the oracle comparison relies)."""
    gu.select_fp8_bound_mode(gu.SAFE)
    yield
    g.set_nonfinite_mode(0)
    gu.restore_fp8_bound_defaults()


def rand(shape, dt, rng):
    x = rng.random(shape) - 0.5
    if np.dtype(dt).kind == "c":
        x = x + 1j * (rng.random(shape) - 0.5)
    return x.astype(dt)


def stored(op_mat, op):
    """The matrix as the caller stores it for `op` (op(stored) == op_mat)."""
    return op_mat if op == "N" else (op_mat.T.copy() if op == "T" else op_mat.conj().T.copy())


def inject(Aop, Bop, rng):
    """NaN / +-Inf in a few rows of op(A) and columns of op(B).  Returns the flagged row and column indices."""
    m, k = Aop.shape
    n = Bop.shape[1]
    cplx = Aop.dtype.kind == "c"
    r = rng.choice(m, 5, replace=False)
    c = rng.choice(n, 3, replace=False)
    kk = rng.choice(k, 4, replace=False)
    Aop[r[0], kk[0]] = np.nan                      # a single NaN
    Aop[r[1], :] = np.inf                          # a row holding only +Inf
    Aop[r[2], kk[1]] = np.inf                      # an Inf that meets a zero of op(B) in column c[2] (NaN there)
    Bop[kk[1], c[2]] = 0
    Aop[r[3], kk[2]], Aop[r[3], kk[3]] = np.inf, -np.inf   # +Inf and -Inf in one sum
    if cplx:
        Aop[r[4], kk[0]] = complex(1.0, -np.inf)   # only one component non-finite
    else:
        Aop[r[4], kk[0]] = -np.inf
    Bop[kk[2], c[0]] = np.nan
    Bop[kk[3], c[1]] = -np.inf
    Bop[kk[0], c[2]] = np.inf
    return np.sort(r), np.sort(c)


def flagged_masks(Aop, Bop):
    fr = ~np.isfinite(Aop).all(axis=1) if Aop.dtype.kind == "f" else ~(np.isfinite(Aop.real) & np.isfinite(Aop.imag)).all(axis=1)
    fc = ~np.isfinite(Bop).all(axis=0) if Bop.dtype.kind == "f" else ~(np.isfinite(Bop.real) & np.isfinite(Bop.imag)).all(axis=0)
    return fr, fc


def cmul(a, b):
    """Textbook complex product (componentwise), as the contract states it for s and alpha * s."""
    if not np.iscomplexobj(a):
        return a * b
    out = np.empty(np.broadcast(a, b).shape, np.result_type(a, b))   # component by component: `re + 1j * im` would turn the real part into NaN (0 * Inf) wherever im is infinite
    out.real, out.imag = a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real
    return out


def expected_flagged(Aop, Bop, fr, fc, alpha, beta, C0):
    """alpha * s + beta * C (alpha * s when beta == 0) in every flagged entry; NaN-filled elsewhere."""
    m, n = Aop.shape[0], Bop.shape[1]
    dt = Aop.dtype
    out = np.full((m, n), np.nan, dt)
    al, be = dt.type(alpha), dt.type(beta)
    with np.errstate(all="ignore"):
        def s_of(Ai, Bj):  # Ai: (r, k), Bj: (k, c) -> sums over k, componentwise textbook products
            if dt.kind == "c":
                ar, ai, br, bi = Ai.real[:, :, None], Ai.imag[:, :, None], Bj.real[None], Bj.imag[None]
                s = np.empty((Ai.shape[0], Bj.shape[1]), dt)   # component by component: `re + 1j * im` would turn the real part into NaN (0 * Inf) wherever im is infinite
                s.real, s.imag = (ar * br - ai * bi).sum(axis=1), (ar * bi + ai * br).sum(axis=1)
                return s
            return (Ai[:, :, None] * Bj[None]).sum(axis=1).astype(dt)
        S = np.zeros((m, n), dt)
        S[fr, :] = s_of(Aop[fr], Bop)
        S[:, fc] = s_of(Aop, Bop[:, fc])
        val = cmul(np.full_like(S, al), S)
        if beta != 0:
            val = val + cmul(np.full_like(C0, be), C0)
        mask = fr[:, None] | fc[None, :]
        out[mask] = val[mask]
    return out, mask


def classes(x):
    """0 NaN, 1 +Inf, 2 -Inf, 3 finite -- per component for complex values."""
    def one(v):
        return np.where(np.isnan(v), 0, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 3)))
    return np.stack([one(x.real), one(x.imag)]) if np.iscomplexobj(x) else one(x)


def same_bits(a, b):
    """Bit-equal, except that any NaN matches any NaN (payloads differ between the oracle's CPU and the GPU)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "c":
        return same_bits(a.real, b.real) and same_bits(a.imag, b.imag)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8))


def run(Aop, Bop, N, fast, backend, opA, opB, alpha, beta, C0, mode, alpha_dev=False):
    """The library through gemmul8_gemm in non-finite `mode`; scalars on the host, or both on the device."""
    prev = g.set_nonfinite_mode(mode)
    try:
        dA, dB = gu.to_dev(stored(Aop, opA)), gu.to_dev(stored(Bop, opB))
        m, n, k = Aop.shape[0], Bop.shape[1], Aop.shape[1]
        dC = gu.to_dev(C0)
        dt = Aop.dtype
        tot, _, _ = g.work_size(dt.kind == "c", backend, m, n, k, N)
        work = torch.empty(tot, dtype=torch.uint8, device="cuda")
        al, be = np.array([alpha], dt), np.array([beta], dt)
        if alpha_dev:
            dal, dbe = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
            pa, pb = dal.data_ptr(), dbe.data_ptr()
        else:
            pa, pb = al.ctypes.data, be.ctypes.data
        st = torch.cuda.current_stream().cuda_stream
        g.check(g.lib().gemmul8_gemm(st, g._dtype_code(dA.dtype), backend, g.OPS[opA], g.OPS[opB], m, n, k, pa, dA.data_ptr(), dA.shape[1],
                                     dB.data_ptr(), dB.shape[1], pb, dC.data_ptr(), m, N, int(fast), work.data_ptr(), None, None, 0, 0, 0, 0, None))
        torch.cuda.synchronize()
        return gu.from_dev(dC).copy()
    finally:
        g.set_nonfinite_mode(prev)


def zeroed(Aop, Bop, fr, fc):
    A2, B2 = Aop.copy(), Bop.copy()
    A2[fr, :] = 0
    B2[:, fc] = 0
    return A2, B2


def check_case(dt, backend, fast, opA, opB, alpha, beta, shape, seed, alpha_dev=False):
    rng = np.random.default_rng(seed)
    m, n, k = shape
    N = NMOD[dt]
    Aop, Bop = rand((m, k), dt, rng), rand((k, n), dt, rng)
    inject(Aop, Bop, rng)
    fr, fc = flagged_masks(Aop, Bop)
    C0 = rand((m, n), dt, rng)
    # non-finite C at a clean and at a flagged position
    ci = int(np.flatnonzero(~fr)[0]), int(np.flatnonzero(~fc)[0])
    C0[ci] = np.nan
    C0[int(np.flatnonzero(fr)[0]), int(np.flatnonzero(~fc)[1])] = -np.inf
    C0[int(np.flatnonzero(~fr)[1]), int(np.flatnonzero(fc)[0])] = np.inf
    got = run(Aop, Bop, N, fast, backend, opA, opB, alpha, beta, C0, 1, alpha_dev)
    if alpha == 0:
        with np.errstate(all="ignore"):
            want = cmul(np.full_like(C0, dt(beta)), C0) if beta != 0 else np.zeros_like(C0)
        mode0 = run(*zeroed(Aop, Bop, fr, fc), N, fast, backend, opA, opB, alpha, beta, C0, 0, alpha_dev)
        assert same_bits(got, mode0), "alpha == 0: C = beta * C everywhere (the mode-0 result on A', B')"
        assert np.array_equal(classes(got), classes(want))
        return
    A2, B2 = zeroed(Aop, Bop, fr, fc)
    clean = ~(fr[:, None] | fc[None, :])
    mode0 = run(A2, B2, N, fast, backend, opA, opB, alpha, beta, C0, 0, alpha_dev)
    assert same_bits(got[clean], mode0[clean]), "clean entries differ from the library in mode 0 on A', B'"
    orc = ol.gemm(stored(A2, opA), stored(B2, opB), N, fastmode=fast, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0,
                  scalar_mode=1 if alpha_dev else 0)   # device scalars: the CRT's general fma form
    assert same_bits(got[clean], orc[clean]), "clean entries differ from the oracle on A', B'"
    want, mask = expected_flagged(Aop, Bop, fr, fc, alpha, beta, C0)
    cg, cw = classes(got), classes(want)
    assert np.array_equal(cg[..., mask], cw[..., mask]), "flagged entries: class differs from alpha * s + beta * C"
    assert (cg[..., mask] != 3).any()


DTS = [np.float32, np.float64, np.complex64, np.complex128]
CASES = []
_ops = [("N", "N"), ("T", "N"), ("N", "T"), ("C", "T"), ("T", "C"), ("C", "N"), ("N", "C"), ("T", "T")]
_scal = [(1.0, 0.0), (-2.5, 1.0), (1.0, 0.5), (-2.5, 0.0)]
for _i, (_dt, _be, _fast) in enumerate((d, b, f) for d in DTS for b in ("INT8", "FP8") for f in (False, True)):
    _opA, _opB = _ops[_i % len(_ops)]
    if np.dtype(_dt).kind == "f":
        _opA, _opB = _opA.replace("C", "T"), _opB.replace("C", "T")
    _shape = (300, 270, 520) if _i % 4 == 0 else (97, 70, 131)
    CASES.append(pytest.param(_dt, _be, _fast, _opA, _opB, *_scal[_i % len(_scal)], _shape, 100 + _i, id=f"{np.dtype(_dt).name}-{_be}-{'fast' if _fast else 'accu'}-{_opA}{_opB}"))


@pytest.mark.parametrize("dt,backend,fast,opA,opB,alpha,beta,shape,seed", CASES)
def test_nonfinite_contract(dt, backend, fast, opA, opB, alpha, beta, shape, seed):
    check_case(dt, getattr(g, backend), fast, opA, opB, alpha, beta, shape, seed)


@pytest.mark.parametrize("dt,backend,fast,alpha,beta", [(np.float64, "INT8", False, -2.5, 0.5), (np.complex128, "FP8", True, 1.0, 1.0),
                                                        (np.float32, "FP8", False, 0.0, 0.5), (np.complex64, "INT8", True, 0.0, 0.0)])
def test_device_alpha_and_alpha_zero(dt, backend, fast, alpha, beta):
    """alpha (and beta) in device memory; alpha == 0 checked on the device: C = beta * C whatever A and B hold."""
    check_case(dt, getattr(g, backend), fast, "N", "T" if np.dtype(dt).kind == "f" else "C", alpha, beta, (97, 70, 131), seed=5, alpha_dev=True)


@pytest.mark.parametrize("dt,backend,fast", [(np.float64, "INT8", False), (np.float64, "INT8", True), (np.complex64, "FP8", False),
                                             (np.float32, "FP8", True)])
def test_finite_inputs_mode1_equals_mode0(dt, backend, fast):
    rng = np.random.default_rng(11)
    Aop, Bop, C0 = rand((300, 520), dt, rng), rand((520, 270), dt, rng), rand((300, 270), dt, rng)
    be = getattr(g, backend)
    a = run(Aop, Bop, NMOD[dt], fast, be, "N", "N", -2.5, 0.5, C0, 1)
    b = run(Aop, Bop, NMOD[dt], fast, be, "N", "N", -2.5, 0.5, C0, 0)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("fast", [False, True])
def test_skip_scaling_reuses_flags(fast):
    """enable_skip_scalA, then skip_scalA = 1 with a new B: the cached operand's flags come with its planes.  The second call's clean
    entries equal the same two-call sequence in mode 0 on A' (the kept shifts of A come from the first partner in both), the NaN row stays NaN."""
    rng = np.random.default_rng(3)
    m, n, k, N = 97, 70, 131, 14
    A, B, B2 = rand((m, k), np.float64, rng), rand((k, n), np.float64, rng), rand((k, n), np.float64, rng)
    A[17, 40] = np.nan
    lib = g.lib()
    tot, _, _ = g.work_size(False, g.INT8, m, n, k, N, True, False)
    work = torch.zeros(tot, dtype=torch.uint8, device="cuda")
    dA, dB, dB2 = gu.to_dev(A), gu.to_dev(B), gu.to_dev(B2)
    dC = torch.zeros((n, m), dtype=torch.float64, device="cuda")
    one, zero = np.array([1.0]), np.array([0.0])
    st = torch.cuda.current_stream().cuda_stream
    A0 = A.copy()
    A0[17, :] = 0
    dA0 = gu.to_dev(A0)

    def call(Xa, Bt, skA):
        g.check(lib.gemmul8_gemm(st, g.D, g.INT8, 0, 0, m, n, k, one.ctypes.data, Xa.data_ptr(), m, Bt.data_ptr(), k, zero.ctypes.data,
                                 dC.data_ptr(), m, N, int(fast), work.data_ptr(), None, None, 1, 0, skA, 0, None))
        torch.cuda.synchronize()
        return gu.from_dev(dC).copy()
    call(dA0, dB, 0)
    R2 = call(dA0, dB2, 1)   # mode 0 on A'
    g.set_nonfinite_mode(1)
    call(dA, dB, 0)
    L = g.Layout()
    g.check(lib.gemmul8_get_layout(g.D, g.INT8, m, n, k, N, work.data_ptr(), None, None, 1, 0, C.byref(L)))
    sftA = work.cpu().numpy()[L.sftA - work.data_ptr():][:2 * m].view(np.int16)
    assert sftA[17] == -32768 and (sftA != -32768).sum() == m - 1, "flagged row: INT16_MIN in sftA (what gemmul8_get_layout readers see)"
    C2 = call(dA, dB2, 1)
    assert np.array_equal(np.delete(C2, 17, axis=0).view(np.uint8), np.delete(R2, 17, axis=0).view(np.uint8))
    assert np.isnan(C2[17]).all() and np.isfinite(np.delete(C2, 17, axis=0)).all()


@pytest.mark.parametrize("fast", [False, True])
def test_batched_flags_stay_in_their_item(fast):
    rng = np.random.default_rng(4)
    batch, m, n, k, N = 5, 97, 70, 131, 14
    A, B = rand((batch, k, m), np.float64, rng), rand((batch, n, k), np.float64, rng)   # (batch, cols, rows): column-major items
    A[3, 50, 11] = np.nan   # item 3, row 11 of A
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    g.set_nonfinite_mode(1)
    C1, _ = g.gemm_batched(dA, dB, N, fastmode=fast)
    g.set_nonfinite_mode(0)
    A0 = A.copy()
    A0[3, :, 11] = 0
    C0, _ = g.gemm_batched(torch.from_numpy(A0).cuda(), dB, N, fastmode=fast)
    C1, C0 = C1.cpu().numpy(), C0.cpu().numpy()
    for b in (0, 1, 2, 4):
        assert np.array_equal(C1[b].view(np.uint8), C0[b].view(np.uint8)), f"item {b}"
    clean = np.ones((n, m), bool)
    clean[:, 11] = False
    assert np.array_equal(C1[3][clean].view(np.uint8), C0[3][clean].view(np.uint8))
    assert np.isnan(C1[3][:, 11]).all()


def test_graph_capture_replay_mode1():
    """One mode-1 call captured in a torch.cuda.graph and replayed (tests/test_gpu_graph.py): the flags are found on the device."""
    m, n, k, N = 520, 392, 1031, 14
    gen = torch.Generator(device="cuda").manual_seed(3)
    A = (torch.rand((k, m), generator=gen, dtype=torch.float64, device="cuda") - 0.5).contiguous()
    B = (torch.rand((n, k), generator=gen, dtype=torch.float64, device="cuda") - 0.5).contiguous()
    Cg = torch.zeros((n, m), dtype=torch.float64, device="cuda")
    tot, _, _ = g.work_size(False, g.INT8, m, n, k, N)
    work = torch.empty(tot, dtype=torch.uint8, device="cuda")
    g.set_nonfinite_mode(1)
    g.gemm(A, B, N, C_out=Cg, work=work)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.gemm(A, B, N, C_out=Cg, work=work)
    for trial in range(3):
        A.copy_(torch.rand((k, m), generator=gen, dtype=torch.float64, device="cuda") - 0.5)
        A[7 * trial + 1, 100 + trial] = float("nan") if trial != 1 else float("inf")
        B[200 + trial, 3 * trial] = float("-inf")
        Cg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        Ce, _, _ = g.gemm(A, B, N)
        torch.cuda.synchronize()
        a, e = Cg.cpu().numpy(), Ce.cpu().numpy()
        assert np.array_equal(a.view(np.uint8), e.view(np.uint8)), f"replay {trial} differs from the eager call"
        assert not np.isfinite(a[:, 100 + trial]).any() and not np.isfinite(a[200 + trial, :]).any()


_CHILD = r"""
import sys, numpy as np, torch
out = sys.argv[1]
rng = np.random.default_rng(0)
res = {}
for name, dt in (("d", torch.float64), ("s", torch.float32)):
    A = torch.from_numpy(rng.random((200, 300)) - 0.5).to(dt)
    B = torch.from_numpy(rng.random((300, 170)) - 0.5).to(dt)
    A[5, 7] = float("nan"); A[9, :] = float("inf"); A[20, 3] = float("inf"); B[3, 40] = 0.0
    A[33, 1], A[33, 2] = float("inf"), float("-inf"); B[10, 60] = float("-inf"); B[11, 61] = float("nan")
    res["A" + name], res["B" + name] = A.numpy(), B.numpy()
    res["C" + name] = torch.matmul(A.cuda(), B.cuda()).cpu().numpy()
np.savez(out, **res)
"""


def test_hook_torch_matmul_propagates_like_native(tmp_path):
    """Under the preload shim with GEMMUL8_NONFINITE=ieee (fresh child processes): torch.matmul on float64 and float32 with NaN / Inf
    operands has the finite / non-finite pattern of native torch, and the NumPy classes of the contract."""
    assert os.path.exists(SHIM), "libgemmul8_preload.so not built"
    script = tmp_path / "child.py"
    script.write_text(_CHILD)

    def child(env_extra, out):
        env = dict(os.environ)
        env.update(env_extra)
        r = subprocess.run([sys.executable, str(script), str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.load(out)
    nat = child({}, tmp_path / "native.npz")
    hk = child({"LD_PRELOAD": SHIM, "GEMMUL8_NONFINITE": "ieee", "GEMMUL8_NUM_MOD_D": "14", "GEMMUL8_NUM_MOD_S": "8",
                "GEMMUL8_MIN_FLOPS": "0"}, tmp_path / "hook.npz")
    for name in ("d", "s"):
        Ch, Cn = hk["C" + name], nat["C" + name]
        assert np.array_equal(np.isfinite(Ch), np.isfinite(Cn)), name
        A, B = hk["A" + name], hk["B" + name]
        fr, fc = flagged_masks(A, B)
        want, mask = expected_flagged(A, B, fr, fc, 1.0, 0.0, np.zeros_like(Ch))
        assert np.array_equal(classes(Ch)[mask], classes(want)[mask]), name
        assert np.isfinite(Ch[~mask]).all()
        assert np.abs(Ch[~mask] - Cn[~mask]).max() < (1e-4 if name == "s" else 1e-12)   # really emulated (and on A', B')
