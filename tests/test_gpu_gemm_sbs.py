"""The residue GEMM's ping-pong schedule with the wave halves' tile epilogues side by side (gemm_i8_sbs_kernel, GEMMUL8_GEMM_SBS=1) against the serialised
form (gemm_i8_kernel, =0): the same planes, byte for byte.  Shapes: k = 5376, the first multiple of 256 above the K-step-barrier schedule's limit (5120),
on 8 workgroups (GEMMUL8_GEMM_CUS=8) so that a workgroup runs several tiles -- the moved barrier sits between two tiles -- and uneven tile counts, ragged
edges and the triangular (SYRK) tile walk.  The barrier order itself is replayed on the host by tests/test_gemm_sbs_barrier_model.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 5376
FILL = 0x5A


def _g():
    import gemmul8_amd as g
    import gpu_util as gu
    image = open(g.LIB_PATH, "rb").read()
    if b"GEMMUL8_GEMM_SBS" not in image or b"gemm_i8_sbs_kernel" not in image:
        pytest.skip("this build has no side-by-side residue GEMM")
    return g, gu


def _operands(m, n, seed):
    rng = np.random.default_rng(seed)
    A = (rng.random((m, K)) - 0.5) * np.exp(rng.standard_normal((m, K)))
    B = (rng.random((K, n)) - 0.5) * np.exp(rng.standard_normal((K, n)))
    return A, B


@pytest.mark.parametrize("m,n,N", [(256, 256, 2),      # 2 tiles, one per workgroup: only the deferred barrier behind the last tile
                                   (512, 768, 3),      # 18 tiles on 8 workgroups: 2 or 3 tiles each
                                   (300, 270, 3)])     # ragged: column guard, partial row tiles
def test_residue_planes_identical(monkeypatch, m, n, N):
    g, gu = _g()
    assert K > 5120 and K % 256 == 0
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", 8)
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_SBS", 0)
    A, B = _operands(m, n, m + n)
    dA, dB = gu.to_dev(A), gu.to_dev(B)
    work = torch.zeros(g.work_size(False, g.INT8, m, n, K, N)[0], dtype=torch.uint8, device="cuda")
    g.gemm(dA, dB, N, fastmode=True, work=work)                     # the quantise pass leaves its planes in the workspace
    torch.cuda.synchronize()
    L = g.Layout()
    g.check(g.lib().gemmul8_get_layout(g.D, g.INT8, m, n, K, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    offC = L.C_mid - work.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    whole = g.work_size(False, g.INT8, m, n, K, N)[0]
    got = {}
    for sbs in (0, 1):
        gu.setknob(monkeypatch, "GEMMUL8_GEMM_SBS", sbs)
        work[offC:offC + N * L.sizeC] = FILL
        before = work.clone()
        g.check(g.lib().gemmul8_lowprec_gemm(st, g.D, g.INT8, m, n, K, N, 0, N, C.byref(L)))
        torch.cuda.synchronize()
        got[sbs] = work[offC:offC + N * L.sizeC].cpu().numpy().copy()
        outside = torch.ones(whole, dtype=torch.bool, device="cuda")
        outside[offC:offC + N * L.sizeC] = False
        assert torch.equal(work[outside], before[outside]), f"GEMMUL8_GEMM_SBS={sbs}: the launch wrote outside C_mid"
    planes = got[0].reshape(N, L.sizeC // L.mp, L.mp)[:, :n, :m]
    assert (planes != FILL).any(axis=(1, 2)).all(), "a residue plane was not written"
    assert np.array_equal(got[0], got[1]), f"{int((got[0] != got[1]).sum())} bytes of C_mid differ between GEMMUL8_GEMM_SBS=0 and 1"


def test_triangular_walk_identical(monkeypatch):
    """512 x 512, 14 moduli through gemmul8_syrk: 3 of 4 tiles per plane, 42 tiles on 8 workgroups."""
    g, gu = _g()
    n, N = 512, 14
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", 8)
    A, _ = _operands(n, 1, 7)
    dA = gu.to_dev(A)
    L = g.Layout()
    out = {}
    for sbs in (0, 1):
        gu.setknob(monkeypatch, "GEMMUL8_GEMM_SBS", sbs)
        work = torch.full((g.work_size(False, g.INT8, n, n, K, N)[0],), FILL, dtype=torch.uint8, device="cuda")
        Cd, _, _ = g.syrk(dA, N, uplo="L", trans="N", fastmode=True, work=work)
        torch.cuda.synchronize()
        g.check(g.lib().gemmul8_get_layout(g.D, g.INT8, n, n, K, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
        offC = L.C_mid - work.data_ptr()
        out[sbs] = (work[offC:offC + N * L.sizeC].cpu().numpy().copy(), Cd.cpu().numpy().copy())
    assert np.array_equal(out[0][0], out[1][0]), f"{int((out[0][0] != out[1][0]).sum())} bytes of C_mid differ between GEMMUL8_GEMM_SBS=0 and 1"
    assert gu.bits_equal(out[0][1], out[1][1])
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_SBS", 0)                   # ... and the triangle is the GEMM's (every tile, serialised form), bit for bit
    Cg, _, _ = g.gemm(dA, dA, N, fastmode=True, opA="N", opB="T")
    torch.cuda.synchronize()
    tri = gu.tri_mask(n, "L").T
    assert gu.bits_equal(out[1][1][tri], Cg.cpu().numpy()[tri])


def test_whole_call_against_the_oracle(monkeypatch):
    """gemmul8_gemm 256 x 256 x 5376, 14 moduli, accurate mode, with the side-by-side kernel: bounds, shifts, planes, C_mid and C against the CPU oracle."""
    g, gu = _g()
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", 8)
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_SBS", 1)
    A, B = _operands(256, 256, 3)
    gu.parity_case(A, B, 14, False)
