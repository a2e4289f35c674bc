"""gemmul8_gemm_batched on the kernel paths tests/test_gpu_batched.py never enters: the three K schedules of the persistent INT8 kernel, workgroups that walk
from one item's planes into the next, the persistent bound GEMM with planes = batch, the FP8 backend's ops / plane formats, views (ld > rows, gaps between
items, stride 0, a strideC off the 16-byte rule), every launcher knob, non-finite mode 1 on views -- each at the smallest shape that selects it.

One driver (gpu_util.batched_views_case) runs every case: the batched call on views inside sentinel-filled buffers, (a) bit-identical to per-item gemmul8_gemm
calls, (b) first / middle / last item bit-identical to the CPU oracle, (c) no byte outside the windows written.  A test that claims a path first asserts the
arithmetic that selects it, from the constants restated below; test_selection_constants_match_the_source (no GPU) holds those against csrc/."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gemmul8_amd", "csrc")

# ---- the selection rules, restated once (the source lines are what test_selection_constants_match_the_source reads)
BM = BN = 256                 # oz2_gemm_common.hpp: constexpr int BM = 256, BN = 256, BK = 128
SHORT_K_MAX_KP = 512          # oz2_gemm_i8.hip, launch<EPI>: a.acc0 = kp * nseg <= 512 ? 0 : 0x80000000 -> launch_sched<EPI, true, 0, true>
OZ2_KBAR_MAX_KP = 5120        # oz2_gemm_i8.hip: #define OZ2_KBAR_MAX_KP 5120 -> launch_sched<EPI, true> up to it, launch_sched<EPI, false> (ping-pong) beyond
OZ2_MAX_SMALL_TILES = 128     # oz2_gemm_i8.hip: #define OZ2_MAX_SMALL_TILES 128 -> the bound GEMM's 128 x 128 kernel while tiles * batch <= it
F6_MIN_N = 64                 # oz2_kernels.h: f6_planes_ok(n) = n >= 64 && ... -> FP6 panel images (lo_format = 1); below 64 columns the e4m3 kernel

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
N_I8 = {F32: 7, F64: 14, C64: 8, C128: 15}
N_F8 = {F32: 6, F64: 12, C64: 7, C128: 9}
# (pad, gap) of A, B, C: ld = rows + pad, stride = ld * cols + gap
VIEWS = [((0, 0, 0), (0, 0, 0)), ((1, 7, 1), (3, 64, 3)), ((7, 0, 7), (64, 3, 0)), ((0, 1, 7), (0, 0, 64)), ((7, 7, 1), (3, 3, 64))]


def pad256(x):
    return (x + 255) // 256 * 256


def tiles(m, n):
    return ((m + BM - 1) // BM) * ((n + BN - 1) // BN)


def i8_schedule(k):
    """the instantiation launch<EPI> of oz2_gemm_i8.hip picks for the residue GEMMs (one K segment)"""
    kp = pad256(k)
    return "short" if kp <= SHORT_K_MAX_KP else "kbar" if kp <= OZ2_KBAR_MAX_KP else "pingpong"


def persistent_grid(cus, gemm_cus=0):
    """workgroups of a persistent launch (launch_sched / oz2_gemm_f6.hip launch): one per CU, a multiple of 8, GEMMUL8_GEMM_CUS below that"""
    grid = cus & ~7
    if 0 < gemm_cus < grid:
        grid = gemm_cus
    return grid or 8


def test_selection_constants_match_the_source():
    """not gpu: the #define / constexpr values behind the path premises, read out of csrc/"""
    i8 = open(os.path.join(CSRC, "oz2_gemm_i8.hip")).read()
    common = open(os.path.join(CSRC, "oz2_gemm_common.hpp")).read()
    assert int(re.search(r"#define OZ2_KBAR_MAX_KP (\d+)", i8).group(1)) == OZ2_KBAR_MAX_KP
    assert int(re.search(r"#define OZ2_MAX_SMALL_TILES (\d+)", i8).group(1)) == OZ2_MAX_SMALL_TILES
    assert int(re.search(r"a\.acc0 = \(size_t\)a\.kp \* \(size_t\)a\.nseg <= (\d+) \? 0 :", i8).group(1)) == SHORT_K_MAX_KP
    assert re.search(r"if \(a\.acc0 == 0\) return launch_sched<EPI, true, 0, true>", i8) and re.search(r"if \(a\.kp \* a\.nseg <= OZ2_KBAR_MAX_KP\) return launch_sched<EPI, true>", i8)
    assert re.search(r"tiles <= \(size_t\)OZ2_MAX_SMALL_TILES", i8)
    mo = re.search(r"constexpr int BM = (\d+), BN = (\d+),", common)
    assert (int(mo.group(1)), int(mo.group(2))) == (BM, BN)
    kernels_h = open(os.path.join(CSRC, "oz2_kernels.h")).read()
    assert int(re.search(r"f6_planes_ok\(size_t n\) \{ return n >= (\d+) &&", kernels_h).group(1)) == F6_MIN_N
    assert [i8_schedule(k) for k in (512, 513, 5120, 5121)] == ["short", "kbar", "kbar", "pingpong"]
    assert [pad256(k) for k in (512, 513, 5120, 5121)] == [512, 768, 5120, 5376]


# ---- case 7's premise (no GPU): the oracle ALONE returns the exact product of small-integer operands
EXACT_R = 500   # entries in [-500, 500] times the item scale 2^(3 b mod 11) <= 2^6 for three items: |C| <= 5121 * (500 * 64)^2 < 2^53, and 10 moduli (P ~ 2^79) leave the
EXACT_N = 10    # quantised operands ~35 bits each: integer * 2^shift is exact with shift >= 0, so nothing is truncated.  (Measured on the oracle: accurate mode is exact
#                 with 8 ... 20 moduli; fast mode with 8 and 10, while from 12 moduli on its CRT leaves fractions of 2^-31 and below of these integers.)
EXACT_CASES = [(512, False), (513, True), (5121, False)]   # (k, fast): one per K schedule -- short-K, K-step barrier, ping-pong
EXACT_M, EXACT_N_COLS, EXACT_BATCH = 257, 40, 3


def exact_items(k):
    import gpu_util as gu

    def ints(shape, dt, rng):
        return rng.integers(-EXACT_R, EXACT_R + 1, shape).astype(dt)
    return gu.batched_data(F64, EXACT_M, EXACT_N_COLS, k, EXACT_BATCH, "N", "N", rng=np.random.default_rng(7000 + k), gen=ints)


def exact_product(A, B):
    P = A.astype(np.int64) @ B.astype(np.int64)   # |entries| < 2^53 < 2^63: exact
    assert np.abs(P).max() < 2 ** 53
    return P.astype(np.float64)


@pytest.mark.parametrize("k,fast", EXACT_CASES)
def test_oracle_alone_is_exact_on_small_integers(k, fast):
    """not gpu: with its own shifts the oracle returns the int64 product exactly, for the first and the last item of test_batched_exact_integer_product's data"""
    import oracle_lib as ol
    As, Bs, _ = exact_items(k)
    for b in (0, EXACT_BATCH - 1):
        Co = np.asarray(ol.gemm(As[b], Bs[b], EXACT_N, fastmode=fast))
        assert np.array_equal(Co, exact_product(As[b], Bs[b])), (k, fast, b)


# ---- the GPU tests
gpu = pytest.mark.gpu


def _g():
    import gemmul8_amd as g
    import gpu_util as gu
    return g, gu


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def scalars(dt, i=0):
    if i % 3 == 2:
        return 1.0, 0.0
    return (-1.5, 0.5) if np.dtype(dt).kind != "c" else (-1.5 + 0.5j, 0.5 - 0.25j)


def run(dt, m, n, k, batch, fast, backend="INT8", N=None, opA="N", opB="N", view=1, scal=0, shareA=False, shareB=False, seed=0, head=0, **kw):
    g, gu = _g()
    be = getattr(g, backend)
    N = N or (N_I8 if backend == "INT8" else N_F8)[dt]
    As, Bs, C0s = gu.batched_data(dt, m, n, k, batch, opA, opB, shareA, shareB, np.random.default_rng(seed))
    alpha, beta = scalars(dt, scal)
    pad, gap = VIEWS[view % len(VIEWS)]
    return gu.batched_views_case(As, Bs, C0s, N, fast, be, opA, opB, alpha, beta, pad, gap, head, **kw)


# 1. K schedules of the persistent INT8 kernel, eight workgroups: every workgroup walks many tiles, across plane and item boundaries.  S, D, C, Z in both modes
# over the four k; 257 x 40 (2 x 1 tiles) everywhere, 257 x 300 (2 x 2) at the two short k.  At k >= 5120 the complex cases hold the first and the last item
# against the oracle and skip the oracle's own-shift run (the oracle needs ~2 s per item there); every other case holds all three items.
_K_CASES = [(512, F64, False), (512, C64, True), (513, F32, False), (513, C128, True), (5120, C128, False), (5120, F32, True), (5121, C64, False), (5121, F64, True)]
K_CASES = [pytest.param(k, dt, fast, 257, 40, i, id=f"k{k}-{np.dtype(dt).name}-{'fast' if fast else 'accu'}-257x40") for i, (k, dt, fast) in enumerate(_K_CASES)]
K_CASES += [pytest.param(k, dt, fast, 257, 300, i + 3, id=f"k{k}-{np.dtype(dt).name}-{'fast' if fast else 'accu'}-257x300") for i, (k, dt, fast) in enumerate(_K_CASES[:4])]
_OPS = [("N", "N"), ("T", "N"), ("N", "T"), ("C", "T"), ("T", "C"), ("C", "N"), ("N", "C"), ("T", "T"), ("C", "C")]


def ops_for(dt, i):
    opA, opB = _OPS[i % len(_OPS)]
    return (opA, opB) if np.dtype(dt).kind == "c" else (opA.replace("C", "T"), opB.replace("C", "T"))


@gpu
@pytest.mark.parametrize("k,dt,fast,m,n,i", K_CASES)
def test_batched_k_schedules(k, dt, fast, m, n, i, monkeypatch):
    g, gu = _g()
    batch, N = 3, 10 if dt == C128 and k >= 5120 else N_I8[dt]
    want = {512: "short", 513: "kbar", 5120: "kbar", 5121: "pingpong"}[k]
    assert i8_schedule(k) == want and pad256(k) == {512: 512, 513: 768, 5120: 5120, 5121: 5376}[k]
    total_tiles = tiles(m, n) * N * batch   # planes of a launch = N moduli per item (complex: per X / Y / Z launch; the scratch, 32 MiB at least, holds the X / Y planes of all N moduli at these sizes)
    assert total_tiles > 8 and persistent_grid(cu_count(), 8) == 8
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", 8)
    opA, opB = ops_for(dt, i)
    slow = np.dtype(dt).kind == "c" and k >= 5120
    run(dt, m, n, k, batch, fast, opA=opA, opB=opB, view=i, scal=i, seed=10 + i, oracle_items=(0, 2) if slow else None, oracle_shifts=not slow)


# 2. workgroups shared by items at the DEFAULT grid: batch x N x tiles > workgroups, the batch count derived from the device's CU count
def items_to_exceed(cus, per_item, at_least):
    return max(at_least, persistent_grid(cus) // per_item + 1)


@gpu
@pytest.mark.parametrize("dt,backend,planes", [(F64, "INT8", None), (C128, "INT8", None), (F32, "FP8", None), (F32, "FP8", "e4m3")],
                         ids=["int8-D", "int8-Z-cplx-epilogue", "fp8-S-fp6-planes", "fp8-S-e4m3-planes"])
def test_batched_items_share_workgroups_at_default_grid(dt, backend, planes, monkeypatch):
    g, gu = _g()
    m, n, k = 300, 300, 200
    N = 14 if backend == "INT8" else 6
    batch = items_to_exceed(cu_count(), tiles(m, n) * N, 6 if backend == "INT8" else 12)
    assert tiles(m, n) == 4 and batch * N * tiles(m, n) > persistent_grid(cu_count()), "some workgroup runs a second tile"
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", None)
    if planes:
        gu.setknob(monkeypatch, "GEMMUL8_FP8_PLANES", planes)
    else:
        assert backend == "INT8" or n >= F6_MIN_N
    run(dt, m, n, k, batch, fast=(dt == C128), backend=backend, N=N, view=2 if backend == "INT8" else 3, seed=20, scal=1 if dt == F32 else 0)


# 3. the bound GEMM's two kernels in a batch (accurate mode): forced, and the persistent one by the rule itself
@gpu
@pytest.mark.parametrize("dt,tile,launches", [(F64, 128, 1), (F64, 256, 1), (F32, 256, 1), (C128, 128, 1), (C128, 256, 1), (C64, 128, 2), (C64, 256, 2), (C128, 256, 2)])
def test_batched_bound_gemm_kernels(dt, tile, launches, monkeypatch):
    """every item's shifts (real types: also its integer row and column maxima; the complex path reuses that scratch for its X / Y planes) equal the per-item
    call's, C equals it and the oracle.  With the 256 x 256 kernel eight workgroups walk the 5 x 4 tiles: each crosses item boundaries."""
    g, gu = _g()
    gu.setknob(monkeypatch, "GEMMUL8_BOUND_TILE", tile)
    if launches == 2:
        gu.setknob(monkeypatch, "GEMMUL8_CPLX_BOUND_LAUNCHES", 2)
    if tile == 256:
        gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", 8)
        assert 5 * tiles(300, 300) > 8
    run(dt, 300, 300, 200, 5, fast=False, view=tile // 128 + launches, seed=30 + tile + launches, maxima=np.dtype(dt).kind == "f", opA="T" if launches == 2 else "N")


@gpu
def test_batched_bound_gemm_persistent_by_rule():
    g, gu = _g()
    batch, m, n = 33, 300, 300
    assert tiles(m, n) * batch == 132 > OZ2_MAX_SMALL_TILES
    run(F64, m, n, 64, batch, fast=False, N=4, view=1, seed=33, maxima=True)


# 4. the remaining knobs in a batch: each against the knob-free result, bitwise (both runs through the driver and its checks)
KNOB_CASES = [
    ("epi_nt", {"GEMMUL8_EPI_NT": 1}, dict(dt=F64, m=300, n=300, k=200, batch=3, fast=False)),
    ("scale_fold_real", {"GEMMUL8_SCALE_FOLD": 0}, dict(dt=F32, m=300, n=70, k=200, batch=3, fast=False, opA="T")),
    ("scale_fold_cplx", {"GEMMUL8_SCALE_FOLD": 0}, dict(dt=C128, m=150, n=70, k=200, batch=3, fast=False)),
    ("cplx_chunk", {"GEMMUL8_CPLX_CHUNK": 1}, dict(dt=C64, m=300, n=70, k=200, batch=3, fast=True)),
    ("map_colblock", {"GEMMUL8_MAP_COLBLOCK": 1, "GEMMUL8_GEMM_CUS": 8}, dict(dt=F64, m=257, n=520, k=200, batch=3, fast=True)),
    ("bounds_one_read", {"GEMMUL8_BOUNDS_ONE_READ": 1}, dict(dt=F64, m=300, n=70, k=256, batch=3, fast=False, opA="N", opB="T")),
    ("fp8_fused_real", {"GEMMUL8_FP8_FUSED": 0}, dict(dt=F32, m=150, n=70, k=200, batch=3, fast=False, backend="FP8")),
    ("fp8_fused_cplx", {"GEMMUL8_FP8_FUSED": 0}, dict(dt=C64, m=150, n=70, k=200, batch=3, fast=True, backend="FP8")),
    ("crt_reg", {"GEMMUL8_CRT_KERNEL": "reg"}, dict(dt=F64, m=1024, n=40, k=96, batch=3, fast=False, view=0)),
    ("crt_dma", {"GEMMUL8_CRT_KERNEL": "dma"}, dict(dt=F64, m=1024, n=40, k=96, batch=3, fast=False, view=0)),
]


@gpu
@pytest.mark.parametrize("name,knobs,case", KNOB_CASES, ids=[c[0] for c in KNOB_CASES])
def test_batched_knob_changes_nothing(name, knobs, case, monkeypatch):
    g, gu = _g()
    case = dict(case)
    if name == "map_colblock":
        assert (case["n"] + BN - 1) // BN >= 3
    base = run(**case, seed=40)
    for kn, v in knobs.items():
        gu.setknob(monkeypatch, kn, v)
    got = run(**case, seed=40, oracle_items=())
    assert gu.bits_equal(got["C"], base["C"]), f"{name}: {int((got['C'].view(np.uint8) != base['C'].view(np.uint8)).sum())} bytes differ from the knob-free result"
    for b, (v0, v1) in enumerate(zip(base["vectors"], got["vectors"])):
        assert np.array_equal(v0["sftA"], v1["sftA"]) and np.array_equal(v0["sftB"], v1["sftB"]), f"{name}: item {b}'s shifts differ from the knob-free call's"


@gpu
@pytest.mark.parametrize("dt,m", [(F32, 1024), (C64, 512), (F64, 1024)])
def test_batched_dma_crt_falls_back_on_unaligned_stride_c(dt, m, monkeypatch):
    """the DMA-eligible shape of test_batched_with_dma_crt_kernel (whole 1024-byte units per column, ldc * element size a multiple of 16), the LDS-DMA form
    forced -- but strideC = ldc * n + 1 elements, which is no multiple of 16 bytes: the launcher must take the register form ((g_batch.sc & 15) == 0)"""
    g, gu = _g()
    gu.setknob(monkeypatch, "GEMMUL8_CRT_KERNEL", "dma")
    n, k, batch = 40, 96, 3
    esz = np.dtype(dt).itemsize
    As, Bs, C0s = gu.batched_data(dt, m, n, k, batch, rng=np.random.default_rng(50))
    alpha, beta = scalars(dt)
    pad, gap = (0, 0, 0), (0, 0, 1)
    assert (m * esz) % 1024 == 0 and ((m + pad[2]) * esz) % 16 == 0 and (((m + pad[2]) * n + gap[2]) * esz) % 16 != 0
    gu.batched_views_case(As, Bs, C0s, N_I8[dt], False, g.INT8, "N", "N", alpha, beta, pad, gap)


# 5. FP8 backend breadth: ops over {N, T, C}^2 for S and C, n on both sides of the FP6 / e4m3 switch, views, one k = 1031
@gpu
@pytest.mark.parametrize("i", range(9))
def test_batched_fp8_ops_and_plane_formats(i):
    g, gu = _g()
    dt = (F32, C64)[i % 2]
    opA, opB = ops_for(dt, i)
    n = (63, 64, 70)[i % 3]
    assert (n >= F6_MIN_N) == (i % 3 != 0)
    run(dt, 150, n, 210, 4, fast=bool(i & 2), backend="FP8", opA=opA, opB=opB, view=i, scal=i, seed=60 + i, shareB=(i == 4), shareA=(i == 7))


@gpu
@pytest.mark.parametrize("dt,n", [(F32, 64), (C64, 63)])
def test_batched_fp8_long_k(dt, n):
    run(dt, 97, n, 1031, 3, fast=False, backend="FP8", opA="T", opB="N", view=4, seed=70)


# 6. non-finite mode 1 in a batch on views
@gpu
@pytest.mark.parametrize("dt,backend,opA,opB", [(F64, "INT8", "T", "N"), (C64, "FP8", "N", "C"), (C128, "INT8", "C", "T")])
def test_batched_nonfinite_on_views(dt, backend, opA, opB):
    """flagged rows in two different items, one flagged column of a B every item shares (strideB = 0), beta != 0 and a NaN already in C at a clean position:
    mode 1 batched equals mode-1 per-item calls (any NaN matching any NaN) with every sentinel byte kept; clean entries equal the mode-0 run on A', B' (the
    flagged rows / columns zeroed; that run against the oracle too); flagged entries are in the class of alpha * s + beta * C."""
    from test_gpu_nonfinite import classes, expected_flagged, flagged_masks, same_bits, stored
    g, gu = _g()
    be = getattr(g, backend)
    rng = np.random.default_rng(80)
    batch, m, n, k = 4, 97, 70, 131
    N = 14 if np.dtype(dt).itemsize >= 8 and dt != C64 else 8
    Aops = [(gu.rand_spread((m, k), dt, rng) * 2.0 ** (3 * b % 11)).astype(dt) for b in range(batch)]
    Bop = gu.rand_spread((k, n), dt, rng)
    C0s = [gu.rand_spread((m, n), dt, rng) for b in range(batch)]
    Aops[1][11, 50] = np.nan
    Aops[3][60, 7] = np.inf
    Aops[3][5, :] = -np.inf if np.dtype(dt).kind == "f" else complex(1.0, -np.inf)
    Bop[100, 33] = -np.inf
    C0s[0][2, 3] = np.nan    # clean in every item: rows 5, 11, 60 and column 33 are the flagged ones
    C0s[3][2, 3] = np.inf
    alpha, beta = (-2.5, 0.5) if np.dtype(dt).kind == "f" else (-2.5 + 1j, 0.5 - 0.25j)
    pad, gap = (1, 7, 7), (3, 0, 64)
    As, Bs = [stored(a, opA) for a in Aops], [stored(Bop, opB)]
    got = gu.batched_views_case(As, Bs, C0s, N, False, be, opA, opB, alpha, beta, pad, gap, mode=1)
    masks = [flagged_masks(a, Bop) for a in Aops]
    assert [int(fr.sum()) for fr, _ in masks] == [0, 1, 0, 2] and all(int(fc.sum()) == 1 for _, fc in masks)
    A0s = []
    for a, (fr, fc) in zip(Aops, masks):
        a = a.copy()
        a[fr, :] = 0
        A0s.append(stored(a, opA))
    B0 = Bop.copy()
    B0[:, masks[0][1]] = 0
    ref = gu.batched_views_case(A0s, [stored(B0, opB)], C0s, N, False, be, opA, opB, alpha, beta, pad, gap, mode=0)
    for b, (fr, fc) in enumerate(masks):
        clean = ~(fr[:, None] | fc[None, :])
        assert same_bits(got["windows"][b][clean], ref["windows"][b][clean]), f"item {b}: clean entries differ from the mode-0 call on A', B'"
        want, mask = expected_flagged(Aops[b], Bop, fr, fc, alpha, beta, C0s[b])
        cg, cw = classes(got["windows"][b]), classes(want)
        assert np.array_equal(cg[..., mask], cw[..., mask]), f"item {b}: flagged entries: class differs from alpha * s + beta * C"
        assert (cg[..., mask] != 3).any()


# 7. a reference that shares no code with the library or the oracle: the exact int64 product of small-integer operands, one float64 case per K schedule
@gpu
@pytest.mark.parametrize("k,fast", EXACT_CASES)
def test_batched_exact_integer_product(k, fast, monkeypatch):
    g, gu = _g()
    assert [i8_schedule(kk) for kk, _ in EXACT_CASES] == ["short", "kbar", "pingpong"]
    gu.setknob(monkeypatch, "GEMMUL8_GEMM_CUS", 8)
    As, Bs, C0s = exact_items(k)
    got = gu.batched_views_case(As, Bs, C0s, EXACT_N, fast, g.INT8, "N", "N", 1.0, 0.0, (1, 7, 1), (3, 64, 3))
    for b in range(EXACT_BATCH):
        ex = exact_product(As[b], Bs[b])
        assert np.array_equal(got["windows"][b], ex), f"item {b}: {int((got['windows'][b] != ex).sum())} entries differ from the exact integer product"


# 8. fuzz on views.  Checks (a) and (c) on every seed; (b) on the even seeds -- seeds 1, 3, 5, 7, 9 and 11 run without the oracle.
FUZZ_SEEDS_WITHOUT_ORACLE = (1, 3, 5, 7, 9, 11)


@gpu
@pytest.mark.parametrize("seed", range(12))
def test_batched_views_fuzz(seed):
    g, gu = _g()
    rng = np.random.default_rng(2000 + seed)
    dt = [F64, F32, C128, C64][seed % 4]
    fp8 = seed % 3 == 2
    m, n = (int(rng.integers(1, 400)) for _ in range(2))
    k = int(rng.integers(1, 1401)) if seed % 2 else int(rng.integers(513, 1401))   # the even seeds past kp = 512 for certain, the odd ones on either side
    batch = int(rng.integers(2, 7))
    cplx = np.dtype(dt).kind == "c"
    opA, opB = (str(rng.choice(["N", "T"] + (["C"] if cplx else []))) for _ in range(2))
    fast = bool(rng.integers(0, 2))
    nmax = (13 if dt in (F32, C64) else 20) if not fp8 else (8 if dt in (F32, C64) else 12)
    N = int(rng.integers(2, nmax + 1))
    pad = tuple(int(rng.choice([0, 1, 7])) for _ in range(3))
    gap = tuple(int(rng.choice([0, 3, 64])) for _ in range(3))
    share = int(rng.integers(0, 4))   # 1: strideA = 0, 2: strideB = 0
    head = int(rng.choice([0, 2]))
    As, Bs, C0s = gu.batched_data(dt, m, n, k, batch, opA, opB, share == 1, share == 2, rng)
    alpha, beta = [(1.0, 0.0), (-1.0, 1.0), (0.75, -0.5)][seed % 3]
    gu.batched_views_case(As, Bs, C0s, N, fast, g.FP8 if fp8 else g.INT8, opA, opB, alpha, beta, pad, gap, head,
                          oracle_items=() if seed in FUZZ_SEEDS_WITHOUT_ORACLE else None, what=f"seed {seed}")
