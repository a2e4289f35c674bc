"""Seeded random sweep over gemmul8_syrk / gemmul8_herk / gemmul8_syr2k through the C ABI, modelled on tests/test_gpu_fuzz.py: routine x type x trans x uplo x mode
x moduli count x scalar pair x shape x data spread x an all-zero row x operand placement (leading dimensions, base offsets of A, B and C drawn separately, ldc
padding) x host or device scalars x one testing knob.  Every case, through gpu_util.rank_k_case: (a) the stored triangle equals the equivalent gemmul8_gemm run in
the same process, (c) no byte of the sentinel-filled C buffer outside the triangle is written, and the whole buffers of A and B are unchanged; HERK sees NaN in the
incoming diagonal's imaginary parts.  (b), the CPU oracle's GEMM fed with the device GEMM's shifts, runs whenever the oracle's cost by the suites' formulas
(n^2 k N / 1e9 s, x 4 for the complex types, SYR2K with 2 pad256(k) for k) is at most 3 s, if need be with the moduli count cut to 2 -- the plan is fixed by the
seed alone, and test_the_plan_* assert without a GPU that at most a third of the seeds go without (b), that every (routine, type, mode) gets (b) and that every
knob meets every routine at least twice."""
import os

import numpy as np
import pytest

from test_gpu_fuzz import _rand

gpu = pytest.mark.gpu

N_SEEDS = int(os.environ.get("GEMMUL8_FUZZ_RANK_K_SEEDS", "72"))   # the suite runs 72; a longer one-off sweep: GEMMUL8_FUZZ_RANK_K_SEEDS=1000
SEED_BASE = 61278   # chosen on the CPU so that the plan of the 72 default seeds meets test_the_plan_*
ROUTINES = ("syrk", "herk", "syr2k")
DTS = [np.float64, np.float32, np.complex128, np.complex64]
DIMS_N = [1, 2, 31, 255, 256, 257, 300, 513, 769]
DIMS_K = [1, 5, 127, 128, 129, 255, 256, 257, 400, 1023, 1025, 1300]
SCALARS = [(1, 0), (-1, 1), (0.75, -0.5), (0, 2)]                                       # the three suites' lists
CSCALARS = [(1, 0), (-1, 1), (0.75 - 0.25j, -0.5 + 1.5j), (0, 2 - 1j)]
KNOBS = {"GEMMUL8_EPI_NT": (0, 1), "GEMMUL8_BOUND_TILE": (128, 256), "GEMMUL8_SCALE_FOLD": (0,), "GEMMUL8_CPLX_CHUNK": (1, 2, 3), "GEMMUL8_BOUNDS_ONE_READ": (0, 1)}
ORACLE_SECONDS = 3.0


def oracle_seconds(routine, cplx, n, k, N):
    kk = 2 * ((k + 255) // 256 * 256) if routine == "syr2k" else k
    return n * n * kk * N * (4 if cplx else 1) / 1e9


def plan(seed):
    """every draw of a seed, and whether it gets (b); no GPU, no data"""
    rng = np.random.default_rng(SEED_BASE + seed)
    routine = ROUTINES[seed % 3]
    dt = DTS[(seed // 3) % 4]
    if routine == "herk" and np.dtype(dt).kind != "c":
        dt = np.complex128 if dt is np.float64 else np.complex64
    cplx = np.dtype(dt).kind == "c"
    single = dt in (np.float32, np.complex64)
    p = dict(seed=seed, routine=routine, dt=dt, n=int(rng.choice(DIMS_N)), k=int(rng.choice(DIMS_K)))
    p["trans"] = str(rng.choice(["N", "C" if routine == "herk" else "T"]))
    p["uplo"] = str(rng.choice(["L", "U"]))
    p["fast"] = bool(rng.integers(0, 2))
    p["N"] = int(rng.integers(2, 14 if single else 21))
    p["scalars"] = (SCALARS if routine == "herk" or not cplx else CSCALARS)[int(rng.integers(0, 4))]
    p["phi"] = float(rng.choice([0.0, 1.0, 3.0]))
    p["zero_row"] = bool(rng.integers(0, 3) == 0)
    p["ld_extra"] = tuple(int(x) for x in rng.choice([0, 1, 4, 7], 2)) + (int(rng.choice([0, 1, 7, 64])),)
    p["base_off"] = tuple(int(x) for x in rng.integers(0, 2, 3))
    p["scalars_dev"] = bool(rng.integers(0, 2))
    name = [None, *KNOBS][int(rng.integers(0, 6))]
    p["knob"] = (name, int(rng.choice(KNOBS[name]))) if name else None
    p["oracle"] = True
    if oracle_seconds(routine, cplx, p["n"], p["k"], p["N"]) > ORACLE_SECONDS:
        p["N"] = 2   # the type's smallest count, before giving up on (b)
        p["oracle"] = oracle_seconds(routine, cplx, p["n"], p["k"], 2) <= ORACLE_SECONDS
    return p


def test_the_plan_keeps_the_oracle_on_two_thirds_of_the_seeds():
    plans = [plan(s) for s in range(72)]   # (the default sweep, whatever GEMMUL8_FUZZ_RANK_K_SEEDS says)
    assert 3 * sum(not p["oracle"] for p in plans) <= 72
    for p in plans:
        if p["oracle"]:
            assert oracle_seconds(p["routine"], np.dtype(p["dt"]).kind == "c", p["n"], p["k"], p["N"]) <= ORACLE_SECONDS


def test_the_plan_covers_every_routine_type_mode_and_knob():
    plans = [plan(s) for s in range(72)]
    want = {(r, dt, f) for r in ROUTINES for dt in DTS for f in (False, True) if r != "herk" or np.dtype(dt).kind == "c"}
    assert {(p["routine"], p["dt"], p["fast"]) for p in plans if p["oracle"]} == want
    for r in ROUTINES:
        for name in KNOBS:
            assert sum(p["routine"] == r and p["knob"] is not None and p["knob"][0] == name for p in plans) >= 2, (r, name)


@gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_rank_k_case(seed, monkeypatch):
    import gpu_util as gu
    p = plan(seed)
    rng = np.random.default_rng(SEED_BASE + 100000 + seed)
    routine, dt, n, k, t = p["routine"], p["dt"], p["n"], p["k"], p["trans"]
    if p["knob"]:
        gu.setknob(monkeypatch, *p["knob"])
    shape = (n, k) if t == "N" else (k, n)
    A = _rand(shape, dt, rng, p["phi"])
    B = _rand(shape, dt, rng, p["phi"]) if routine == "syr2k" else None
    if p["zero_row"] and n > 2:
        (A if t == "N" else A.T)[n // 2, :] = 0        # an all-zero row of op(A)
    C0 = _rand((n, n), dt, rng, 0.0)
    if routine == "herk":
        C0[np.arange(n), np.arange(n)] = C0[np.arange(n), np.arange(n)].real
    alpha, beta = p["scalars"]
    print(f"plan: {p}")
    gu.rank_k_case(routine, A, B, C0, p["uplo"], t, p["N"], p["fast"], alpha, beta, ld_extra=p["ld_extra"], base_off=p["base_off"], scalars_dev=p["scalars_dev"],
                   oracle=p["oracle"], rng=rng)
