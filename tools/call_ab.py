#!/usr/bin/env python3
"""A/B of the WHOLE emulated call (gemmul8_gemm: bounds, quantise, low-precision GEMMs, CRT) across several builds of libgemmul8.so
loaded in ONE process and timed INTERLEAVED (A,B,C,A,B,C,...) so that box-to-box and power-state drift cancel.
usage: python tools/call_ab.py [--size 8192 | --m M --n N] [--k 1024,8192] [--moduli 14] [--dtype d|s|z|c] [--fast] [--rounds 9] [--preheat 2]
       [--uniform] lib_a.so lib_b.so[@KNOB=VALUE[,KNOB=VALUE]] ...
An arm is a library, optionally with testing knobs (csrc/oz2_knobs.hpp) that hold for that arm only: every arm is a private copy of its library,
which parses the knobs once.  A knob named by any arm is unset for the arms that do not name it; other knobs come from the caller's environment.  Besides the medians, every arm after the first is reported as a PAIRED difference against the first (mean over the rounds
of t_arm - t_first within a round, and its standard error)."""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gemmul8_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--size", type=int, default=8192)
ap.add_argument("--m", type=int, default=0, help="rows of A / C (default: --size)")
ap.add_argument("--n", type=int, default=0, help="columns of B / C (default: --size)")
ap.add_argument("--preheat", type=float, default=0.0, help="seconds of untimed calls (all arms in turn) before the timed rounds")
ap.add_argument("--uniform", action="store_true", help="operands uniform in [-0.5, 0.5) as bench.py's (default: standard normal)")
ap.add_argument("--k", default="8192")
ap.add_argument("--moduli", type=int, default=14)
ap.add_argument("--dtype", default="d")
ap.add_argument("--fast", action="store_true")
ap.add_argument("--backend", default="int8", help="int8 | fp8")
ap.add_argument("--rounds", type=int, default=9)
a = ap.parse_args()
tdt = {"d": torch.float64, "s": torch.float32, "z": torch.complex128, "c": torch.complex64}[a.dtype]
ndt = {"d": np.float64, "s": np.float32, "z": np.complex128, "c": np.complex64}[a.dtype]
ref = g.lib()
tmp = tempfile.mkdtemp()
libs = []
# an arm = (library path, {knob: value}).  Every knob that ANY arm names is controlled for ALL arms: an arm that does not name it runs with it unset,
# whatever the caller's environment holds; knobs that no arm names are inherited from the caller by every arm alike.  The caller's values are put back below.
arms = [(x.partition("@")[0], dict(kv.split("=", 1) for kv in x.partition("@")[2].split(",") if kv)) for x in a.libs]
names = [x if not kn else f"{x}@{','.join(f'{k}={v}' for k, v in kn.items())}" for x, kn in arms]
controlled = sorted({k for _, kn in arms for k in kn})
saved = {k: os.environ.pop(k, None) for k in controlled}
for i, (pth, kn) in enumerate(arms):
    cp = os.path.join(tmp, f"v{i}.so")
    shutil.copy(pth, cp)
    os.environ.update(kn)
    L = C.CDLL(cp)
    L.gemmul8_reload_knobs.restype = None
    L.gemmul8_reload_knobs()   # this private copy parses its knobs now, once
    for key in kn:
        del os.environ[key]
    L.gemmul8_gemm.restype = C.c_int
    L.gemmul8_gemm.argtypes = ref.gemmul8_gemm.argtypes
    libs.append(L)
os.environ.update({k: v for k, v in saved.items() if v is not None})
N = a.moduli
m, n = a.m or a.size, a.n or a.size
BACKEND = g.FP8 if a.backend.lower() == "fp8" else 0
st = torch.cuda.current_stream().cuda_stream
al, be = np.array([1.0], dtype=ndt), np.array([0.0], dtype=ndt)
for k in [int(x) for x in a.k.split(",")]:
    mk = (lambda *sh: torch.rand(sh, dtype=tdt, device="cuda") - 0.5) if a.uniform else (lambda *sh: torch.randn(sh, dtype=tdt, device="cuda"))
    A = mk(k, m)   # column-major m x k as a (k, m) tensor
    B = mk(n, k)   # column-major k x n as a (n, k) tensor
    Cout = torch.zeros((n, m), dtype=tdt, device="cuda")
    tot, _, _ = g.work_size(tdt.is_complex, BACKEND, m, n, k, N)
    work = torch.empty(tot, dtype=torch.uint8, device="cuda")
    dcode = g._dtype_code(tdt)
    ts = [[] for _ in libs]

    def call(L):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.gemmul8_gemm(st, dcode, BACKEND, g.OPS["N"], g.OPS["N"], m, n, k, al.ctypes.data, A.data_ptr(), m, B.data_ptr(), k,
                            be.ctypes.data, Cout.data_ptr(), m, N, int(a.fast), work.data_ptr(), None, None, 0, 0, 0, 0, None)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1)
    t_end = time.perf_counter() + a.preheat
    while time.perf_counter() < t_end:
        for L in libs:
            call(L)
    for r in range(a.rounds + 2):
        for i, L in enumerate(libs):
            t = call(L)
            if r >= 2:
                ts[i].append(t)
    flops = (8 if tdt.is_complex else 2) * m * n * k
    for i in range(len(libs)):
        t = sorted(ts[i])
        med = t[len(t) // 2]
        print(f"m={m} n={n} k={k:6d} {os.path.basename(names[i]):28s} whole call median {med:8.3f} ms  min {t[0]:8.3f}  -> {flops / med / 1e9:7.1f} TFLOPS", flush=True)
    for i in range(1, len(libs)):
        d = np.array(ts[i]) - np.array(ts[0])
        se = d.std(ddof=1) / np.sqrt(d.size)
        print(f"m={m} n={n} k={k:6d} {os.path.basename(names[i])} - {os.path.basename(names[0])}: paired mean {d.mean() * 1e3:+9.2f} us  s.e. {se * 1e3:7.2f} us"
              f"  ({d.mean() / np.mean(ts[0]) * 100:+.2f} %, {d.mean() / se:+.1f} s.e., {d.size} pairs)", flush=True)
