#!/usr/bin/env python3
"""Interleaved A/B of gemmul8_trsm on one box, in the manner of tools/trmm_ab.py.  Legs, interleaved round by round, medians of --rounds (default 9) with
device events, min and max kept (the spread is the margin); B is restored from a copy before every call, outside the timed region:
  (a) trsm     gemmul8_trsm, the whole call (in place on B)
  (b) native   hipblas?trsm of the hipBLAS this process has mapped (accurate-mode rows only: it has no modes)
  (c) trmm     gemmul8_trmm of the same shape: about the matrix work the GEMM part of (a) has to do
Beside (a) the timers_ns of a second call in the same round: [scaling, residue GEMMs, LEAF SOLVES, CRT] summed over the call, so the leaf share is visible
(that call synchronises once per GEMM and per leaf and is not the timed one).
Rows: D, left / lower / N / non-unit, ka = 1024 .. 16384 with n = ka and n = 1024; one D right row; Z at 4096 and 8192; both modes at D 8192; and, with
--alt-lib (a laboratory build with the other leaf order: make -C gemmul8_amd/csrc ../lib/lib_trsm_leaf128.so), both candidate L at D 8192 x 8192 and
Z 4096 x 4096, interleaved in the same rounds.  A is well conditioned (off-diagonal entries within +-1/ka, diagonal magnitudes in [1, 2]).
usage: python tools/trsm_ab.py [--rounds 9] [--moduli 14] [--alt-lib gemmul8_amd/lib/lib_trsm_leaf128.so] [--out profiles/trsm_ab.json] [--quick]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gemmul8_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--moduli", type=int, default=14)
ap.add_argument("--alt-lib", default=None, help="a build of the library with the other leaf order")
ap.add_argument("--out", default=None)
ap.add_argument("--quick", action="store_true", help="ka <= 4096 only (a smoke run of the tool)")
a = ap.parse_args()
this = g.lib()
alt = g.bind(C.CDLL(os.path.abspath(a.alt_lib))) if a.alt_lib else None
st = torch.cuda.current_stream().cuda_stream
TYPES = {"D": (g.D, torch.float64, np.float64), "Z": (g.Z, torch.complex128, np.complex128)}


def native_routine(name):
    """hipblas?trsm on the current stream through the hipBLAS this process has mapped (PyTorch's copy), else the system's"""
    path = "libhipblas.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libhipblas.so" in line:
                path = line.split()[-1]
                break
    hb = C.CDLL(path)
    handle = C.c_void_p()
    assert hb.hipblasCreate(C.byref(handle)) == 0 and hb.hipblasSetStream(handle, C.c_void_p(st)) == 0
    fn = getattr(hb, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lambda side, m, n, ka, al, A, B: fn(handle, 141 + side, 122, 111, 131, m, n, al.ctypes.data, A.data_ptr(), ka, B.data_ptr(), m)


# (type, ka, other dimension, side, modes, both leaf orders)
cases = [("D", ka, other, 0, (0, 1) if (ka, other) == (8192, 8192) else (0,), (ka, other) == (8192, 8192))
         for ka in (1024, 2048, 4096, 8192, 16384) for other in sorted({ka, 1024})]
cases += [("D", 8192, 8192, 1, (0,), False), ("Z", 4096, 4096, 0, (0,), True), ("Z", 8192, 8192, 0, (0, 1), False)]
if a.quick:
    cases = [c for c in cases if c[1] <= 4096]
rows = []
for ty, ka, other, side, modes, both_leaves in cases:
    code, tdt, sdt = TYPES[ty]
    N = a.moduli
    al = np.array([1.0], dtype=sdt)
    m, n = (other, ka) if side else (ka, other)
    gen = torch.Generator(device="cuda").manual_seed(ka + other)
    A = (torch.rand((ka, ka), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1) / ka
    d = (1 + torch.rand(ka, generator=gen, device="cuda", dtype=torch.float64)) * (torch.randint(0, 2, (ka,), generator=gen, device="cuda") * 2 - 1)
    A.diagonal().copy_(d)
    A = A.to(tdt)                                               # column-major ka x ka; the LOWER triangle (tensor: triu) is the stored one
    B0 = (torch.rand((n, m), generator=gen, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)   # column-major m x n
    B = torch.empty_like(B0)
    Cout = torch.empty_like(B0)
    wbytes = max(g.trsm_work_size(tdt.is_complex, m, n, "LR"[side], N), g.trmm_work_size(tdt.is_complex, m, n, "LR"[side], N))
    if alt is not None:
        wbytes = max(wbytes, alt.gemmul8_trsm_work_size(int(tdt.is_complex), g.INT8, side, m, n, N))
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    native = native_routine("hipblas" + ty + "trsm")
    for fast in modes:
        def trsm_of(lib):
            return lambda tm=None: lib.gemmul8_trsm(st, code, g.INT8, side, 0, 0, 0, m, n, al.ctypes.data, A.data_ptr(), ka, B.data_ptr(), m, N, fast, work.data_ptr(), tm)

        def trmm(tm=None):
            return this.gemmul8_trmm(st, code, g.INT8, side, 0, 0, 0, m, n, al.ctypes.data, A.data_ptr(), ka, B.data_ptr(), m, Cout.data_ptr(), m, N, fast,
                                     work.data_ptr(), tm)

        legs = [("trsm", trsm_of(this)), ("trmm", trmm)]
        if not fast:
            legs.append(("native", lambda tm=None: native(side, m, n, ka, al, A, B)))
        if both_leaves and alt is not None and not fast:
            legs.append(("trsm_alt", trsm_of(alt)))
        timed = [name for name, _ in legs if name.startswith("trsm")]
        ts = {name: [] for name, _ in legs}
        phases = {name: [] for name in timed}
        for r in range(a.rounds + 2):
            for name, fn in legs:
                B.copy_(B0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0, (name, rc)
                if r >= 2:
                    ts[name].append(e0.elapsed_time(e1))
                if r == 0 and name == "trsm":
                    X_this = B.clone()
                if r == 0 and name == "trsm_alt":   # another L is another recipe: not the same bits, but the same solution
                    alt_diff = float((B - X_this).abs().max() / X_this.abs().max())
                if name in phases and r >= 2 and r % 3 == 2:   # the library's own timers, of a second call
                    B.copy_(B0)
                    tm = (C.c_double * 4)()
                    assert fn(tm) == 0
                    phases[name].append([tm[i] * 1e-6 for i in range(4)])
        rec = {"routine": ty + "trsm", "side": "LR"[side], "uplo": "L", "trans": "N", "diag": "N", "m": m, "n": n, "ka": ka, "moduli": N,
               "mode": "fast" if fast else "accurate", "rounds": a.rounds, "leaf": this.gemmul8_trsm_leaf()}
        for name, fn in legs:
            t = sorted(ts[name])
            rec[name + "_ms"] = round(t[len(t) // 2], 4)
            rec[name + "_min_ms"] = round(t[0], 4)
            rec[name + "_max_ms"] = round(t[-1], 4)
            if name in phases:
                med = [sorted(p[i] for p in phases[name])[len(phases[name]) // 2] for i in range(4)]
                rec[name + "_timers_ms"] = {"scale": round(med[0], 4), "lowprec_gemm": round(med[1], 4), "leaf": round(med[2], 4), "crt": round(med[3], 4)}
        if "trsm_alt_ms" in rec:
            rec["alt_leaf"] = alt.gemmul8_trsm_leaf()
            rec["alt_max_diff_rel"] = alt_diff
        rec["trsm_over_trmm"] = round(rec["trsm_ms"] / rec["trmm_ms"], 4)
        if "native_ms" in rec:
            rec["trsm_over_native"] = round(rec["trsm_ms"] / rec["native_ms"], 4)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:   # rewritten after every row: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, f, indent=1)
    del A, B0, B, Cout, work
    torch.cuda.empty_cache()
