#!/usr/bin/env python3
"""Interleaved A/B of gemmul8_symm / gemmul8_hemm on one box, side = L: DSYMM and ZHEMM at 14 moduli, accurate and fast mode, m = n = 8192 and
m = 8192 with n = 1024.  Legs, interleaved round by round, medians of --rounds (default 9) with device events:
  (a) symm            gemmul8_symm / gemmul8_hemm, the whole call; timers_ns[0] (the scaling phase) of one extra call beside it
  (b) gemm_full       gemmul8_gemm on a materialised Afull, without the copy, and
      copy_gemm_full  with the copy in front of it: Afull built from the stored triangle with torch ops (what a caller without the routine has to do)
  (c) native          hipblasDsymm / hipblasZhemm of the hipBLAS this process has mapped (accurate-mode rows only: it has no modes)
The comparison that counts is (a) against copy_gemm_full; the spread of each leg (min and max of the rounds) is the margin.
usage: python tools/symm_ab.py [--rounds 9] [--shapes 8192x8192,8192x1024] [--types D,Z] [--moduli 14] [--out profiles/symm_ab.json]"""
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
ap.add_argument("--shapes", default="8192x8192,8192x1024", help="m x n; side = L, so A is m x m")
ap.add_argument("--types", default="D,Z", help="D: DSYMM, Z: ZHEMM")
ap.add_argument("--moduli", type=int, default=14)
ap.add_argument("--out", default=None)
a = ap.parse_args()
this = g.lib()
st = torch.cuda.current_stream().cuda_stream
TYPES = {"D": (g.D, torch.float64, np.float64, "gemmul8_symm", "hipblasDsymm"), "Z": (g.Z, torch.complex128, np.complex128, "gemmul8_hemm", "hipblasZhemm")}


def native_routine(name):
    """hipblasDsymm / hipblasZhemm on the current stream through the hipBLAS this process has mapped (PyTorch's copy), else the system's"""
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
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    return lambda m, n, al, A, B, be, Cm: fn(handle, 141, 122, m, n, al.ctypes.data, A.data_ptr(), m, B.data_ptr(), m, be.ctypes.data, Cm.data_ptr(), m)


rows = []
for ty, shape in ((t, s) for t in a.types.split(",") for s in a.shapes.split(",")):
    code, tdt, sdt, entry, native_name = TYPES[ty]
    herm = ty == "Z"
    N = a.moduli
    al, be = np.array([1.0], dtype=sdt), np.array([0.0], dtype=sdt)
    m, n = (int(x) for x in shape.split("x"))
    A = torch.randn((m, m), dtype=tdt, device="cuda")        # column-major m x m; the LOWER triangle (tensor: triu) is the stored one
    B = torch.randn((n, m), dtype=tdt, device="cuda")        # column-major m x n
    Afull = torch.empty_like(A)
    Cout = torch.zeros((n, m), dtype=tdt, device="cuda")
    work = torch.empty(g.symm_work_size(tdt.is_complex, m, n, "L", N), dtype=torch.uint8, device="cuda")
    diag = torch.arange(m, device="cuda")

    def materialise():
        """Afull from the lower triangle of A with torch ops: the stored triangle, its (conjugate) transpose across, a real diagonal for HEMM"""
        up = torch.triu(A)
        strict = torch.triu(A, 1)
        torch.add(up, (strict.conj() if herm else strict).transpose(0, 1), out=Afull)
        if herm:
            Afull[diag, diag] = Afull[diag, diag].real.to(tdt)

    materialise()
    native = native_routine(native_name)
    fn_symm = getattr(this, entry)
    for fast in (0, 1):
        def symm(tm=None):
            return fn_symm(st, code, g.INT8, 0, 0, m, n, al.ctypes.data, A.data_ptr(), m, B.data_ptr(), m, be.ctypes.data, Cout.data_ptr(), m, N, fast,
                           work.data_ptr(), tm)

        def gemm_full(tm=None):
            return this.gemmul8_gemm(st, code, g.INT8, 0, 0, m, n, m, al.ctypes.data, Afull.data_ptr(), m, B.data_ptr(), m, be.ctypes.data, Cout.data_ptr(), m, N,
                                     fast, work.data_ptr(), None, None, 0, 0, 0, 0, tm)

        def copy_gemm_full(tm=None):
            materialise()
            return gemm_full(tm)

        legs = [("symm", symm), ("gemm_full", gemm_full), ("copy_gemm_full", copy_gemm_full)]
        if not fast:
            legs.append(("native", lambda tm=None: native(m, n, al, A, B, be, Cout)))
        ts = {name: [] for name, _ in legs}
        for r in range(a.rounds + 2):
            for name, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0, (name, rc)
                if r >= 2:
                    ts[name].append(e0.elapsed_time(e1))
        rec = {"routine": native_name[7:], "side": "L", "uplo": "L", "m": m, "n": n, "moduli": N, "mode": "fast" if fast else "accurate", "rounds": a.rounds}
        for name, fn in legs:
            t = sorted(ts[name])
            rec[name + "_ms"] = round(t[len(t) // 2], 4)
            rec[name + "_min_ms"] = round(t[0], 4)
            rec[name + "_max_ms"] = round(t[-1], 4)
            if name in ("symm", "gemm_full"):
                tm = (C.c_double * 4)()
                assert fn(tm) == 0
                rec[name + "_phases_ms"] = {"scale": round(tm[0] * 1e-6, 4), "lowprec_gemm": round(tm[1] * 1e-6, 4), "crt": round(tm[3] * 1e-6, 4)}
        rec["symm_over_gemm_full"] = round(rec["symm_ms"] / rec["gemm_full_ms"], 4)
        rec["symm_over_copy_gemm_full"] = round(rec["symm_ms"] / rec["copy_gemm_full_ms"], 4)
        if "native_ms" in rec:
            rec["symm_over_native"] = round(rec["symm_ms"] / rec["native_ms"], 4)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, f, indent=1)
