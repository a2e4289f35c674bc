#!/usr/bin/env python3
"""Interleaved A/B of gemmul8_trmm on one box: DTRMM and ZTRMM, left / lower / N / non-unit, at 14 moduli, accurate and fast mode, m = n = 8192 and
m = 8192 with n = 1024, plus one RIGHT row.  Legs, interleaved round by round, medians of --rounds (default 9) with device events, min and max kept:
  (a) trmm            gemmul8_trmm, the whole call
  (b) gemm_full       gemmul8_gemm on an already materialised M (the triangle with an explicit zero triangle), without the copy, and
      copy_gemm_full  with the copy in front of it: M built from the stored triangle with a torch op (what a caller without the routine has to do)
  (c) native          hipblas?trmm (out of place) of the hipBLAS this process has mapped (accurate-mode rows only: it has no modes)
Beside every whole-call time of (a) and (b) the residue-GEMM phase, timers_ns[1], of a second call in the same round: its median ratio trmm / gemm_full is
the measured counterpart of the K-step count (T + 1) / (2 T) of a T x T tile grid (T = ka / 256), recorded next to it.
The comparison that counts is (a) against copy_gemm_full; the spread of each leg (min and max of the rounds) is the margin.
usage: python tools/trmm_ab.py [--rounds 9] [--shapes 8192x8192,8192x1024] [--types D,Z] [--moduli 14] [--right 8192x8192] [--out profiles/trmm_ab.json]"""
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
ap.add_argument("--shapes", default="8192x8192,8192x1024", help="m x n of the LEFT rows (A is m x m)")
ap.add_argument("--right", default="8192x8192", help="m x n of the one RIGHT row (type D; A is n x n); empty = none")
ap.add_argument("--types", default="D,Z")
ap.add_argument("--moduli", type=int, default=14)
ap.add_argument("--out", default=None)
a = ap.parse_args()
this = g.lib()
st = torch.cuda.current_stream().cuda_stream
TYPES = {"D": (g.D, torch.float64, np.float64, "hipblasDtrmm"), "Z": (g.Z, torch.complex128, np.complex128, "hipblasZtrmm")}


def native_routine(name):
    """hipblas?trmm on the current stream through the hipBLAS this process has mapped (PyTorch's copy), else the system's"""
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
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lambda side, m, n, ka, al, A, B, Cm: fn(handle, 141 + side, 122, 111, 131, m, n, al.ctypes.data, A.data_ptr(), ka, B.data_ptr(), m, Cm.data_ptr(), m)


cases = [(t, s, 0) for t in a.types.split(",") for s in a.shapes.split(",")] + ([("D", a.right, 1)] if a.right else [])
rows = []
for ty, shape, side in cases:
    code, tdt, sdt, native_name = TYPES[ty]
    N = a.moduli
    al, be = np.array([1.0], dtype=sdt), np.array([0.0], dtype=sdt)
    m, n = (int(x) for x in shape.split("x"))
    ka = n if side else m
    A = torch.randn((ka, ka), dtype=tdt, device="cuda")      # column-major ka x ka; the LOWER triangle (tensor: triu) is the stored one
    B = torch.randn((n, m), dtype=tdt, device="cuda")        # column-major m x n
    M = torch.empty_like(A)
    Cout = torch.zeros((n, m), dtype=tdt, device="cuda")
    work = torch.empty(g.trmm_work_size(tdt.is_complex, m, n, "LR"[side], N), dtype=torch.uint8, device="cuda")

    def materialise():
        """M = Atri from the lower triangle of A: the stored triangle and an explicit zero triangle"""
        torch.triu(A, out=M)

    materialise()
    native = native_routine(native_name)
    for fast in ((0, 1) if side == 0 else (0,)):
        def trmm(tm=None):
            return this.gemmul8_trmm(st, code, g.INT8, side, 0, 0, 0, m, n, al.ctypes.data, A.data_ptr(), ka, B.data_ptr(), m, Cout.data_ptr(), m, N, fast,
                                     work.data_ptr(), tm)

        def gemm_full(tm=None):
            left, right, lda, ldb = (M, B, ka, m) if side == 0 else (B, M, m, ka)
            return this.gemmul8_gemm(st, code, g.INT8, 0, 0, m, n, ka, al.ctypes.data, left.data_ptr(), lda, right.data_ptr(), ldb, be.ctypes.data, Cout.data_ptr(),
                                     m, N, fast, work.data_ptr(), None, None, 0, 0, 0, 0, tm)

        def copy_gemm_full(tm=None):
            materialise()
            return gemm_full(tm)

        legs = [("trmm", trmm), ("gemm_full", gemm_full), ("copy_gemm_full", copy_gemm_full)]
        if not fast:
            legs.append(("native", lambda tm=None: native(side, m, n, ka, al, A, B, Cout)))
        ts = {name: [] for name, _ in legs}
        phases = {"trmm": [], "gemm_full": []}
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
                if name in phases:   # the phase timers of a second call, beside the untimed-by-the-library one above
                    tm = (C.c_double * 4)()
                    assert fn(tm) == 0
                    if r >= 2:
                        phases[name].append((tm[0] * 1e-6, tm[1] * 1e-6, tm[3] * 1e-6))
        T = ka // 256
        rec = {"routine": native_name[7:], "side": "LR"[side], "uplo": "L", "trans": "N", "diag": "N", "m": m, "n": n, "moduli": N,
               "mode": "fast" if fast else "accurate", "rounds": a.rounds}
        for name, fn in legs:
            t = sorted(ts[name])
            rec[name + "_ms"] = round(t[len(t) // 2], 4)
            rec[name + "_min_ms"] = round(t[0], 4)
            rec[name + "_max_ms"] = round(t[-1], 4)
            if name in phases:
                med = [sorted(p[i] for p in phases[name])[len(phases[name]) // 2] for i in range(3)]
                rec[name + "_phases_ms"] = {"scale": round(med[0], 4), "lowprec_gemm": round(med[1], 4), "crt": round(med[2], 4)}
                lp = sorted(p[1] for p in phases[name])
                rec[name + "_lowprec_gemm_min_max_ms"] = [round(lp[0], 4), round(lp[-1], 4)]
        rec["trmm_over_gemm_full"] = round(rec["trmm_ms"] / rec["gemm_full_ms"], 4)
        rec["trmm_over_copy_gemm_full"] = round(rec["trmm_ms"] / rec["copy_gemm_full_ms"], 4)
        rec["lowprec_gemm_ratio"] = round(rec["trmm_phases_ms"]["lowprec_gemm"] / rec["gemm_full_phases_ms"]["lowprec_gemm"], 4)
        rec["k_step_count_ratio"] = round((T + 1) / (2 * T), 4) if T else None
        if "native_ms" in rec:
            rec["trmm_over_native"] = round(rec["trmm_ms"] / rec["native_ms"], 4)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": rows}, f, indent=1)
