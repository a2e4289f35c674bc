#!/usr/bin/env python3
"""Interleaved A/B of gemmul8_syrk against the GEMM it replaces, gemmul8_gemm(A, A^T), on one box: DSYRK n = k = 8192, n = 8192 k = 1024 and
n = 16384 k = 512, 14 moduli, accurate and fast mode.  The GEMM side may come from another build of libgemmul8.so (--gemm-lib: e.g. the parent
commit's), loaded in the same process; a second GEMM column of this build shows that the GEMM itself did not move.  Per-phase timers
(timers_ns: scaling, low-precision GEMMs, CRT) of one extra call each are printed beside the medians.
--herk: gemmul8_herk against gemmul8_gemm(A, A^H) instead -- ZHERK n = k = 8192 at 20 moduli and CHERK at 13 (--shapes / --moduli / --types override).
--syr2k: gemmul8_syr2k against what replaced it before the routine existed -- gemmul8_gemm on the materialised P = [A, Z, B, Z] and Q = [B, Z, A, Z]
(the GEMM alone, and with the two packing copies in front of it) -- and against the native hipblas?syr2k: D, 14 moduli, n = 8192 with k = 4096 and k = 512.
--her2k: gemmul8_her2k against what a caller does today -- gemmul8_gemm for W = A B^H, then torch operations for alpha W + (alpha W)^H over the full
square -- and against the native hipblasZher2k: Z, 14 moduli, n = 8192 with k = 4096, 512 and 64 (profiles/her2k_ab.json).
usage: python tools/syrk_ab.py [--herk | --syr2k | --her2k] [--gemm-lib parent/libgemmul8.so] [--rounds 9] [--shapes 8192x8192,8192x1024,16384x512] [--moduli 14] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gemmul8_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("--gemm-lib", default=None)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--herk", action="store_true")
ap.add_argument("--syr2k", action="store_true")
ap.add_argument("--her2k", action="store_true")
ap.add_argument("--shapes", default=None)
ap.add_argument("--moduli", type=int, default=None, help="default: 14 (SYRK); --herk: 20 for Z, 13 for C")
ap.add_argument("--types", default=None, help="SYRK: D; --herk: Z,C")
ap.add_argument("--out", default=None)
a = ap.parse_args()
this = g.lib()
other = None
if a.gemm_lib:
    cp = os.path.join(tempfile.mkdtemp(), "gemm_side.so")
    shutil.copy(a.gemm_lib, cp)
    other = C.CDLL(cp)
    other.gemmul8_gemm.restype = C.c_int
    other.gemmul8_gemm.argtypes = this.gemmul8_gemm.argtypes
st = torch.cuda.current_stream().cuda_stream
TYPES = {"S": (g.S, torch.float32, np.float32, np.float32), "D": (g.D, torch.float64, np.float64, np.float64), "Z": (g.Z, torch.complex128, np.complex128, np.float64),
         "C": (g.Cx, torch.complex64, np.complex64, np.float32)}   # code, tensor type, GEMM scalar type, rank-k scalar type


def native_syr2k(ty, routine="syr2k"):
    """hipblas{S,D}syr2k (or hipblas{C,Z}her2k: the same argument list) on the current stream through the hipBLAS this process has mapped (PyTorch's copy), else the system's"""
    path = "libhipblas.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libhipblas.so" in line:
                path = line.split()[-1]
                break
    hb = C.CDLL(path)
    handle = C.c_void_p()
    assert hb.hipblasCreate(C.byref(handle)) == 0 and hb.hipblasSetStream(handle, C.c_void_p(st)) == 0
    fn = getattr(hb, f"hipblas{ty}{routine}")
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    return lambda n, k, al, A, B, be, Cm: fn(handle, 122, 111, n, k, al.ctypes.data, A.data_ptr(), n, B.data_ptr(), n, be.ctypes.data, Cm.data_ptr(), n)


def syr2k_ab():
    rows = []
    for ty, shape in ((t, s) for t in (a.types or "D").split(",") for s in (a.shapes or "8192x4096,8192x512").split(",")):
        code, tdt, gdt, _ = TYPES[ty]
        N = a.moduli or 14
        al, be = np.array([1.0], dtype=gdt), np.array([0.0], dtype=gdt)
        n, k = (int(x) for x in shape.split("x"))
        kh = (k + 255) // 256 * 256
        A, B = (torch.randn((k, n), dtype=tdt, device="cuda") for _ in range(2))   # column-major n x k
        P, Q = (torch.zeros((2 * kh, n), dtype=tdt, device="cuda") for _ in range(2))

        def pack():
            P[:k], P[kh:kh + k], Q[:k], Q[kh:kh + k] = A, B, B, A
        pack()
        Cout = torch.zeros((n, n), dtype=tdt, device="cuda")
        work = torch.empty(g.syr2k_work_size(tdt.is_complex, n, k, N), dtype=torch.uint8, device="cuda")
        native = native_syr2k(ty) if ty in "SD" else None
        for fast in (0, 1):
            def gemm(tm=None):
                return this.gemmul8_gemm(st, code, g.INT8, 0, 1, n, n, 2 * kh, al.ctypes.data, P.data_ptr(), n, Q.data_ptr(), n, be.ctypes.data, Cout.data_ptr(), n, N,
                                         fast, work.data_ptr(), None, None, 0, 0, 0, 0, tm)

            def pack_gemm(tm=None):
                pack()
                return gemm(tm)

            def syr2k(tm=None):
                return this.gemmul8_syr2k(st, code, g.INT8, 0, 0, n, k, al.ctypes.data, A.data_ptr(), n, B.data_ptr(), n, be.ctypes.data, Cout.data_ptr(), n, N, fast,
                                          work.data_ptr(), tm)
            legs = [("syr2k", syr2k), ("gemm_pq", gemm), ("pack_gemm_pq", pack_gemm)]
            if native and not fast:
                legs.append(("native", lambda tm=None: native(n, k, al, A, B, be, Cout)))
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
            rec = {"type": ty, "n": n, "k": k, "moduli": N, "mode": "fast" if fast else "accurate", "rounds": a.rounds}
            for name, fn in legs:
                t = sorted(ts[name])
                rec[name + "_ms"] = round(t[len(t) // 2], 4)
                rec[name + "_min_ms"] = round(t[0], 4)
                if name in ("syr2k", "gemm_pq"):
                    tm = (C.c_double * 4)()
                    assert fn(tm) == 0
                    rec[name + "_phases_ms"] = {"scale": round(tm[0] * 1e-6, 4), "lowprec_gemm": round(tm[1] * 1e-6, 4), "crt": round(tm[3] * 1e-6, 4)}
            rec["syr2k_over_gemm_pq"] = round(rec["syr2k_ms"] / rec["gemm_pq_ms"], 4)
            rec["syr2k_over_pack_gemm_pq"] = round(rec["syr2k_ms"] / rec["pack_gemm_pq_ms"], 4)
            if "native_ms" in rec:
                rec["syr2k_over_native"] = round(rec["syr2k_ms"] / rec["native_ms"], 4)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    return rows


def her2k_ab():
    rows = []
    for ty, shape in ((t, s) for t in (a.types or "Z").split(",") for s in (a.shapes or "8192x4096,8192x512,8192x64").split(",")):
        code, tdt, gdt, rdt = TYPES[ty]
        N = a.moduli or 14
        alpha = 0.75 - 0.25j
        al, be, rbe = np.array([alpha], dtype=gdt), np.array([0.0], dtype=gdt), np.array([0.0], dtype=rdt)
        one = np.array([1.0], dtype=gdt)
        n, k = (int(x) for x in shape.split("x"))
        A, B = (torch.randn((k, n), dtype=tdt, device="cuda") for _ in range(2))   # column-major n x k
        W, Cout = (torch.zeros((n, n), dtype=tdt, device="cuda") for _ in range(2))
        work = torch.empty(g.her2k_work_size(n, k, N), dtype=torch.uint8, device="cuda")
        native = native_syr2k(ty, "her2k")
        for fast in (0, 1):
            def gemm_w(tm=None):
                return this.gemmul8_gemm(st, code, g.INT8, 0, 2, n, n, k, one.ctypes.data, A.data_ptr(), n, B.data_ptr(), n, be.ctypes.data, W.data_ptr(), n, N, fast,
                                         work.data_ptr(), None, None, 0, 0, 0, 0, tm)

            def gemm_combine(tm=None):
                rc = gemm_w(tm)
                aw = W * alpha
                torch.add(aw, aw.mH, out=Cout)   # W is held transposed, and so is Cout: the conjugate transpose is the same view on both
                return rc

            def her2k(tm=None):
                return this.gemmul8_her2k(st, code, g.INT8, 0, 0, n, k, al.ctypes.data, A.data_ptr(), n, B.data_ptr(), n, rbe.ctypes.data, Cout.data_ptr(), n, N, fast,
                                          work.data_ptr(), tm)
            legs = [("her2k", her2k), ("gemm_w", gemm_w), ("gemm_combine", gemm_combine)]
            if not fast:
                legs.append(("native", lambda tm=None: native(n, k, al, A, B, rbe, Cout)))
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
            rec = {"type": ty, "n": n, "k": k, "moduli": N, "mode": "fast" if fast else "accurate", "rounds": a.rounds}
            for name, fn in legs:
                t = sorted(ts[name])
                rec[name + "_ms"] = round(t[len(t) // 2], 4)
                rec[name + "_min_ms"] = round(t[0], 4)
                if name in ("her2k", "gemm_w"):
                    tm = (C.c_double * 4)()
                    assert fn(tm) == 0
                    rec[name + "_phases_ms"] = {"scale": round(tm[0] * 1e-6, 4), "lowprec_gemm": round(tm[1] * 1e-6, 4), "crt": round(tm[3] * 1e-6, 4)}
            rec["her2k_over_gemm_combine"] = round(rec["her2k_ms"] / rec["gemm_combine_ms"], 4)
            if "native_ms" in rec:
                rec["her2k_over_native"] = round(rec["her2k_ms"] / rec["native_ms"], 4)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    return rows


shapes = a.shapes or ("8192x8192" if a.herk else "8192x8192,8192x1024,16384x512")
rows = syr2k_ab() if a.syr2k else her2k_ab() if a.her2k else []
for ty, shape in ((t, s) for t in (() if a.syr2k or a.her2k else (a.types or ("Z,C" if a.herk else "D")).split(",")) for s in shapes.split(",")):
    code, tdt, gdt, rdt = TYPES[ty]
    N = a.moduli or ((20 if ty == "Z" else 13) if a.herk else 14)
    al, be = np.array([1.0], dtype=gdt), np.array([0.0], dtype=gdt)      # the GEMM's scalars (complex for Z / C)
    ral, rbe = np.array([1.0], dtype=rdt), np.array([0.0], dtype=rdt)    # SYRK: the same type; HERK: real
    n, k = (int(x) for x in shape.split("x"))
    A = torch.randn((k, n), dtype=tdt, device="cuda")   # column-major n x k
    Cout = torch.zeros((n, n), dtype=tdt, device="cuda")
    work = torch.empty(g.work_size(tdt.is_complex, g.INT8, n, n, k, N)[0], dtype=torch.uint8, device="cuda")
    for fast in (0, 1):
        def gemm(L, tm=None):
            return L.gemmul8_gemm(st, code, g.INT8, 0, 2 if a.herk else 1, n, n, k, al.ctypes.data, A.data_ptr(), n, A.data_ptr(), n, be.ctypes.data,
                                  Cout.data_ptr(), n, N, fast, work.data_ptr(), None, None, 0, 0, 0, 0, tm)

        def syrk(L, tm=None):
            fn = L.gemmul8_herk if a.herk else L.gemmul8_syrk
            return fn(st, code, g.INT8, 0, 0, n, k, (ral if a.herk else al).ctypes.data, A.data_ptr(), n, (rbe if a.herk else be).ctypes.data, Cout.data_ptr(), n, N,
                      fast, work.data_ptr(), tm)
        rk = "herk" if a.herk else "syrk"
        legs = [(rk, lambda tm=None: syrk(this, tm)), ("gemm", lambda tm=None: gemm(this, tm))]
        if other is not None:
            legs.append(("gemm_other_lib", lambda tm=None: gemm(other, tm)))
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
        rec = {"type": ty, "n": n, "k": k, "moduli": N, "mode": "fast" if fast else "accurate", "rounds": a.rounds}
        for name, fn in legs:
            t = sorted(ts[name])
            tm = (C.c_double * 4)()
            assert fn(tm) == 0
            rec[name + "_ms"] = round(t[len(t) // 2], 4)
            rec[name + "_min_ms"] = round(t[0], 4)
            rec[name + "_phases_ms"] = {"scale": round(tm[0] * 1e-6, 4), "lowprec_gemm": round(tm[1] * 1e-6, 4), "crt": round(tm[3] * 1e-6, 4)}
        base = rec.get("gemm_other_lib_ms", rec["gemm_ms"])
        rec[rk + "_over_gemm"] = round(rec[rk + "_ms"] / base, 4)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "gemm_side": "other build" if other is not None else "this build", "results": rows}, f, indent=1)
