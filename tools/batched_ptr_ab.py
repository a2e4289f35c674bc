#!/usr/bin/env python3
"""Interleaved A/B of the pointer-array batched GEMM on one box, in the manner of tools/trsm_ab.py.  The pointer arrays name the items of ONE contiguous
strided buffer, so every leg computes on the same data.  Legs, interleaved round by round in an order that rotates by one leg per round, medians of --rounds (default 9)
with device events, min and max kept (the spread of a leg is its (max - min) / median; a difference below the larger spread of the two legs compared is not a difference):
  (a) strided      gemmul8_gemm_batched of this tree
  (b) ptr          gemmul8_gemm_batched_ptr of this tree
  (c) strided_reg  (a) with GEMMUL8_CRT_KERNEL=reg: the strided form made to take the CRT's register form, the one the pointer form always takes -- (c) - (a)
                   is what the CRT form costs, (b) - (c) what reading the item addresses from the arrays costs
  (d) native       hipblas{D,Z}gemmBatched of the hipBLAS this process has mapped
  (e) strided_alt  with --alt-lib (a library built from the parent commit): its gemmul8_gemm_batched -- "did the strided form get slower?"
Rows: float64 32 x 512^3 and 8 x 2048^3 at 14 moduli (the two torch.bmm shapes of README.md), complex128 8 x 1024^3.  Accurate mode, INT8 backend.
usage: python tools/batched_ptr_ab.py [--rounds 9] [--moduli 14] [--alt-lib path/to/parent/libgemmul8.so] [--out profiles/batched_ptr_ab.json] [--quick]"""
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
ap.add_argument("--alt-lib", default=None, help="a build of the library from the parent commit")
ap.add_argument("--out", default=None)
ap.add_argument("--quick", action="store_true", help="the 512^3 row only (a smoke run of the tool)")
a = ap.parse_args()
this = g.lib()
alt = None
if a.alt_lib:
    alt = C.CDLL(os.path.abspath(a.alt_lib))
    alt.gemmul8_gemm_batched.restype = C.c_int
    alt.gemmul8_gemm_batched.argtypes = this.gemmul8_gemm_batched.argtypes
st = torch.cuda.current_stream().cuda_stream
TYPES = {"D": (g.D, torch.float64, np.float64), "Z": (g.Z, torch.complex128, np.complex128)}


def native_routine(name):
    """hipblas?gemmBatched on the current stream through the hipBLAS this process has mapped (PyTorch's copy), else the system's"""
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
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return lambda m, n, k, al, pa, pb, be, pc, batch: fn(handle, 111, 111, m, n, k, al.ctypes.data, pa.data_ptr(), m, pb.data_ptr(), k, be.ctypes.data, pc.data_ptr(), m, batch)


def crt_knob(value):
    """GEMMUL8_CRT_KERNEL for the calls of THIS tree's library that follow (parsed once: re-parse)"""
    if value is None:
        os.environ.pop("GEMMUL8_CRT_KERNEL", None)
    else:
        os.environ["GEMMUL8_CRT_KERNEL"] = value
    this.gemmul8_reload_knobs()


cases = [("D", 32, 512), ("D", 8, 2048), ("Z", 8, 1024)]
if a.quick:
    cases = cases[:1]
rows = []
for ty, batch, s in cases:
    code, tdt, sdt = TYPES[ty]
    N = a.moduli
    m = n = k = s
    al, be = np.array([1.0], dtype=sdt), np.array([0.0], dtype=sdt)
    gen = torch.Generator(device="cuda").manual_seed(s + batch)

    def rnd(shape):
        x = torch.rand(shape, generator=gen, device="cuda", dtype=torch.float64) - 0.5
        return torch.complex(x, torch.rand(shape, generator=gen, device="cuda", dtype=torch.float64) - 0.5) if tdt.is_complex else x
    A, B = rnd((batch, k, m)), rnd((batch, n, k))
    Cs = {name: torch.zeros((batch, n, m), dtype=tdt, device="cuda") for name in ("strided", "ptr", "strided_reg", "native", "strided_alt")}
    esz = A.element_size()
    pa = torch.tensor([A.data_ptr() + b * m * k * esz for b in range(batch)], dtype=torch.int64).cuda()
    pb = torch.tensor([B.data_ptr() + b * k * n * esz for b in range(batch)], dtype=torch.int64).cuda()
    pcs = {name: torch.tensor([c.data_ptr() + b * m * n * esz for b in range(batch)], dtype=torch.int64).cuda() for name, c in Cs.items()}
    work = torch.empty(this.gemmul8_work_size_batched(int(tdt.is_complex), g.INT8, m, n, k, N, batch), dtype=torch.uint8, device="cuda")
    native = native_routine("hipblas" + ty + "gemmBatched")

    def strided_of(lib, name):
        return lambda: lib.gemmul8_gemm_batched(st, code, g.INT8, 0, 0, m, n, k, al.ctypes.data, A.data_ptr(), m, m * k, B.data_ptr(), k, k * n, be.ctypes.data,
                                                Cs[name].data_ptr(), m, m * n, batch, N, 0, work.data_ptr())

    def ptr():
        return this.gemmul8_gemm_batched_ptr(st, code, g.INT8, 0, 0, m, n, k, al.ctypes.data, pa.data_ptr(), m, pb.data_ptr(), k, be.ctypes.data, pcs["ptr"].data_ptr(), m,
                                             batch, N, 0, work.data_ptr())
    legs = [("strided", strided_of(this, "strided"), None), ("ptr", ptr, None), ("strided_reg", strided_of(this, "strided_reg"), "reg"),
            ("native", lambda: native(m, n, k, al, pa, pb, be, pcs["native"], batch), None)]
    if alt is not None:
        legs.append(("strided_alt", strided_of(alt, "strided_alt"), None))
    ts = {name: [] for name, _, _ in legs}
    for r in range(a.rounds + 2):
        for name, fn, knob in legs[r % len(legs):] + legs[:r % len(legs)]:   # the order rotates: no leg always runs behind the same neighbour
            if knob:
                crt_knob(knob)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            torch.cuda.synchronize()
            if knob:
                crt_knob(None)
            assert rc == 0, (name, rc)
            if r >= 2:
                ts[name].append(e0.elapsed_time(e1))
    for name in ("ptr", "strided_reg") + (("strided_alt",) if alt is not None else ()):   # every emulated leg computed the same bits
        assert torch.equal(Cs[name].view(torch.uint8), Cs["strided"].view(torch.uint8)), name
    rec = {"routine": ty + "gemmBatched", "batch": batch, "m": m, "n": n, "k": k, "moduli": N, "mode": "accurate", "rounds": a.rounds}
    spread = {}
    for name, _, _ in legs:
        t = sorted(ts[name])
        med = t[len(t) // 2]
        rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = round(med, 4), round(t[0], 4), round(t[-1], 4)
        spread[name] = (t[-1] - t[0]) / med
        rec[name + "_spread"] = round(spread[name], 4)
    flops = 2.0 * m * n * k * batch * (4 if tdt.is_complex else 1)
    rec["ptr_tflops"] = round(flops / rec["ptr_ms"] * 1e-9, 2)

    def compare(x, y):
        ratio = rec[x + "_ms"] / rec[y + "_ms"]
        return round(ratio, 4), abs(ratio - 1.0) <= max(spread[x], spread[y])
    rec["ptr_over_strided"], rec["ptr_vs_strided_within_spread"] = compare("ptr", "strided")
    rec["ptr_over_strided_reg"], rec["ptr_vs_strided_reg_within_spread"] = compare("ptr", "strided_reg")
    rec["crt_form_ms"] = round(rec["strided_reg_ms"] - rec["strided_ms"], 4)   # register form minus what launch_crt selects for the strided call
    rec["ptr_over_native"] = round(rec["ptr_ms"] / rec["native_ms"], 4)
    if alt is not None:
        rec["strided_over_alt"], rec["strided_vs_alt_within_spread"] = compare("strided", "strided_alt")
    rows.append(rec)
    print(json.dumps(rec), flush=True)
    if a.out:   # rewritten after every row: a run that is cut short keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "alt_lib": bool(alt), "results": rows}, f, indent=1)
    del A, B, Cs, work
    torch.cuda.empty_cache()
