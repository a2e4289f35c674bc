#!/usr/bin/env python3
"""Turn two rocprofv3 counter-collection passes (FETCH_SIZE, WRITE_SIZE -- separate passes, tools/pmc_fetch.txt and
tools/pmc_write.txt) into a per-kernel HBM-side traffic summary: profiles/<tag>_pmc_traffic.json.

Units/corrections (guides/MI355X_MICROARCH.md, HBM section): both counters are in KiB; on gfx950 FETCH_SIZE reports HALF the
bytes of wide coalesced streaming reads (128-B requests tallied at 64 B).  Which kernels that applies to is CALIBRATED here,
not assumed: every streaming kernel of the pipeline reads a known number of bytes exactly once per launch (the operand for the
scale kernels, the N residue planes for the CRT), so factor = round(known bytes / reported bytes) in {1, 2}, printed as evidence;
the GEMM kernels (all reads are global_load_lds_dwordx4, 16 B per lane) take the guide's x2.  Round 1 applied x2 to the GEMM
kernels only, which left the quantise (32 B per lane) and CRT (8 B per lane, 512 B per wave and plane) kernels a factor 2 low
(VERDICT r01).  WRITE_SIZE matched the known byte counts of every kernel and is used as reported.

usage: tools/pmc_traffic.py <fetch_dir> <write_dir> <out.json> [n=8192] [N=14] [fp8]   (fp8: config 3, SGEMM n^3 on the FP8 backend)
"""
import collections
import csv
import glob
import json
import sys


def collect(root, counter):
    acc = collections.defaultdict(list)
    for f in glob.glob(root + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter and "oz2::" in r["Kernel_Name"]:
                acc[r["Kernel_Name"].split("(")[0].replace("void ", "")].append(float(r["Counter_Value"]))
    return {k: sum(v) / len(v) for k, v in acc.items()}


fetch = collect(sys.argv[1], "FETCH_SIZE")
write = collect(sys.argv[2], "WRITE_SIZE")
n = int(sys.argv[4]) if len(sys.argv) > 4 else 8192
N = int(sys.argv[5]) if len(sys.argv) > 5 else 14
operand = n * n * 8.0  # one FP64 operand
known_reads = {  # bytes a launch reads exactly once (config 2: DGEMM n^3, N moduli, op N/N)
    "oz2::amax_strided_kernel<double>": operand,
    "oz2::amax_pair_kernel<double>": operand,            # round 6 names (config 2, op N/N: A is the one row-strided operand)
    "oz2::extract_pair_kernel<double>": 2 * operand,
    "oz2::extract_strided_kernel<double>": operand,
    "oz2::extract_kmajor_kernel<double>": operand,
    "oz2::quantise_pair_kernel<double>": 2 * operand,       # round 4: A and B in one launch
    "oz2::fast_shift_pair_kernel<double>": 2 * operand,
    "oz2::crt_dma_kernel<double, false>": N * n * n * 1.0,   # the residue planes (beta = 0: C is not read)
    "oz2::crt_kernel<double, false, signed char>": N * n * n * 1.0,
    # names of rounds 1-3 (one launch per operand)
    "oz2::stage_strided_kernel<double, 0>": operand,
    "oz2::stage_kmajor_kernel<double, 0>": operand,
    "oz2::stage_strided_kernel<double, 1>": operand,
    "oz2::stage_kmajor_kernel<double, 1>": operand,
}
if len(sys.argv) > 6 and sys.argv[6] == "fp8":   # config 3: SGEMM n^3, N moduli, FP8 backend (float operands, int16 residue planes)
    op32 = n * n * 4.0
    known_reads = {
        "oz2::amax_strided_kernel<float>": op32,
        "oz2::amax_pair_kernel<float>": op32,
        "oz2::extract_pair_kernel<float>": 2 * op32,
        "oz2::extract_strided_kernel<float>": op32,
        "oz2::extract_kmajor_kernel<float>": op32,
        "oz2::quantise_f6_pair_kernel<float>": 2 * op32,
        "oz2::quantise_pair_kernel<float>": 2 * op32,
        "oz2::fast_shift_pair_kernel<float>": 2 * op32,
    }
out = {}
for k in sorted(set(fetch) | set(write)):
    f_kib, w_kib = fetch.get(k, 0.0), write.get(k, 0.0)
    if "gemm_i8_kernel" in k or "gemm_i8_sbs_kernel" in k or "gemm_i8_kr_kernel" in k or "gemm_f8_kernel" in k or "gemm_f6_kernel" in k:
        corr, why = 2.0, "16 B/lane LDS-DMA reads (guide)"
    elif "crt_kernel<float" in k and f_kib > 0 and len(sys.argv) > 6:   # the N int16 residue planes, read once (beta = 0)
        ratio = N * n * n * 2.0 / (f_kib * 1024.0)
        corr = 2.0 if ratio > 1.5 else 1.0
        why = f"calibrated: reads {N * n * n * 2.0 / 2**20:.0f} MiB once, counter says {f_kib / 1024:.0f} MiB (ratio {ratio:.2f})"
    elif k in known_reads and f_kib > 0:
        ratio = known_reads[k] / (f_kib * 1024.0)
        corr = 2.0 if ratio > 1.5 else 1.0
        why = f"calibrated: reads {known_reads[k] / 2**20:.0f} MiB once, counter says {f_kib / 1024:.0f} MiB (ratio {ratio:.2f})"
    else:
        corr, why = 1.0, "uncalibrated (small kernel)"
    out[k] = {"FETCH_SIZE_KiB": f_kib, "WRITE_SIZE_KiB": w_kib, "fetch_correction": corr, "fetch_correction_basis": why,
              "hbm_side_bytes_per_launch": (f_kib * corr + w_kib) * 1024.0}
json.dump(out, open(sys.argv[3], "w"), indent=1)
for k, v in out.items():
    print(f"{k[:62]:62s} {v['hbm_side_bytes_per_launch'] / 1e9:8.3f} GB/launch  (fetch x{v['fetch_correction']:.0f}: {v['fetch_correction_basis']})")
