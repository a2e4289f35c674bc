#!/usr/bin/env python3
"""bench.py -- emulated DGEMM TFLOPS (N=8192, moduli=14) on N GPUs of one node (BASELINE.json metric).

One "step" = one whole emulated DGEMM C = A*B (8192^3, FP64 in/out, 14 moduli, INT8 MFMA backend,
accurate mode = the reference's default: 15 INT8 GEMMs) with A, B already resident in HBM.
N>1: one process per GPU over RCCL -- either started by the driver under torch.distributed.run, or by THIS file when it is called
plainly as `python bench.py --gpus N` (self_launch).  A and B are replicated on every rank; ALL THREE C++ plans behind
include/gemmul8_dist.h run in one invocation (`plans`: blocks = output blocks on a rank grid, one all_reduce(MAX) of the bounds;
moduli = moduli sharded + INT8 residue exchange; fp64sum = moduli sharded + the FP64 reduce-scatter north_star names), each with its
TFLOPS, GEMM roofline fraction, collective / exchange time and bytes; the headline `value` is the best bit-exact plan.  "strong"
scaling: the problem is fixed, value = 2*n^3 / (max over ranks of the step time).

Prints ONE JSON line (rank 0) with the driver's contract keys plus `roofline` (dominant kernel =
the batched INT8 MFMA GEMM, events recorded on the launch stream inside the timed region),
`cpu_baseline` (the CPU oracle port on a bounded sample), `host_blas_dgemm` (numpy/OpenBLAS DGEMM on
the box's cores, same shape) and `max_rel_err` (vs an 80-bit long-double product on a sampled block).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # this pool's host driver only supports dmabuf IPC (RCCL needs it)

import numpy as np
import torch


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--moduli", type=int, default=14)
    ap.add_argument("--fast", action="store_true", help="fast mode (14 GEMMs) instead of accurate (15)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baselines (profiling runs)")
    ap.add_argument("--lean", action="store_true", help="configs 3 / 5: only the configuration itself (no more_moduli / bound-mode comparison calls): "
                                                        "profiling runs, so that every launch of the dominant kernel under rocprofv3 is the workload's")
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 4, 5],
                    help="BASELINE.json config: 2 = DGEMM 8192^3 N=14 INT8 (headline, default); 3 = SGEMM 16384^3 N=6 FP8; "
                         "4 = DGEMM 16384^3 N=16 INT8 (same code path as 2 at that size; meant for --gpus 8 under torch.distributed.run); "
                         "5 = ZGEMM 8192^3 N=20 INT8 (single GPU only; extra measurement lines, not the driver's metric)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the C of the last timed step to DIR/C.npy (see dump_outputs) for output-for-output comparisons")
    return ap.parse_args()


DUMP_VALUES = 1 << 22   # per dumped array: 4 Mi float64 values = 32 MB


def dump_outputs(dirname, arrays):
    """--dump-outputs: each tensor of `arrays` (name -> column-major matrix held as a (cols, rows) tensor) as DIR/<name>.npy, float32 or
    float64, complex values as a trailing (re, im) axis.  Up to DUMP_VALUES values: the whole m x n matrix.  Larger: a fixed sample of
    DUMP_VALUES / (1 or 2) elements, 1-D, at the sorted distinct flat column-major positions np.unique(default_rng(0).integers(0, m*n, count))
    -- the same positions in every run of the same shape."""
    os.makedirs(dirname, exist_ok=True)
    for name, t in arrays.items():
        per = 2 if t.is_complex() else 1
        if t.numel() * per <= DUMP_VALUES:
            t = t.transpose(0, 1)   # (rows, cols)
        else:
            idx = np.unique(np.random.default_rng(0).integers(0, t.numel(), DUMP_VALUES // per))
            print(f"[bench] {name}.npy: {idx.size} of {t.numel()} elements, at seeded column-major positions", file=sys.stderr)
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(dirname, name + ".npy"), (torch.view_as_real(t) if t.is_complex() else t).cpu().numpy())


def make_inputs(n, device):
    """U(-0.5, 0.5) FP64, seeds 12345 (A) / 54321 (B) (testing/common.hpp:35-36), column-major."""
    gA = torch.Generator(device=device).manual_seed(12345)
    gB = torch.Generator(device=device).manual_seed(54321)
    A = torch.rand((n, n), generator=gA, dtype=torch.float64, device=device) - 0.5
    B = torch.rand((n, n), generator=gB, dtype=torch.float64, device=device) - 0.5
    return A, B  # tensor (cols, rows) == column-major matrix


def cpu_baseline_port(moduli, fast):
    """Oracle (scalar C port of the reference algorithm) on a bounded sample of the same workload: the full pipeline on a
    DGEMM 1280^3 with the same moduli and mode (~10-15 s on one core; 1/262 of the flops of the 8192^3 step)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    s = 1280
    rng = np.random.default_rng(1)
    A = rng.random((s, s)) - 0.5
    B = rng.random((s, s)) - 0.5
    t0 = time.perf_counter()
    ol.gemm(A, B, moduli, fastmode=fast)
    dt = time.perf_counter() - t0
    return {"value": 2.0 * s ** 3 / dt * 1e-12, "unit": "TFLOPS", "cores": 1, "kind": "port",
            "sample": f"oracle/oz2_oracle.c full pipeline on DGEMM {s}^3, moduli={moduli}, {dt:.2f} s"}


def host_blas(n):
    A = np.random.default_rng(12345).random((n, n)) - 0.5
    B = np.random.default_rng(54321).random((n, n)) - 0.5
    A @ B[:, :256]  # warm-up
    best = 1e30
    for _ in range(2):
        t0 = time.perf_counter()
        A @ B
        best = min(best, time.perf_counter() - t0)
    try:
        from threadpoolctl import threadpool_info
        thr = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        thr = os.cpu_count()
    return {"value": 2.0 * n ** 3 / best * 1e-12, "unit": "TFLOPS", "threads": thr, "cores": os.cpu_count(),
            "lib": "numpy-bundled OpenBLAS DGEMM", "shape": f"{n}^3", "seconds": best}


def native_fp64(A, B):
    """The reference's own comparator (testing/test_flops.hpp:87-115): the vendor's native DGEMM on the same GPU
    (rocBLAS through torch.matmul).  Yardstick only -- nothing in the product calls a BLAS."""
    n = A.shape[0]
    for _ in range(2):
        torch.matmul(B, A)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        Cn = torch.matmul(B, A)  # tensors are (cols, rows): (B^T A^T) = (A B)^T in column-major terms
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 3
    return {"value": 2.0 * n ** 3 / ms * 1e-9, "unit": "TFLOPS", "ms": ms, "lib": "rocBLAS DGEMM via torch.matmul (float64)"}, Cn


def sampled_error(A, B, C, n):
    """max |C-Chat|/|Chat| on a 48x48 sampled block, Chat = long-double (80-bit) product."""
    rows = np.arange(0, n, n // 48)[:48]
    cols = np.arange(7, n, n // 48)[:48]
    Ah = A[:, rows].cpu().numpy().T.astype(np.longdouble)   # (48, k): rows of the matrix
    Bh = B[cols, :].cpu().numpy().T.astype(np.longdouble)   # (k, 48)
    ref = Ah @ Bh
    got = C[cols][:, rows].cpu().numpy().T
    return float(np.max(np.abs((got - ref) / ref)))


def run_other_config(args):
    """Configs 3 and 5 of BASELINE.json on one GPU: whole-call timing through gemmul8_gemm (events), accuracy on a sampled block."""
    import gemmul8_amd as g
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.config == 3:
        n, N, dt, be, name, cflops = 16384, 6, torch.float32, g.FP8, "SGEMM", 1
    else:
        n, N, dt, be, name, cflops = 8192, 20, torch.complex128, g.INT8, "ZGEMM", 4
    if args.size != 8192:
        n = args.size
    gen = torch.Generator(device=dev).manual_seed(12345)
    rdt = torch.float32 if dt == torch.float32 else torch.float64
    def rnd():
        x = torch.rand((n, n), generator=gen, dtype=rdt, device=dev) - 0.5
        if dt.is_complex:
            x = torch.complex(x, torch.rand((n, n), generator=gen, dtype=rdt, device=dev) - 0.5)
        return x.contiguous()
    A, B = rnd(), rnd()
    Cm = torch.zeros((n, n), dtype=dt, device=dev)
    tot, _, _ = g.work_size(dt.is_complex, be, n, n, n, N)
    work = torch.empty(tot, dtype=torch.uint8, device=dev)
    mode = bool(args.fast)
    for _ in range(args.warmup):
        g.gemm(A, B, N, fastmode=mode, backend=be, C_out=Cm, work=work)
    torch.cuda.synchronize()
    ts, phases = [], np.zeros(4)
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.gemm(A, B, N, fastmode=mode, backend=be, C_out=Cm, work=work)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    C_timed = Cm.clone() if args.dump_outputs else None   # the comparison calls below overwrite Cm
    _, tm, _ = g.gemm(A, B, N, fastmode=mode, backend=be, C_out=Cm, work=work, timers=True)
    ms = float(np.median(ts))
    rows = np.arange(0, n, n // 32)[:32]
    cols = np.arange(7, n, n // 32)[:32]
    hp = np.clongdouble if dt.is_complex else np.longdouble
    Ah = A[:, rows].cpu().numpy().T.astype(hp)
    Bh = B[cols, :].cpu().numpy().T.astype(hp)
    ref = Ah @ Bh
    got = Cm[cols][:, rows].cpu().numpy().T
    err = float(np.max(np.abs(got - ref) / np.abs(ref)))
    # the reference's comparator (testing/test_accuracy.hpp): the vendor's native GEMM of the same type, same metric
    torch.matmul(B, A)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    Cn = torch.matmul(B, A)
    e1.record()
    torch.cuda.synchronize()
    nat_ms = e0.elapsed_time(e1)
    gotn = Cn[cols][:, rows].cpu().numpy().T
    errn = float(np.max(np.abs(gotn - ref) / np.abs(ref)))
    del Cn
    gcnt = {3: 3 * N + (0 if mode else 1), 5: 3 * N + (0 if mode else 5)}[args.config]  # complex bounds: K-concatenated 2+3 units
    # FP8 backend: the residue GEMMs multiply the backend's integer pieces (|v| <= 16) as FP6 e2m3 codes (csrc/oz2_gemm_f6.hip: same values, same
    # bits out, CDNA4 runs FP6 at the FP4 rate) unless GEMMUL8_FP8_PLANES=e4m3 keeps the e4m3 planes -- the roofline is priced against the format used
    f6 = be == g.FP8 and os.environ.get("GEMMUL8_FP8_PLANES", "fp6")[:1] != "e"
    lp_peak = 10000.0 if f6 else 5000.0  # dense MFMA peak of the operand format, TOP/s (MI355X_MICROARCH.md: FP6/FP4 ~10 PF, FP8/INT8 ~5 PF)
    lp_dtype = ("fp6 e2m3 MFMA on the FP8 backend's integer pieces (exact; f32 accumulate) + e4m3 bound GEMM + f64 CRT" if f6 else
                "fp8 e4m3 MFMA (f32 accumulate) + f64 CRT" if be == g.FP8 else "int8 MFMA (i32 accumulate) + f64 CRT")
    out = {"metric": f"emulated {name} TFLOPS (config {args.config})", "value": cflops * 2.0 * n ** 3 / ms * 1e-9, "unit": "TFLOPS",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": lp_dtype,
           "data": "synthetic U(-0.5,0.5)", "config": {"workload": f"{name} {n}^3, moduli={N}, {'FP8' if be == g.FP8 else 'INT8'} backend, "
                                                                      f"{'fast' if mode else 'accurate'} mode, op N/N, alpha=1, beta=0"},
           "phase_ms": {"scaling": tm[0] * 1e-6, "lowprec_gemm": tm[1] * 1e-6, "requantise": tm[2] * 1e-6, "inverse_scaling": tm[3] * 1e-6},
           "roofline": {"bound": "mfma", "kernel": "the residue GEMMs of the low-precision phase (3 per modulus; the accurate mode's bound GEMMs "
                                                       "run inside the scaling phase and are not counted here)",
                        "achieved": (3 * N) * 2.0 * n ** 3 / (tm[1] * 1e-6) * 1e-9, "peak": lp_peak,
                        "frac": (3 * N) * 2.0 * n ** 3 / (tm[1] * 1e-6) * 1e-9 / lp_peak, "traffic": None, "traffic_measured_in_run": False,
                        "sustained_mfma_on_backend_data_TOPs": 6816.0 if f6 else 4487.0 if be == g.FP8 else 3969.0,
                        "unit": "TOP/s", "lowprec_units_of_2mnk_whole_call": gcnt, "lowprec_phase_ms": tm[1] * 1e-6},
           "max_rel_err": err,
           "native_same_gpu": {"lib": f"rocBLAS/hipBLASLt {name} via torch.matmul", "value": cflops * 2.0 * n ** 3 / nat_ms * 1e-9,
                               "unit": "TFLOPS", "ms": nat_ms, "max_rel_err": errn}}
    if args.config == 3 and n == 16384 and N == 6 and f6 and not mode:
        # fabric-side bytes of ONE launch of the dominant kernel (the 6-moduli gemm_f6_kernel<7>), from the committed PMC passes named in profiles/MANIFEST.json
        # (FETCH_SIZE x 2 + WRITE_SIZE, separate --pmc passes of `bench.py --config 3 --lean`); algorithmic bytes = 2 x 12 plane images + 6 int16 residue planes
        tr = traffic_manifest_entry(n, N, "sgemm_16384_moduli6_fp8")
        if tr:
            out["roofline"]["traffic"] = tr["hbm_side_bytes_per_launch"]
            out["roofline"]["traffic_source"] = tr["source"]
            out["roofline"]["traffic_kernel"] = tr["kernel"]
            out["roofline"]["algorithmic_bytes_per_launch"] = 2 * 12 * n * n * 0.75 + 6 * n * n * 2.0
    if args.config == 3 and not args.lean:
        # the accuracy axis: 6 moduli (BASELINE's count) leave the emulated SGEMM ~9x less accurate than the native one on this sampled block; the same call
        # with 7 / 8 moduli (the reference sweeps up to 12 for S: testing/common.hpp:38-43), timed the same way, beside it
        more = []
        for N2 in (7, 8):
            tot2, _, _ = g.work_size(False, be, n, n, n, N2)
            work2 = torch.empty(tot2, dtype=torch.uint8, device=dev)
            g.gemm(A, B, N2, fastmode=mode, backend=be, C_out=Cm, work=work2)
            torch.cuda.synchronize()
            t2 = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.gemm(A, B, N2, fastmode=mode, backend=be, C_out=Cm, work=work2)
                e1.record()
                torch.cuda.synchronize()
                t2.append(e0.elapsed_time(e1))
            got2 = Cm[cols][:, rows].cpu().numpy().T
            more.append({"num_moduli": N2, "value": 2.0 * n ** 3 / float(np.median(t2)) * 1e-9, "unit": "TFLOPS", "ms": float(np.median(t2)),
                         "max_rel_err": float(np.max(np.abs(got2 - ref) / np.abs(ref)))})
            del work2
        out["more_moduli"] = more
    if be == g.FP8 and not mode and not args.lean:
        # how far is the default (engine-safe) FP8 accurate-mode bound from the reference's formula (k+1)*2^-24
        # (src/find_max.hpp:82-96) on THESE inputs?  Same call in both modes: rows / columns whose shift differs, elements of C that differ.
        import ctypes as C_
        L = g.Layout()
        g.check(g.lib().gemmul8_get_layout(g._dtype_code(dt), be, n, n, n, N, work.data_ptr(), None, None, 0, 0, C_.byref(L)))
        base = work.data_ptr()
        def shifts():
            a0, b0 = L.sftA - base, L.sftB - base
            return work[a0:a0 + 2 * n].view(torch.int16).clone(), work[b0:b0 + 2 * n].view(torch.int16).clone()
        prev = g.lib().gemmul8_set_fp8_bound_mode(0)
        g.gemm(A, B, N, fastmode=False, backend=be, C_out=Cm, work=work)
        torch.cuda.synchronize()
        sA0, sB0 = shifts()
        C0 = Cm.clone()
        g.lib().gemmul8_set_fp8_bound_mode(1)
        g.gemm(A, B, N, fastmode=False, backend=be, C_out=Cm, work=work)
        torch.cuda.synchronize()
        sA1, sB1 = shifts()
        g.lib().gemmul8_set_fp8_bound_mode(prev)
        dA_, dB_ = (sA0 != sA1), (sB0 != sB1)
        out["fp8_bound_mode"] = {"default": "engine-safe inflation 7*2^-13 + 4(k+1)*2^-24 + 7 kp 2^-14 (mode 0)" if prev == 0 else f"mode {prev}",
                                 "reference_formula": "(k+1)*2^-24 (src/find_max.hpp:82-96; mode 1, GEMMUL8_FP8_BOUND=reference)",
                                 "rows_with_a_different_shift": int(dA_.sum()), "cols_with_a_different_shift": int(dB_.sum()), "of": n,
                                 "max_abs_shift_diff": int(max((sA0 - sA1).abs().max().item(), (sB0 - sB1).abs().max().item())),
                                 "elements_of_C_that_differ": int((C0 != Cm).sum().item()), "elements": n * n,
                                 "max_rel_diff_of_C_between_modes": float(((C0 - Cm).abs() / C0.abs().clamp_min(1e-30)).max().item())}
        del C0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"C": C_timed})
    print(json.dumps(out))


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start N ranks of this file under torch.distributed.run on a free
    port of 127.0.0.1 and relay their output / exit status.  With fewer than N visible GPUs (a single-GPU test box) the ranks share the
    GPUs through the host-staged gloo TEST transport (GEMMUL8_DIST_BACKEND=gloo); the JSON line says which transport ran."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    ngpu = torch.cuda.device_count()
    if ngpu < args.gpus and "GEMMUL8_DIST_BACKEND" not in env:
        env["GEMMUL8_DIST_BACKEND"] = "gloo"
        print(f"[bench] {ngpu} GPU(s) visible for --gpus {args.gpus}: the ranks share them over the gloo test transport", file=sys.stderr)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def traffic_manifest_entry(n, N, workload=None):
    """profiles/MANIFEST.json -> the committed PMC traffic record of the dominant kernel of a workload (default: DGEMM n^3 with N moduli, INT8);
    None if the manifest has no entry for it, or the file / kernel it names is missing."""
    try:
        man = json.load(open(os.path.join(ROOT, "profiles", "MANIFEST.json")))
        ent = man["workloads"][workload or f"dgemm_{n}_moduli{N}_int8"]
        recs = json.load(open(os.path.join(ROOT, "profiles", ent["pmc_traffic"])))
        rec = recs[ent["kernel"]]
        return {"hbm_side_bytes_per_launch": rec["hbm_side_bytes_per_launch"], "source": "profiles/" + ent["pmc_traffic"], "kernel": ent["kernel"]}
    except (OSError, KeyError, ValueError):
        return None


def smi_sampler():
    """Background sampling of sclk / socket power with rocm-smi (best effort: returns (stop, samples) -- samples stays empty where
    rocm-smi is missing or prints another format)."""
    import re
    import subprocess
    import threading
    samples, flag = [], {"stop": False}

    def run():
        while not flag["stop"]:
            try:
                o = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=10).stdout
                m1 = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", o)
                m2 = re.search(r"Power \(W\): ([0-9.]+)", o)
                if m1 and m2:
                    samples.append((int(m1.group(1)), float(m2.group(1))))
            except Exception:
                return
    th = threading.Thread(target=run, daemon=True)
    th.start()

    def stop():
        flag["stop"] = True
        th.join(timeout=15)
    return stop, samples


def event_pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def single_gpu_phases(args, n, N, A, B, dev, stream):
    """Phase times of the single-GPU call (bounds | quantise | INT8 GEMMs | CRT, ms; events on the launch stream, mean of 3 calls after one
    warm-up): the inputs of plan_model."""
    import ctypes as C
    import gemmul8_amd as g
    lib = g.lib()
    Cmat = torch.zeros((n, n), dtype=torch.float64, device=dev)
    one, zero = np.array([1.0]), np.array([0.0])
    tot, _, _ = g.work_size(False, g.INT8, n, n, n, N)
    work = torch.empty(tot, dtype=torch.uint8, device=dev)
    L = g.Layout()
    g.check(lib.gemmul8_get_layout(g.D, g.INT8, n, n, n, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    st = stream.cuda_stream
    acc = np.zeros(4)
    for it in range(4):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record(stream)
        if not args.fast:
            g.check(lib.gemmul8_scale_bounds(st, g.D, g.INT8, 0, 0, n, n, n, A.data_ptr(), n, B.data_ptr(), n, N, 0, n, C.byref(L), 0, 0))
        ev[1].record(stream)
        g.check(lib.gemmul8_scale_finish(st, g.D, g.INT8, 0, 0, n, n, n, A.data_ptr(), n, B.data_ptr(), n, N, int(args.fast), 0, N, C.byref(L), 0, 0))
        ev[2].record(stream)
        g.check(lib.gemmul8_lowprec_gemm(st, g.D, g.INT8, n, n, n, N, 0, N, C.byref(L)))
        ev[3].record(stream)
        g.check(lib.gemmul8_crt(st, g.D, g.INT8, N, n, n, L.C_mid, L.mp, L.sizeC, L.sftA, L.sftB, one.ctypes.data, zero.ctypes.data, Cmat.data_ptr(), n))
        ev[4].record(stream)
        torch.cuda.synchronize()
        if it:
            acc += np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(4)])
    ph = dict(zip(("bounds", "quantise", "lowprec_gemm", "crt"), (acc / 3).tolist()))
    # The persistent residue GEMM holds every CU it runs on: an RCCL point-to-point / reduce-scatter kernel on the plan's exchange stream only overlaps
    # on CUs the GEMM gives up (GEMMUL8_GEMM_CUS, csrc/oz2_knobs.hpp).  What giving up 8 / 16 CUs COSTS the GEMM is measurable on one GPU, today:
    # the same launch on 256 / 248 / 240 CUs (mean of 3), so that the first multi-GPU run can choose its exchange schedule against measured numbers.
    by_cus = {}
    try:
        for cus in (0, 248, 240):
            if cus:
                os.environ["GEMMUL8_GEMM_CUS"] = str(cus)
            else:
                os.environ.pop("GEMMUL8_GEMM_CUS", None)
            lib.gemmul8_reload_knobs()
            ts = []
            for it in range(4):
                e0, e1 = event_pair()
                e0.record(stream)
                g.check(lib.gemmul8_lowprec_gemm(st, g.D, g.INT8, n, n, n, N, 0, N, C.byref(L)))
                e1.record(stream)
                torch.cuda.synchronize()
                if it:
                    ts.append(e0.elapsed_time(e1))
            by_cus[str(cus or 256)] = float(np.mean(ts))
    finally:
        os.environ.pop("GEMMUL8_GEMM_CUS", None)
        lib.gemmul8_reload_knobs()
    ph["lowprec_gemm_by_cus"] = by_cus
    del work, Cmat
    return ph


def plan_model(name, world, N, n, ph, grid):
    """DESIGN.md 5's per-rank time model of a plan, from the single-GPU phase times `ph` measured in this run -- so that the first curve
    measured on an 8-GPU node can be held against a prediction made before it existed.  Assumptions (all stated in the JSON):
      * every kernel scales with the share of rows / columns / moduli a rank works on (no efficiency loss on smaller problems);
      * bounds phase = 30 % A side (amax + extract), 17 % B side (extract), 53 % bound GEMM; quantise = 52 % A, 48 % B;
      * moduli plan: the residue exchange of the first of two plane groups overlaps the second group's GEMMs (the A-side extract of the bounds
        phase is still replicated on every rank: 0.30 b);
      * an all-reduce(MAX) of 4 (m + n) bytes: 0.05 ms; point-to-point: every xGMI peer link carries 45 GB/s per direction, all peers at
        once; reduce-scatter of FP64 partials: ring over min(G - 1, 7) links in parallel at the same rate."""
    G = world
    gr, gc = grid
    b, q, gm, cr = ph["bounds"], ph["quantise"], ph["lowprec_gemm"], ph["crt"]
    link = 45e9
    ar = 0.05 if (b > 0 and G > 1) else 0.0
    mr = -(-N // G)  # moduli of the busiest rank
    if name == "blocks":
        terms = {"bounds": b * (0.30 / gr + 0.17 / gc + 0.53 / G), "quantise": q * (0.52 / gr + 0.48 / gc), "lowprec_gemm": gm / G, "crt": cr / G,
                 "allreduce": ar, "exchange": 0.0}
    elif name == "moduli":
        out_bytes = (G - 1) / G * mr * n * n                    # INT8 residue blocks this rank sends; (G - 1) peers in parallel
        # round 5: the rank's planes go out in two groups, the exchange of the first group travels beside the GEMMs of the second (csrc/oz2_dist.cpp):
        # only what the exchange takes beyond half of the GEMM time is exposed, plus the second group's own exchange (half of the bytes)
        gm_r = gm * mr / N
        ex = (out_bytes / max(1, G - 1)) / link * 1e3 if G > 1 else 0.0
        ex_exposed = (max(0.0, ex / 2 - gm_r / 2) + ex / 2) if mr >= 2 else ex
        terms = {"bounds": b * (0.30 + 0.17 / G + 0.53 / G), "quantise": q * mr / N, "lowprec_gemm": gm_r, "crt": cr / G, "allreduce": ar,
                 "exchange": ex_exposed}
    else:  # fp64sum
        part_bytes = (mr + 16.0) * n * n                        # partial CRT: read mr residue planes, write two double planes
        rs_bytes = (G - 1) / G * 16.0 * n * n
        terms = {"bounds": b * (0.30 + 0.17 / G + 0.53 / G), "quantise": q * mr / N, "lowprec_gemm": gm * mr / N,
                 "crt": part_bytes / 5.0e12 * 1e3 + cr / G * 0.5, "allreduce": ar,
                 "exchange": rs_bytes / (link * max(1, min(G - 1, 7))) * 1e3 if G > 1 else 0.0}
    out = {"model_ms": float(sum(terms.values())), "model_terms_ms": {k_: float(v) for k_, v in terms.items()}}
    # the same model if the GEMM leaves 8 / 16 CUs to the exchange kernels (measured single-GPU GEMM cost on 248 / 240 CUs, same run) and the
    # exchange then overlaps completely (moduli plan) -- the other corner of the trade; the truth of an 8-GPU node lies between the two
    by = ph.get("lowprec_gemm_by_cus") or {}
    if name == "moduli" and G > 1 and by.get("256"):
        alt = {}
        for cus in ("248", "240"):
            if by.get(cus):
                t = dict(terms)
                t["lowprec_gemm"] = terms["lowprec_gemm"] * by[cus] / by["256"]
                t["exchange"] = (out_bytes / max(1, G - 1)) / link * 1e3 / 2 if mr >= 2 else terms["exchange"]   # only the last group's exchange stays exposed
                alt[cus] = float(sum(t.values()))
        out["model_ms_if_gemm_leaves_cus"] = alt
    return out


def run_plans(args, n, N, A, B, dev, stream, backend, rank, world):
    """N > 1: every plan of include/gemmul8_dist.h in ONE invocation (blocks, moduli, fp64sum), each with `warmup` untimed and `steps`
    timed calls bracketed by barrier + synchronize, max over ranks.  Returns (records by plan name, gathered C of the headline plan,
    description of the transport)."""
    import torch.distributed as dist
    import gemmul8_amd as g
    from gemmul8_amd import dist as gd
    peak = 5000.0
    # First contact with the transport, before anything is timed (GEMMUL8_DIST_SELFTEST=0 skips it): communicator size, all-reduce(MAX),
    # grouped send/recv ring, reduce-scatter(sum) against host arithmetic.  Order of choice on the nccl backend: the library's own RCCL
    # communicator (RcclComm, the product path); if it cannot be created or fails the self-test on ANY rank, every rank falls back to
    # torch's nccl (= RCCL) process group on the same device buffers (TorchNcclTransport; GEMMUL8_DIST_BACKEND=torch-nccl forces it) and
    # the JSON says so -- a first multi-GPU lease then still returns a measured line.  A transport that fails there too ends the run
    # with ONE line that says which check failed.
    want_test = os.environ.get("GEMMUL8_DIST_SELFTEST", "1") != "0"

    def agree(bad):
        flag = torch.tensor([1 if bad else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        return int(flag.item()) != 0

    def bring_up(make, expect_rccl):
        comm, ok, msg = None, True, "skipped"
        try:
            comm = make()
            if want_test:
                ok, msg = gd.selftest(comm, dev, stream.cuda_stream, expect_rccl=expect_rccl)
        except Exception as e:
            ok, msg = False, f"rank {rank}: {type(e).__name__}: {e}"
        if not ok:
            print(f"[bench] DIST SELFTEST FAILED: {msg}", file=sys.stderr, flush=True)
        if agree(not ok):
            if comm is not None:
                comm.close()
            return None, msg if not ok else "failed on another rank (see stderr)"
        return comm, msg

    fallback_reason = None
    comm, msg = (None, None)
    if backend == "nccl":
        def first_choice():
            if os.environ.get("GEMMUL8_BENCH_FAIL_FIRST_TRANSPORT", "0") == "1":   # test knob: exercise the fall-back (tests/test_gpu_dist.py)
                raise RuntimeError("GEMMUL8_BENCH_FAIL_FIRST_TRANSPORT=1")
            return gd.RcclComm()
        comm, msg = bring_up(first_choice, True)
        if comm is None:
            fallback_reason = msg
            backend = "torch-nccl"
            if rank == 0:
                print("[bench] the library's own RCCL communicator is not usable here; falling back to torch's nccl process group", file=sys.stderr, flush=True)
    if comm is None:
        comm, msg = bring_up(gd.TorchNcclTransport if backend == "torch-nccl" else (lambda: gd.TorchTransport(device=True)), False)
    if comm is None:
        if rank == 0:
            print(json.dumps({"metric": f"emulated DGEMM TFLOPS (N={n}, moduli={N})", "value": None, "n_gpus": world, "error": "dist selftest failed",
                              "dist_selftest": msg, "first_choice_failure": fallback_reason}))
        dist.barrier()
        dist.destroy_process_group()
        sys.exit(3)
    rccl_ranks = comm.rccl_ranks()
    checked = "all-reduce(MAX,int32), grouped send/recv ring, reduce-scatter(sum,f64) checked against host arithmetic"
    selftest = "skipped" if not want_test else {"nccl": "ok: ncclCommCount, " + checked, "torch-nccl": "ok (torch's nccl process group): " + checked}.get(
        backend, "ok (gloo test transport): " + checked)
    # single-GPU phase times on rank 0 (the other ranks wait): the inputs of the per-plan time model in the JSON
    phases = None
    if rank == 0:
        phases = single_gpu_phases(args, n, N, A, B, dev, stream)
    dist.barrier()

    def barrier():
        dist.barrier()
        torch.cuda.synchronize()

    def ev_ms(pairs):
        v = [a.elapsed_time(b) for a, b in pairs]
        return float(np.mean(v)) if v else None

    results, gathered = {}, {}
    Cmat = torch.zeros((n, n), dtype=torch.float64, device=dev)
    for name in ("blocks", "moduli", "fp64sum"):
        plan = gd.make_plan(comm, g.D, g.INT8, n, n, n, N, mode=name, fastmode=args.fast)
        gemm_ev, ar_ev, xc_ev = [], [], []

        def step(record):
            if record:
                e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                for x in e:
                    x.record(stream)   # creates the handles; the plan re-records the ones its path reaches
                plan.set_events(e[0], e[1])
                plan.set_exchange_events(e[2:6])
                plan.run(A, B, Cmat)
                gemm_ev.append((e[0], e[1]))
                ar_ev.append((e[2], e[3]))
                xc_ev.append((e[4], e[5]))
            else:
                plan.set_events(None, None)
                plan.set_exchange_events(None)
                plan.run(A, B, Cmat)
        Cmat.zero_()
        for _ in range(args.warmup):
            step(False)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(True)
        barrier()
        dt = time.perf_counter() - t0
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        ar_bytes, sent, recvd = plan.exchange_bytes()
        has_ar = ar_bytes > 0
        has_xc = name != "blocks"
        gemm_ms = ev_ms(gemm_ev)
        ops = plan.my_planes * 2.0 * plan.work_rows * plan.work_cols * n    # this rank's share of the low-precision GEMMs
        ach = ops / (gemm_ms * 1e-3) * 1e-12 if gemm_ms else None
        ms = dt / args.steps * 1e3
        rec = {"value": 2.0 * n ** 3 / (ms * 1e-3) * 1e-12, "unit": "TFLOPS", "ms_per_step": ms, "parallelism": plan.describe(),
               "gemm_launch_ms_rank0": gemm_ms, "gemm_ops_rank0": ops, "gemm_achieved_TOPs_rank0": ach, "gemm_frac_of_int8_peak_rank0": ach / peak if ach else None,
               "bounds_allreduce_ms_rank0": ev_ms(ar_ev) if has_ar else 0.0, "exchange_ms_rank0": ev_ms(xc_ev) if has_xc else 0.0,
               # the moduli plan's exchange runs beside the later groups' GEMMs: exchange_ms spans GEMM time; what the step actually waits for is the
               # part behind the last GEMM (include/gemmul8_dist.h, gemmul8_dist_set_exchange_events)
               "exchange_exposed_ms_rank0": max(0.0, ev_ms([(g_[1], x_[1]) for g_, x_ in zip(gemm_ev, xc_ev)])) if has_xc else 0.0,
               "allreduce_bytes": ar_bytes, "bytes_sent_rank0": sent, "bytes_received_rank0": recvd,
               "workspace_bytes_rank0": plan.workspace_bytes()}
        full = plan.gather_result(Cmat)
        torch.cuda.synchronize()
        if rank == 0:
            gathered[name] = full.clone()
            rec["max_rel_err"] = sampled_error(A, B, full, n)
            gr = max(1, round(n / max(1, plan.work_rows))) if name == "blocks" else 1   # rank 0 owns the first row block of the Gr x Gc grid
            rec.update(plan_model(name, world, N, n, phases, (gr, max(1, world // gr))))
        results[name] = rec
        plan.close()
        barrier()
    transport = {"nccl": "RCCL (ncclCommInitRank inside libgemmul8.so)",
                 "torch-nccl": "RCCL through torch.distributed's nccl process group, device buffers (second choice: see first_choice_failure)"}.get(
        backend, f"gloo TEST transport, host-staged ({world} ranks on {torch.cuda.device_count()} GPU(s))")
    info = {"transport": transport, "first_choice_failure": fallback_reason,
            "rccl_ranks": rccl_ranks, "dist_selftest": selftest, "single_gpu_phase_ms": phases,
            "model_assumptions": "plans[*].model_ms = DESIGN.md 5's per-rank model from single_gpu_phase_ms: kernels scale with the rank's share; bounds = 30 % A side + 17 % B "
                                 "side + 53 % bound GEMM; quantise 52 % A / 48 % B; all-reduce(MAX) 0.05 ms; 45 GB/s per xGMI peer link and direction, all peers at once; "
                                 "FP64 reduce-scatter as a ring over min(G-1, 7) links"}
    headline = None
    if rank == 0:
        ref = gathered["moduli"]
        results["blocks"]["mismatches_vs_moduli"] = int((gathered["blocks"] != ref).sum().item())
        results["moduli"]["mismatches_vs_moduli"] = 0
        results["fp64sum"]["mismatches_vs_moduli"] = int((gathered["fp64sum"] != ref).sum().item())
        results["fp64sum"]["elements"] = int(ref.numel())
        exact = [k_ for k_ in ("blocks", "moduli") if results[k_]["mismatches_vs_moduli"] == 0]
        headline = max(exact, key=lambda k_: results[k_]["value"])
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"C": gathered[headline]})
    comm.close()
    return results, headline, info


def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(self_launch(args))
    if env_world is not None and int(env_world) != args.gpus and os.environ.get("GEMMUL8_BENCH_FORCE_PLAN", "0") != "1":
        print(f"bench.py: --gpus {args.gpus} disagrees with WORLD_SIZE={env_world} (launch one rank per GPU, or call plain "
              f"`python bench.py --gpus N` and let this file start the ranks)", file=sys.stderr)
        sys.exit(2)
    if args.config == 4:
        args.size, args.moduli = 16384, 16
    elif args.config != 2:
        return run_other_config(args)
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("GEMMUL8_DIST_BACKEND", "nccl") not in ("nccl", "torch-nccl"):
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # GEMMUL8_BENCH_FORCE_PLAN=1: take the multi-GPU code path (process group, plans, barrier, max-over-ranks timing, gather) even
    # with ONE rank, so that it can be exercised on the real RCCL backend of a single-GPU box (tests/test_gpu_dist.py)
    multi = world > 1 or os.environ.get("GEMMUL8_BENCH_FORCE_PLAN", "0") == "1"
    backend = os.environ.get("GEMMUL8_DIST_BACKEND", "nccl")
    if multi:
        import torch.distributed as dist
        # RCCL ("nccl") is the product path; GEMMUL8_DIST_BACKEND=gloo only exists to smoke-test this file with
        # several ranks sharing one GPU (host-staged exchange), where NCCL refuses duplicate devices.
        # GEMMUL8_DIST_BACKEND=torch-nccl: the same nccl process group, the plans' exchanges through it instead of the library's
        # own communicator (run_plans' second choice, forced).
        if backend in ("nccl", "torch-nccl"):
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    import ctypes as C
    import gemmul8_amd as g

    n, N = args.size, args.moduli
    A, B = make_inputs(n, dev)
    lib = g.lib()
    stream = torch.cuda.current_stream(dev)
    flops = 2.0 * n ** 3
    peak = 5000.0  # dense INT8 MFMA TOPS (MI355X_MICROARCH.md: ~5 PF-class dense FP8/INT8)
    workload = (f"DGEMM {n}x{n}x{n}, moduli={N}, INT8 backend, {'fast' if args.fast else 'accurate'} mode "
                f"({N + (0 if args.fast else 1)} INT8 GEMMs), op N/N, alpha=1, beta=0, inputs resident in HBM")

    if multi:
        import torch.distributed as dist
        results, headline, info = run_plans(args, n, N, A, B, dev, stream, backend, rank, world)
        if rank == 0:
            h = results[headline]
            out = {
                "metric": f"emulated DGEMM TFLOPS (N={n}, moduli={N})", "value": h["value"], "unit": "TFLOPS", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": h["ms_per_step"], "higher_is_better": True, "scaling": "strong",
                "vs_baseline": None, "dtype": "int8", "dtype_detail": "int8 MFMA (i32 accumulate) + f64 CRT",
                "data": "synthetic U(-0.5,0.5), seeds 12345/54321",
                "config": {"workload": workload, "parallelism": h["parallelism"], "headline_plan": headline,
                           "placement": "A, B replicated on every rank; C full-size on every rank, each rank updates the block it owns"},
                "roofline": {"bound": "mfma", "kernel": "oz2::gemm_i8_kernel<EPI_MOD> (this rank's share, batched over its moduli)",
                             "achieved": h["gemm_achieved_TOPs_rank0"], "peak": peak, "unit": "TOP/s", "frac": h["gemm_frac_of_int8_peak_rank0"],
                             "traffic": None, "traffic_measured_in_run": False, "launch_ms": h["gemm_launch_ms_rank0"],
                             "ops_per_launch": h["gemm_ops_rank0"]},
                "plans": results, "max_rel_err": h["max_rel_err"],
                "headline_rule": "best of the plans that are bit-identical to each other (blocks, moduli); fp64sum is reported with its mismatch count",
            }
            out.update(info)
            print(json.dumps(out))
        dist.barrier()
        dist.destroy_process_group()
        return

    # ---------------------------------------------------------------- one GPU
    Cmat = torch.zeros((n, n), dtype=torch.float64, device=dev)
    one = np.array([1.0])
    zero = np.array([0.0])
    tot, _, _ = g.work_size(False, g.INT8, n, n, n, N)
    work = torch.empty(tot, dtype=torch.uint8, device=dev)
    L = g.Layout()
    g.check(lib.gemmul8_get_layout(g.D, g.INT8, n, n, n, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    phase_events = []

    def step(record):
        st = stream.cuda_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if record else None
        if record:
            ev[4].record(stream)   # start of the call
        if not args.fast:
            g.check(lib.gemmul8_scale_bounds(st, g.D, g.INT8, 0, 0, n, n, n, A.data_ptr(), n, B.data_ptr(), n, N, 0, n, C.byref(L), 0, 0))
        if record:
            ev[0].record(stream)
        g.check(lib.gemmul8_scale_finish(st, g.D, g.INT8, 0, 0, n, n, n, A.data_ptr(), n, B.data_ptr(), n, N, int(args.fast), 0, N,
                                         C.byref(L), 0, 0))
        if record:
            ev[1].record(stream)
        g.check(lib.gemmul8_lowprec_gemm(st, g.D, g.INT8, n, n, n, N, 0, N, C.byref(L)))
        if record:
            ev[2].record(stream)
        g.check(lib.gemmul8_crt(st, g.D, g.INT8, N, n, n, L.C_mid, L.mp, L.sizeC, L.sftA, L.sftB, one.ctypes.data,
                                zero.ctypes.data, Cmat.data_ptr(), n))
        if record:
            ev[3].record(stream)
            phase_events.append(ev)

    # the native comparator first (its own warm-up + 3 timed calls): the emulated steps then start on a device that is already out
    # of its idle power state, like every call of a running application (the first launches after idle run 5-20 % slow)
    nat, Cn = native_fp64(A, B)   # (its error check is host work: after the timed region, so that the device does not idle here)

    for _ in range(args.warmup):
        step(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0

    # the other mode alongside (report both; the headline above is the mode selected by --fast), timed HERE, on the device the
    # headline left warm -- behind the host-side error checks below its first launches ran on a device back in its idle power state
    # (6.7 / 6.2 / 5.7 ms for the same GEMM launch: profiles/archive/r04b_config2_kernel_stats_note.txt) and the fast-mode line read 169 where the sweeps read 175
    C_head = Cmat.clone()
    other = not args.fast
    for _ in range(2):
        g.gemm(A, B, N, fastmode=other, C_out=Cmat, work=work)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(5):
        g.gemm(A, B, N, fastmode=other, C_out=Cmat, work=work)
    torch.cuda.synchronize()
    oms = (time.perf_counter() - t1) / 5 * 1e3
    C_other = Cmat

    # Settled figure: the timed region above is 0.1-0.2 s on a device that has been busy for about a second.  Here
    # the SAME step first runs for >= 2 s with the host idle (nothing but this launch loop), then 30 calls are timed one by one with
    # events (the reference's protocol: testing/test_flops.hpp:169-206, median of per-call timings); sclk / socket power are sampled
    # with rocm-smi during the pre-heat.  Reported beside `value`, never instead of it.
    n_timed_events = len(phase_events)
    stop_smi, smi = smi_sampler()
    t_heat = time.perf_counter()
    heat_calls = 0
    while time.perf_counter() - t_heat < 2.0:
        for _ in range(20):
            step(False)
        torch.cuda.synchronize()
        heat_calls += 20
    stop_smi()
    settled_ev = []
    for _ in range(30):
        e0, e1 = event_pair()
        e0.record(stream)
        step(False)
        e1.record(stream)
        settled_ev.append((e0, e1))
    torch.cuda.synchronize()
    settled_ms = float(np.median([a.elapsed_time(b) for a, b in settled_ev]))
    busy = [s_ for s_ in smi if s_[1] > 600]

    ms = dt / args.steps * 1e3
    value = flops / (ms * 1e-3) * 1e-12
    assert len(phase_events) == n_timed_events == args.steps
    gemm_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in phase_events]))
    call_ms = sorted(e[4].elapsed_time(e[3]) for e in phase_events)
    med_ms = float(call_ms[len(call_ms) // 2] if len(call_ms) % 2 else 0.5 * (call_ms[len(call_ms) // 2 - 1] + call_ms[len(call_ms) // 2]))
    ops = N * flops
    ach = ops / (gemm_ms * 1e-3) * 1e-12
    roof = {"bound": "mfma", "kernel": "oz2::gemm_i8_kernel<EPI_MOD> (batched over moduli)", "achieved": ach, "peak": peak,
            "unit": "TOP/s", "frac": ach / peak, "traffic": None, "traffic_measured_in_run": False, "launch_ms": gemm_ms, "ops_per_launch": ops,
            "algorithmic_bytes_per_launch": N * 3.0 * n * n,
            # measured with tools/ubench/mfma_shapes.hip (profiles/archive/r02_mfma_shapes.txt): a register-only loop of the kernel's
            # instruction (v_mfma_i32_16x16x64_i8) reaches the nominal peak on all-zero operands but is limited by the 1400 W
            # socket cap to this on uniformly distributed residues (v_mfma_i32_32x32x32_i8: 3448)
            "sustained_mfma_on_residue_data_TOPs": 3969.0}
    # HBM-side bytes per launch of this kernel from the committed rocprofv3 PMC passes (FETCH_SIZE x2 on gfx950 +
    # WRITE_SIZE, tools/pmc_traffic.py) -- a committed constant of the profiled configuration, NOT measured in this run.  The file is
    # NAMED in profiles/MANIFEST.json (key "pmc_traffic" of the workload's entry), together with the kernel it was taken from: a stale or
    # missing entry yields traffic = null, never a silently outdated number.
    man = traffic_manifest_entry(n, N)
    if man:
        roof["traffic"] = man["hbm_side_bytes_per_launch"]
        roof["traffic_source"] = man["source"]
        print(f"[bench] roofline.traffic from {man['source']} ({man['kernel']})", file=sys.stderr)
    out = {
        "metric": f"emulated DGEMM TFLOPS (N={n}, moduli={N})", "value": value, "unit": "TFLOPS", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "int8", "dtype_detail": "int8 MFMA (i32 accumulate) + f64 CRT", "data": "synthetic U(-0.5,0.5), seeds 12345/54321",
        "config": {"workload": workload, "parallelism": "single-gpu"},
        # the reference's protocol (testing/test_flops.hpp:169-206): median of per-call event timings
        "ms_per_step_median_of_events": med_ms, "value_median_of_events": flops / (med_ms * 1e-3) * 1e-12,
        "roofline": roof,
        "settled": {"value": flops / (settled_ms * 1e-3) * 1e-12, "unit": "TFLOPS", "ms_per_step": settled_ms,
                    "protocol": f"{heat_calls} untimed calls ({time.perf_counter() - t_heat:.1f} s incl. the timed ones, host idle) then the median of 30 event-timed calls",
                    "sclk_mhz": float(np.mean([s_[0] for s_ in busy])) if busy else None,
                    "socket_power_w": float(np.mean([s_[1] for s_ in busy])) if busy else None, "smi_samples": len(busy)},
    }
    # the HBM-bound kernels beside the GEMM (events on the launch stream inside the timed region): algorithmic bytes / time
    # against the 8 TB/s HBM3E peak (a 16-B-per-lane streaming copy reaches ~6.3 TB/s on this part, MI355X_MICROARCH.md)
    q_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in phase_events]))
    c_ms = float(np.mean([e[2].elapsed_time(e[3]) for e in phase_events]))
    q_bytes = 2.0 * (8.0 * n * n + N * n * n)   # quantise A and B: read the FP64 operand, write N int8 planes
    c_bytes = N * n * n + 8.0 * n * n             # CRT: read N int8 planes, write the FP64 result
    out["secondary_kernels"] = [
        {"kernel": "oz2 quantise pair: A (row-strided) + B (K-major), <double,MOD> (+ shift_finalize; fast mode: + the norm kernels)",
         "bound": "hbm", "ms": q_ms, "algorithmic_bytes": q_bytes, "achieved": q_bytes / q_ms * 1e-6, "peak": 8000.0, "unit": "GB/s",
         "frac": q_bytes / q_ms * 1e-6 / 8000.0},
        {"kernel": "oz2::crt_dma_kernel<double> (CRT + unscale + axpby; register form oz2::crt_kernel for ragged shapes)", "bound": "hbm", "ms": c_ms, "algorithmic_bytes": c_bytes, "achieved": c_bytes / c_ms * 1e-6,
         "peak": 8000.0, "unit": "GB/s", "frac": c_bytes / c_ms * 1e-6 / 8000.0}]
    if not args.fast:
        b_ms = float(np.mean([e[4].elapsed_time(e[0]) for e in phase_events]))
        b_bytes = 3.0 * 8.0 * n * n + 2.0 * n * n   # A read twice (amax, extract), B once; two 1-byte bound planes written
        out["secondary_kernels"].append(
            {"kernel": "accurate-mode bounds phase: amax + extract (A, B) + bound GEMM (1 INT8 GEMM) + zeroing", "bound": "hbm + mfma",
             "ms": b_ms, "algorithmic_bytes": b_bytes, "lowprec_ops": flops})
    out["phase_ms"] = {"bounds": float(np.mean([e[4].elapsed_time(e[0]) for e in phase_events])) if not args.fast else 0.0,
                       "quantise": q_ms, "lowprec_gemm": gemm_ms, "crt": c_ms}
    out["max_rel_err"] = sampled_error(A, B, C_head, n)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"C": C_head})
    nat["max_rel_err"] = sampled_error(A, B, Cn, n)
    del Cn, C_head
    out["native_fp64_dgemm_same_gpu"] = nat
    out["other_mode"] = {"mode": "fast" if other else "accurate", "value": flops / oms * 1e-9, "unit": "TFLOPS", "ms_per_step": oms,
                         "max_rel_err": sampled_error(A, B, C_other, n)}
    if not args.no_cpu:
        # The CPU legs take ~14 s of host time (oracle port on one core, OpenBLAS on 128 threads).  They run on a helper thread (both are
        # foreign calls that release the GIL) while THIS thread keeps issuing the emulated GEMM: the device is busy for the whole life of the
        # process instead of idling behind 0.14 s of timed work, and the loop doubles as a sustained-throughput figure
        # (thermally settled, but with the host cores busy beside the launch thread: reported separately, never as `value`).
        import threading
        cpu = {}

        def cpu_legs():
            cpu["cpu_baseline"] = cpu_baseline_port(N, args.fast)
            cpu["host_blas_dgemm"] = host_blas(n)
        th = threading.Thread(target=cpu_legs)
        th.start()
        calls, t2 = 0, time.perf_counter()
        while th.is_alive():
            for _ in range(20):
                step(False)
            torch.cuda.synchronize()
            calls += 20
        sus = time.perf_counter() - t2
        th.join()
        out.update(cpu)
        out["sustained_beside_cpu_legs"] = {"value": flops * calls / sus * 1e-12, "unit": "TFLOPS", "calls": calls, "seconds": sus,
                                            "note": "the same step looped while the CPU baselines run on the host cores; not the headline"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
