"""-m gpu: the multi-GPU plans of include/gemmul8_dist.h with the REAL HIP engine.

The GPU box has one GPU, so (a) two gloo ranks share cuda:0 (host-staged TorchTransport; NCCL refuses duplicate devices) to check
every plan bit for bit against the single-GPU C-ABI result on device memory, (b) the RCCL transport created inside
libgemmul8.so (ncclCommInitRank, all-reduce, grouped send/recv, reduce-scatter) runs with world = 1, and (c) bench.py is
launched the way the driver launches it.  The 8-GPU run uses exactly this code with world = 8."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, plan, grid_rows, N, fast, m, n, k, typ, q, be=0):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gemmul8_amd as g
        from gemmul8_amd import dist as gd
        torch.cuda.set_device(0)
        tdt = {"d": torch.float64, "s": torch.float32, "z": torch.complex128}[typ]
        gen = torch.Generator(device="cuda").manual_seed(4)
        rdt = torch.float32 if typ == "s" else torch.float64

        def rnd(shape):
            x = torch.rand(shape, generator=gen, dtype=rdt, device="cuda") - 0.5
            if tdt.is_complex:
                x = torch.complex(x, torch.rand(shape, generator=gen, dtype=rdt, device="cuda") - 0.5)
            return x.contiguous()
        A, B = rnd((k, m)), rnd((n, k))      # (cols, rows) = column-major m x k, k x n
        Cm = torch.zeros((n, m), dtype=tdt, device="cuda")
        comm = gd.TorchTransport(device=True)
        pl = gd.DistGemm(comm, plan, g._dtype_code(tdt), be, m, n, k, N, fastmode=fast, grid_rows=grid_rows)
        pl.run(A, B, Cm)
        torch.cuda.synchronize()
        pl.gather_result(Cm)
        torch.cuda.synchronize()
        if rank == 0:
            ref, _, _ = g.gemm(A, B, N, fastmode=fast, backend=be)
            torch.cuda.synchronize()
            a = torch.view_as_real(Cm) if tdt.is_complex else Cm
            b = torch.view_as_real(ref) if tdt.is_complex else ref
            nbad = int((a != b).sum().item())
            rel = float(((a - b).abs() / b.abs().clamp_min(1e-300)).max().item())
            q.put((nbad, a.numel(), rel))
        pl.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _start_and_reap(procs, timeout):
    """Start the ranks, wait, and KILL whatever is still alive afterwards: a rank that died (port taken, runtime error) leaves its peer
    inside a collective, and multiprocessing joins non-daemon children at interpreter exit -- one flaky rendezvous then blocks the
    whole pytest process until the collective's own timeout (half an hour)."""
    for p in procs:
        p.daemon = True
        p.start()
    import time
    deadline = time.time() + timeout
    for p in procs:
        p.join(max(0.0, deadline - time.time()))
        if p.exitcode not in (0, None):   # a rank failed: its peers will never finish
            break
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join(10)
    return codes


def _run(plan, grid_rows, N, fast, m, n, k, typ="d", be=0):
    ctx = mp.get_context("spawn")
    for attempt in range(2):   # the free port is chosen before the ranks bind it: one retry for the rare rendezvous collision
        q = ctx.Queue()
        port = _port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, plan, grid_rows, N, fast, m, n, k, typ, q, be)) for r in range(2)]
        codes = _start_and_reap(procs, 300)
        if codes == [0] * len(procs):
            return q.get(timeout=10)
    raise AssertionError(f"ranks exited with {codes}")


@pytest.mark.parametrize("plan,grid_rows", [("blocks", 0), ("blocks", 1), ("moduli", 0)])
@pytest.mark.parametrize("N,fast", [(14, False), (15, True)])
def test_two_ranks_one_gpu_bitwise(plan, grid_rows, N, fast):
    nbad, total, _ = _run(plan, grid_rows, N, fast, 300, 515, 1000)
    assert nbad == 0, f"{plan}: {nbad} of {total} elements differ from the single-GPU result"


@pytest.mark.parametrize("typ,N", [("z", 13), ("s", 8)])
def test_two_ranks_one_gpu_bitwise_other_types(typ, N):
    for plan in ("blocks", "moduli"):
        nbad, total, _ = _run(plan, 0, N, False, 260, 130, 520, typ=typ)
        assert nbad == 0, (plan, typ, nbad, total)


@pytest.mark.parametrize("typ,N,fast", [("s", 8, False), ("d", 13, True), ("z", 9, False)])
def test_two_ranks_one_gpu_bitwise_fp8_backend(typ, N, fast):
    """The FP8 backend through the plans (round 5: FP6 panel images, the fused three-product tile loop with t_begin > 0 and in plane groups, the
    lane-per-fragment writer on a moduli range that starts at an odd modulus, int16 residue exchange): bit-identical to the single-GPU call."""
    for plan in ("blocks", "moduli"):
        nbad, total, _ = _run(plan, 0, N, fast, 260, 140, 520, typ=typ, be=1)
        assert nbad == 0, (plan, typ, nbad, total)


@pytest.mark.parametrize("typ,N,fast", [("d", 14, False), ("d", 16, True), ("s", 8, False), ("z", 15, False)])
def test_fp64sum_variant_mismatch_count(typ, N, fast):
    """Exchange variant (A) (FP64 partial CRT sums, reduce-scatter) against the bit-exact single-GPU result: the hi chain of the
    double-double accumulation is error-free however the moduli are grouped, the rounded lo chain (the only chain for float
    outputs) is not -- a small fraction of the elements moves by an ulp.  The count is printed (pytest -s / DESIGN.md 5)."""
    nbad, total, rel = _run("fp64sum", 0, N, fast, 300, 515, 1000, typ=typ)
    print(f"fp64sum {typ} N={N} fast={fast}: {nbad} of {total} values differ from the single-GPU result, max rel {rel:.3e}")
    assert rel <= (2.0 ** -22 if typ == "s" else 2.0 ** -50), (nbad, total, rel)
    assert nbad <= 0.5 * total


def _overlap_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gemmul8_amd as g
        from gemmul8_amd import dist as gd
        torch.cuda.set_device(0)
        gen = torch.Generator(device="cuda").manual_seed(9)
        m = n = k = 2048
        A = torch.rand((k, m), generator=gen, dtype=torch.float64, device="cuda") - 0.5
        B = torch.rand((n, k), generator=gen, dtype=torch.float64, device="cuda") - 0.5
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        pl = gd.DistGemm(gd.TorchTransport(device=True), "moduli", g.D, g.INT8, m, n, k, 14)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for e in ev:
            e.record()   # (the handles exist after the first record)
        pl.set_events(ev[0], ev[1])
        pl.set_exchange_events([None, None, ev[2], ev[3]])
        pl.run(A, B, Cm)
        torch.cuda.synchronize()
        pl.gather_result(Cm)
        torch.cuda.synchronize()
        if rank == 0:
            ref, _, _ = g.gemm(A, B, 14)
            torch.cuda.synchronize()
            # ev[0] .. ev[1]: first to last residue GEMM of the rank; ev[2] .. ev[3]: first to last grouped send / recv (on the plan's exchange stream)
            q.put((bool(torch.equal(Cm, ref)), ev[2].elapsed_time(ev[1]), ev[0].elapsed_time(ev[2]), ev[1].elapsed_time(ev[3])))
        pl.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_moduli_plan_exchange_starts_before_the_last_gemm_ends():
    """Round 5: the moduli plan multiplies the rank's planes in two groups; the residue blocks of group 0 leave on the plan's exchange stream as
    soon as its GEMMs are done, beside the GEMMs of group 1.  Checked with the plan's own events: the exchange begins after the first GEMM starts and
    BEFORE the last GEMM ends, and ends after it; the result stays bit-identical to the single-GPU one."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_overlap_worker, args=(r, 2, port, q)) for r in range(2)]
    assert _start_and_reap(procs, 300) == [0, 0]
    same, x_to_gemm_end, gemm_begin_to_x, gemm_end_to_x_end = q.get(timeout=10)
    assert same
    assert gemm_begin_to_x > 0 and x_to_gemm_end > 0 and gemm_end_to_x_end > 0, (gemm_begin_to_x, x_to_gemm_end, gemm_end_to_x_end)


def _rccl_worker(port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"], os.environ["WORLD_SIZE"] = "0", "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import ctypes as C
    import gemmul8_amd as g
    from gemmul8_amd import dist as gd
    torch.cuda.set_device(0)
    L = gd._lib()
    cp = C.POINTER(gd.Comm)()
    g.check(L.gemmul8_comm_rccl_from_env(C.byref(cp)), "gemmul8_comm_rccl_from_env")   # the C++-only bootstrap (no torch.distributed)
    comm = cp.contents
    st = torch.cuda.current_stream().cuda_stream
    ok = True
    mx = torch.arange(-5, 1019, dtype=torch.int32, device="cuda")
    ref = mx.clone()
    ok &= comm.allreduce_max_i32(comm.ctx, mx.data_ptr(), mx.numel(), st) == 0
    part = torch.rand(4096, dtype=torch.float64, device="cuda")
    red = torch.empty_like(part)
    ok &= comm.reduce_scatter_sum_f64(comm.ctx, part.data_ptr(), red.data_ptr(), part.numel(), st) == 0
    ok &= comm.sendrecv(comm.ctx, 0, None, st) == 0
    torch.cuda.synchronize()
    ok &= bool(torch.equal(mx, ref)) and bool(torch.equal(part, red))

    class Wrap:
        ptr, rank, world = cp, 0, 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    m, n, k, N = 700, 515, 900, 14
    A = torch.rand((k, m), generator=gen, dtype=torch.float64, device="cuda") - 0.5
    B = torch.rand((n, k), generator=gen, dtype=torch.float64, device="cuda") - 0.5
    refC, _, _ = g.gemm(A, B, N)
    for plan in ("blocks", "moduli", "fp64sum"):
        pl = gd.DistGemm(Wrap, plan, g.D, g.INT8, m, n, k, N)
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        pl.run(A, B, Cm)
        pl.gather_result(Cm)
        torch.cuda.synchronize()
        ok &= bool(torch.equal(Cm, refC))     # one rank: also variant (A) groups all moduli together -> identical bits
        pl.close()
    L.gemmul8_comm_destroy(cp)
    q.put(bool(ok))


def test_rccl_transport_of_the_library_world1():
    """The RCCL transport inside libgemmul8.so (librccl found at run time, unique id, ncclCommInitRank, all-reduce(MAX) on int32,
    reduce-scatter(sum) on FP64, grouped send/recv) and all three plans on it, with the one rank this box allows."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_port(), q))
    assert _start_and_reap([p], 300) == [0]
    assert q.get(timeout=10)


def _check_multi_line(d, ranks, rccl):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "plans", "rccl_ranks", "transport"):
        assert key in d, key
    assert d["n_gpus"] == ranks and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "strong" and d["value"] > 0
    assert "replicated" in d["config"]["parallelism"] and "replicated" in d["config"]["placement"]
    assert d["max_rel_err"] < 1e-9
    assert set(d["plans"]) == {"blocks", "moduli", "fp64sum"}
    for name, p in d["plans"].items():
        for key in ("value", "ms_per_step", "gemm_frac_of_int8_peak_rank0", "bounds_allreduce_ms_rank0", "exchange_ms_rank0", "bytes_sent_rank0",
                    "bytes_received_rank0", "mismatches_vs_moduli", "max_rel_err"):
            assert key in p, (name, key)
        assert p["value"] > 0 and p["max_rel_err"] < 1e-9
    assert d["plans"]["blocks"]["mismatches_vs_moduli"] == 0            # both bit-identical to one GPU, hence to each other
    assert d["plans"]["blocks"]["bytes_sent_rank0"] == 0 and d["plans"]["moduli"]["bytes_sent_rank0"] > 0
    # FP64 partial sums: 16 bytes (hi, lo) per element of the other ranks' column blocks against N / G residue bytes
    assert d["plans"]["fp64sum"]["bytes_sent_rank0"] > d["plans"]["moduli"]["bytes_sent_rank0"] or ranks == 1
    assert d["plans"]["fp64sum"]["mismatches_vs_moduli"] <= 0.001 * d["plans"]["fp64sum"]["elements"]
    assert d["config"]["headline_plan"] in ("blocks", "moduli") and d["value"] == d["plans"][d["config"]["headline_plan"]]["value"]
    assert d["rccl_ranks"] == (ranks if rccl else -1)
    assert d["roofline"]["traffic_measured_in_run"] is False
    # round 4: transport self-test before timing, single-GPU phase times and the per-plan time model they feed
    assert d["dist_selftest"].startswith("ok"), d["dist_selftest"]
    assert set(d["single_gpu_phase_ms"]) == {"bounds", "quantise", "lowprec_gemm", "crt", "lowprec_gemm_by_cus"} and d["single_gpu_phase_ms"]["lowprec_gemm"] > 0
    # round 6: what leaving 8 / 16 CUs to an exchange kernel costs the persistent GEMM, measured on this GPU (the moduli plan's alternative model uses it)
    by = d["single_gpu_phase_ms"]["lowprec_gemm_by_cus"]
    assert set(by) == {"256", "248", "240"} and all(v > 0 for v in by.values())
    if ranks > 1:
        alt = d["plans"]["moduli"].get("model_ms_if_gemm_leaves_cus")
        assert alt and set(alt) == {"248", "240"} and all(v > 0 for v in alt.values())
    assert "exchange_exposed_ms_rank0" in d["plans"]["moduli"]
    for name, p in d["plans"].items():
        assert p["model_ms"] > 0 and abs(sum(p["model_terms_ms"].values()) - p["model_ms"]) < 1e-9, name


def _one_json_line(out):
    import json
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout + out.stderr[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("ranks", [2, 4])
def test_bench_multi_rank_contract(ranks):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one rank per process), here with 2 or 4 ranks sharing
    the box's single GPU over gloo (GEMMUL8_DIST_BACKEND: NCCL refuses duplicate devices): ONE JSON line from rank 0 with the
    contract keys, the right rank count, all three plans measured, an accurate result.  4 ranks, not 8: with this process and the
    launcher that already puts 6 processes on the one GPU of a shared test machine, the most it takes at once."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GEMMUL8_DIST_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), os.path.join(root, "bench.py"), "--gpus", str(ranks), "--steps", "2", "--warmup", "1",
                          "--size", "1024"], env=env, capture_output=True, text=True, timeout=900)
    _check_multi_line(_one_json_line(out), ranks, rccl=False)


def test_bench_plain_python_self_launches_ranks():
    """The driver's OTHER calling convention: plain `python bench.py --gpus 2` with no launcher environment must start two ranks by
    itself (VERDICT r2 missing #1: it used to ignore --gpus and print n_gpus = 1).  One GPU here -> the ranks share it over gloo."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GEMMUL8_DIST_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--size", "1024"],
                         env=env, capture_output=True, text=True, timeout=900)
    _check_multi_line(_one_json_line(out), 2, rccl=False)


def test_bench_rejects_gpus_world_size_mismatch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--size", "1024"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "disagrees" in out.stderr


def test_bench_plan_path_on_real_rccl_one_rank():
    """bench.py's multi-GPU code path (nccl process group with device_id, RCCL communicator of the library, the three plans, barrier,
    max-over-ranks timing, gather) on the REAL RCCL backend with the single rank this box allows (GEMMUL8_BENCH_FORCE_PLAN=1)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GEMMUL8_BENCH_FORCE_PLAN="1")
    env.pop("GEMMUL8_DIST_BACKEND", None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--size", "2048"], env=env, capture_output=True, text=True, timeout=600)
    d = _one_json_line(out)
    assert d["n_gpus"] == 1 and d["value"] > 10 and d["max_rel_err"] < 1e-9 and d["roofline"]["achieved"] > 0
    assert d["rccl_ranks"] == 1 and "RCCL" in d["transport"] and "ncclCommCount" in d["dist_selftest"]
    assert all(p["mismatches_vs_moduli"] == 0 for p in d["plans"].values())   # one rank: every plan groups all moduli together


@pytest.mark.parametrize("how", ["forced", "fallback"])
def test_bench_plan_path_on_torch_nccl_transport_one_rank(how):
    """bench.py's SECOND-choice transport (gemmul8_amd.dist.TorchNcclTransport: the plans' exchanges through torch's own nccl = RCCL
    process group, on the device buffers) with the single rank this box allows: forced by GEMMUL8_DIST_BACKEND=torch-nccl, and reached
    as the fall-back when the library's own communicator cannot be brought up (injected failure)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GEMMUL8_BENCH_FORCE_PLAN="1")
    env.pop("GEMMUL8_DIST_BACKEND", None)
    if how == "forced":
        env["GEMMUL8_DIST_BACKEND"] = "torch-nccl"
    else:
        env["GEMMUL8_BENCH_FAIL_FIRST_TRANSPORT"] = "1"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--size", "2048"], env=env, capture_output=True, text=True, timeout=600)
    d = _one_json_line(out)
    assert d["n_gpus"] == 1 and d["value"] > 10 and d["max_rel_err"] < 1e-9
    assert "torch.distributed" in d["transport"] and d["dist_selftest"].startswith("ok (torch's nccl")
    assert (d["first_choice_failure"] is None) == (how == "forced")
    if how == "fallback":
        assert "FAIL_FIRST_TRANSPORT" in d["first_choice_failure"]
    assert all(p["mismatches_vs_moduli"] == 0 for p in d["plans"].values())


def _torch_nccl_worker(port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import ctypes as C
    import gemmul8_amd as g
    from gemmul8_amd import dist as gd
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    comm = gd.TorchNcclTransport()
    ok, msg = gd.selftest(comm, "cuda:0", None, expect_rccl=True)   # rccl_ranks() = the group's size
    c = comm.ptr.contents
    side = torch.cuda.Stream()
    for st in (torch.cuda.current_stream(), side):                  # the plan's stream need not be torch's current one
        with torch.cuda.stream(st):
            out = torch.arange(5000, dtype=torch.int32, device="cuda").to(torch.uint8)
            inn = torch.zeros_like(out)
        ops = (gd.P2POp * 2)(gd.P2POp(out.data_ptr(), out.numel(), 0, 1), gd.P2POp(inn.data_ptr(), inn.numel(), 0, 0))   # to / from myself
        ok &= c.sendrecv(c.ctx, 2, ops, st.cuda_stream) == 0
        part = torch.rand(4096, dtype=torch.float64, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        red = torch.empty_like(part)
        ok &= c.reduce_scatter_sum_f64(c.ctx, part.data_ptr(), red.data_ptr(), part.numel(), st.cuda_stream) == 0
        torch.cuda.synchronize()
        ok &= bool(torch.equal(inn, out)) and bool(torch.equal(part, red))
    gen = torch.Generator(device="cuda").manual_seed(1)
    m, n, k, N = 700, 515, 900, 14
    A = torch.rand((k, m), generator=gen, dtype=torch.float64, device="cuda") - 0.5
    B = torch.rand((n, k), generator=gen, dtype=torch.float64, device="cuda") - 0.5
    refC, _, _ = g.gemm(A, B, N)
    for plan in ("blocks", "moduli", "fp64sum"):
        pl = gd.DistGemm(comm, plan, g.D, g.INT8, m, n, k, N)
        Cm = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        pl.run(A, B, Cm)
        pl.gather_result(Cm)
        torch.cuda.synchronize()
        ok &= bool(torch.equal(Cm, refC))
        pl.close()
    dist.destroy_process_group()
    q.put((bool(ok), msg))


def test_torch_nccl_transport_world1():
    """gemmul8_amd.dist.TorchNcclTransport (bench.py's second-choice transport: the plans' exchanges through torch's nccl = RCCL process
    group on the device buffers themselves): self-test, a send/recv pair to itself and a reduce-scatter on torch's current stream AND on a
    side stream, and all three plans, with the one rank this box allows."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_torch_nccl_worker, args=(_port(), q))
    assert _start_and_reap([p], 300) == [0]
    ok, msg = q.get(timeout=10)
    assert ok, msg


@pytest.mark.parametrize("typ,N,groups", [("z", 15, 3), ("d", 13, 8)])
def test_fp64sum_in_moduli_groups_two_ranks_one_gpu(typ, N, groups, monkeypatch):
    """GEMMUL8_DIST_FP64_GROUPS on the HIP engine (round 6): group-wise GEMMs -> FP64 partial sums on the caller's stream, reduce-scatter + running sum
    (gemmul8_add_f64) on the plan's exchange stream behind events, two alternating partial buffers.  Same bound against the single-GPU result as the
    one-collective plan; 8 groups of 6-7 planes: empty groups contribute zeros."""
    monkeypatch.setenv("GEMMUL8_DIST_FP64_GROUPS", str(groups))
    nbad, total, rel = _run("fp64sum", 0, N, False, 300, 515, 1000, typ=typ)
    print(f"fp64sum in {groups} groups, {typ} N={N}: {nbad} of {total} values differ from the single-GPU result, max rel {rel:.3e}")
    assert rel <= 2.0 ** -50, (nbad, total, rel)
    assert nbad <= 0.5 * total
