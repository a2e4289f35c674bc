"""Cost of non-finite mode 1 (gemmul8_set_nonfinite_mode), interleaved A/B/C arms on one GPU:
  mode0      the default path;
  ieee       mode 1 on finite operands (flag launch + an empty patch launch);
  ieee_flag  mode 1 with one flagged row of op(A) (a NaN) and one flagged column of op(B) (an Inf).
Each round runs every arm `reps` times back to back, the arm order rotating from round to round; per arm the median over rounds of the
per-call time (HIP events around the batch) is reported, and its ratio to mode0.
  python tools/nonfinite_ab.py [--rounds R] [--reps K] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemmul8_amd as g  # noqa: E402

CONFIGS = [("D", torch.float64, g.INT8, 8192, 14), ("D", torch.float64, g.INT8, 1024, 14), ("S", torch.float32, g.FP8, 8192, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}; {g.lib().gemmul8_version().decode()}; rounds {args.rounds} x reps {args.reps}, accurate mode"]
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, dt, be, s, N in CONFIGS:
        A = torch.rand((s, s), generator=gen, dtype=dt, device="cuda") - 0.5
        B = torch.rand((s, s), generator=gen, dtype=dt, device="cuda") - 0.5
        Af, Bf = A.clone(), B.clone()
        Af[s // 3, s // 2] = float("nan")    # column-major tensors (cols, rows): row s/2 of A, column s/3 of B
        Bf[s // 3, s // 5] = float("inf")
        C = torch.zeros((s, s), dtype=dt, device="cuda")
        tot, _, _ = g.work_size(False, be, s, s, s, N)
        work = torch.empty(tot, dtype=torch.uint8, device="cuda")
        arms = {"mode0": (0, A, B), "ieee": (1, A, B), "ieee_flag": (1, Af, Bf)}
        times = {a: [] for a in arms}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def batch(arm, reps):
            mode, X, Y = arms[arm]
            g.set_nonfinite_mode(mode)
            ev0.record()
            for _ in range(reps):
                g.gemm(X, Y, N, backend=be, C_out=C, work=work)
            ev1.record()
            ev1.synchronize()
            g.set_nonfinite_mode(0)
            return ev0.elapsed_time(ev1) / reps
        for arm in arms:
            batch(arm, 2)  # warm-up
        order = list(arms)
        for r in range(args.rounds):
            for arm in order[r % 3:] + order[:r % 3]:
                times[arm].append(batch(arm, args.reps))
        med = {a: sorted(t)[len(t) // 2] for a, t in times.items()}
        for a in arms:
            rec = {"gemm": f"{name}GEMM {s}^3", "backend": "INT8" if be == g.INT8 else "FP8", "moduli": N, "arm": a, "median_ms": round(med[a], 4),
                   "vs_mode0": round(med[a] / med["mode0"], 4), "all_ms": [round(t, 4) for t in times[a]]}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del A, B, Af, Bf, C, work
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
