#!/usr/bin/env python3
"""What the on-chip CG path (SHLinearised.run_batch) does to the semi-implicit SH stepper on the
grids the reference runs.

In one process, at h = 0.625, k = 0.2, r = 0.2, g = 0 (sh_linearised.py's constants), from seeded
0.5 * standard_normal states:

  step        SHLinearised.step in a loop: the multi-launch path, the yardstick
  run_batch   B = 1 with one step per call and with --long steps in one launch; B in --batches
              with --steps steps in one launch

Every leg is warmed up with the launches it times, starts from the same states, and is timed with
a host clock around calls that end in a device synchronise.  Reports steps/s per member and in
total, CG iterations per step and microseconds per CG iteration (wall time of the leg over the
iterations of one member: members run side by side).  Prints a markdown table (and appends it to
--out).

    python scripts/shlin_resident_probe.py [--n 64] [--batches 64,256,1024] [--out profiles/...md]

To keep a failed leg from starting another on the GPU, run each grid as a command of its own under
a time limit and chain them:

    timeout -k 10 300 python scripts/shlin_resident_probe.py --n 64 && \\
    timeout -k 10 300 python scripts/shlin_resident_probe.py --n 96 --batches 256
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "iterative-solvers-summer-2020_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64, help="grid side")
    ap.add_argument("--h", type=float, default=0.625)
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--steps", type=int, default=50, help="steps per launch of the batched legs")
    ap.add_argument("--long", type=int, default=250, help="steps of the B = 1 single launch")
    ap.add_argument("--loop", type=int, default=250, help="calls of the one-step-per-call legs")
    ap.add_argument("--reps", type=int, default=3, help="timed repeats of each launch leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import nkhip

    n, h, k, r, g = args.n, args.h, 0.2, 0.2, 0.0
    batches = [int(b) for b in args.batches.split(",") if b]
    U0 = torch.as_tensor(0.5 * np.random.default_rng(2020).standard_normal((max(batches + [1]),
                                                                            n * n)), device="cuda")
    s = nkhip.SHLinearised(N=n, d=h * n, k=k, r=r, g=g)
    rows = []

    def timed(fn, reps):
        fn()  # warm-up: the same launches as the timed ones
        torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            its = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, its

    def row(name, B, steps, dt, its):
        rows.append(f"| {name} | {B} | {steps} | {steps / dt:.1f} | {B * steps / dt:.1f} | "
                    f"{its / steps:.1f} | {1e6 * dt / its:.2f} |")
        print(rows[-1], flush=True)

    def loop_step():
        U = Uo = U0[0]
        its = 0
        for _ in range(args.loop):
            U, Uo = s.step(U, Uo), U
            its += s.last_iters
        return its

    def loop_batch():
        U, Uo, its = U0[:1], None, 0
        for _ in range(args.loop):
            U, Uo = s.run_batch(U, Uo, nsteps=1)
            its += int(s.last_batch["iters"][0])
        return its

    def launch(B, steps):
        def fn():
            s.run_batch(U0[:B], nsteps=steps)
            return int(s.last_batch["iters"][0])
        return fn

    try:
        dt, its = timed(loop_step, 1)
        row("`step` loop", 1, args.loop, dt, its)
        dt, its = timed(loop_batch, 1)
        row("`run_batch`, 1 step per call", 1, args.loop, dt, its)
        dt, its = timed(launch(1, args.long), args.reps)
        row("`run_batch`, one launch", 1, args.long, dt, its)
        for B in batches:
            dt, its = timed(launch(B, args.steps), args.reps)
            row("`run_batch`, one launch", B, args.steps, dt, its)
    finally:
        s.close()
    text = "\n".join([f"## shlin_resident_probe: {n} x {n}, h = {h}, k = {k}, r = {r}, g = {g}", "",
                      "| leg | B | steps | steps/s per member | steps/s in total | "
                      "CG iterations/step (member 0) | us per CG iteration |",
                      "|---|---|---|---|---|---|---|"] + rows) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
