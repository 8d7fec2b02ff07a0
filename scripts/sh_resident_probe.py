#!/usr/bin/env python3
"""What the on-chip Newton-CG path (SwiftHohenberg.run_batch) does to the implicit SH stepper on
small grids.

In one process, at k = 0.2, r = 0.01, g = 1 (sh_scipy_nk.py's constants), default f_tol, from
seeded 0.5 * standard_normal states:

  step        SwiftHohenberg.step in a loop, jvp="fd" and jvp="analytic": the multi-launch path,
              the yardstick
  run_batch   B = 1 with one step per call and with --long steps in one launch, plain and
              precond="spectral"; B in --batches with --steps steps in one launch

Every leg is warmed up with the launches it times, starts from the same states, and is timed with
a host clock around calls that end in a device synchronise.  Reports steps/s per member and in
total, Newton and CG iterations per step (member 0) and microseconds per CG iteration (wall time
of the leg over the CG iterations of one member: members run side by side).  Prints a markdown
table (and appends it to --out).

    python scripts/sh_resident_probe.py [--ny 64 --nx 64] [--h 0.625] [--out profiles/...md]

To keep a failed leg from starting another on the GPU, run each grid as a command of its own under
a time limit and chain them:

    timeout -k 10 300 python scripts/sh_resident_probe.py && \\
    timeout -k 10 300 python scripts/sh_resident_probe.py --h 0.0625 --no-plain && \\
    timeout -k 10 300 python scripts/sh_resident_probe.py --ny 128 --h 0.0625 --no-plain
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
    ap.add_argument("--ny", type=int, default=64)
    ap.add_argument("--nx", type=int, default=64)
    ap.add_argument("--h", type=float, default=0.625)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--steps", type=int, default=20, help="steps per launch of the batched legs")
    ap.add_argument("--long", type=int, default=50, help="steps of the B = 1 single launch")
    ap.add_argument("--loop", type=int, default=20, help="calls of the one-step-per-call legs")
    ap.add_argument("--reps", type=int, default=3, help="timed repeats of each launch leg")
    ap.add_argument("--no-plain", action="store_true",
                    help="stiff meshes: skip the step loops and plain CG (thousands of iterations)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import nkhip

    ny, nx, h = args.ny, args.nx, args.h
    batches = [int(b) for b in args.batches.split(",") if b]
    U0 = torch.as_tensor(0.5 * np.random.default_rng(2020).standard_normal((max(batches + [1]),
                                                                            ny * nx)), device="cuda")
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
        nit, cg = its
        rows.append(f"| {name} | {B} | {steps} | {steps / dt:.1f} | {B * steps / dt:.1f} | "
                    f"{nit / steps:.1f} | {cg / steps:.1f} | "
                    + (f"{1e6 * dt / cg:.2f} |" if cg else "– |"))
        print(rows[-1], flush=True)

    def loop_step(s):
        def fn():
            U, nit = U0[0].reshape(ny, nx), 0
            for _ in range(args.loop):
                U = s.step(U)
                nit += s.last_stats["nit"]
            return nit, 0
        return fn

    def loop_batch(s, pc):
        def fn():
            U, nit, cg = U0[:1], 0, 0
            for _ in range(args.loop):
                U = s.run_batch(U, precond=pc)
                nit += int(s.last_batch["nit"][0])
                cg += int(s.last_batch["iters"][0])
            return nit, cg
        return fn

    def launch(s, B, steps, pc):
        def fn():
            s.run_batch(U0[:B], nsteps=steps, precond=pc)
            return int(s.last_batch["nit"][0]), int(s.last_batch["iters"][0])
        return fn

    kw = dict(N=nx, ny=ny, d=h * nx, k=0.2, r=0.01, g=1.0)
    spectral_ok = all(8 <= v <= 128 and v & (v - 1) == 0 for v in (ny, nx)) and ny * nx <= 8192
    if not args.no_plain:
        for jvp in ("fd", "analytic"):
            s = nkhip.SwiftHohenberg(jvp=jvp, **kw)
            try:
                dt, its = timed(loop_step(s), 1)
                row(f"`step` loop, jvp={jvp}", 1, args.loop, dt, its)
            finally:
                s.close()
    s = nkhip.SwiftHohenberg(**kw)
    try:
        for pc in ([] if args.no_plain else [None]) + (["spectral"] if spectral_ok else []):
            tag = "plain" if pc is None else pc
            dt, its = timed(loop_batch(s, pc), 1)
            row(f"`run_batch` {tag}, 1 step per call", 1, args.loop, dt, its)
            dt, its = timed(launch(s, 1, args.long, pc), args.reps)
            row(f"`run_batch` {tag}, one launch", 1, args.long, dt, its)
            for B in batches:
                dt, its = timed(launch(s, B, args.steps, pc), args.reps)
                row(f"`run_batch` {tag}, one launch", B, args.steps, dt, its)
    finally:
        s.close()
    text = "\n".join([f"## sh_resident_probe: {ny} x {nx}, h = {h}, k = 0.2, r = 0.01, g = 1", "",
                      "| leg | B | steps | steps/s per member | steps/s in total | Newton its/step | "
                      "CG its/step (member 0) | us per CG iteration |",
                      "|---|---|---|---|---|---|---|---|"] + rows) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
