#!/usr/bin/env python3
"""What the on-chip spectral preconditioner (SHLinearised.run_batch(precond="spectral")) does to
small-grid and ensemble runs of the semi-implicit SH stepper.

In one process, at k = 0.2, r = 0.2, g = 0 from seeded 0.5 * standard_normal states, for one grid
and mesh spacing per run and each B in --batches:

  spectral    run_batch(precond="spectral"), one launch
  plain       run_batch, one launch, with maxiter raised so that a stiff mesh converges
  step        SHLinearised(precond="spectral").step in a loop (B = 1: the multi-launch path)

The one-launch legs are timed at --steps and at twice that; the difference removes the call's
fixed cost, and gives microseconds per step and per CG iteration (over the iterations of member
0: members run side by side).  Microseconds per application of M: the spectral leg's per
iteration minus the plain leg's (one application per iteration).  Every leg is warmed up with the
launches it times; host clock around calls that end in a device synchronise; best of --reps.

    python scripts/shlin_resident_precond_probe.py --ny 64 --nx 64 --h 0.0625 [--out profiles/...md]
    python scripts/shlin_resident_precond_probe.py --ny 96 --nx 96 --kind spectral-mixed

--kind names the preconditioner of the spectral and `step` legs: "spectral" (sides that are powers
of two) or "spectral-mixed" (sides 2^a 3^b 5^c, csrc/shlin_resident_pcm.hip).

Run each grid as a command of its own under a time limit and chain them with &&, so that a failed
leg starts nothing more on the GPU.
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
    ap.add_argument("--h", type=float, default=0.0625)
    ap.add_argument("--kind", default="spectral", choices=["spectral", "spectral-mixed"])
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--steps", type=int, default=20, help="steps of the shorter spectral launch")
    ap.add_argument("--plain-steps", type=int, default=2, help="the same for the plain leg")
    ap.add_argument("--loop", type=int, default=100, help="calls of the `step` loop")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import nkhip

    ny, nx, h, k, r, g = args.ny, args.nx, args.h, 0.2, 0.2, 0.0
    batches = [int(b) for b in args.batches.split(",") if b]
    U0 = torch.as_tensor(0.5 * np.random.default_rng(2020).standard_normal((max(batches),
                                                                            ny * nx)), device="cuda")
    kw = dict(N=nx, ny=ny, d=h * nx, k=k, r=r, g=g)
    s = nkhip.SHLinearised(maxiter=20000, **kw)
    m = nkhip.SHLinearised(precond=args.kind, **kw)
    rows = []

    def timed(fn):
        fn()  # warm-up: the same launches as the timed ones
        torch.cuda.synchronize()
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            its = fn()
            torch.cuda.synchronize()
            best = min(best or 1e9, time.perf_counter() - t0)
        return best, its

    def launch(B, steps, precond):
        def fn():
            s.run_batch(U0[:B], nsteps=steps, precond=precond)
            return int(s.last_batch["iters"][0])
        return fn

    def one_launch(name, B, steps, precond):
        (t1, i1), (t2, i2) = timed(launch(B, steps, precond)), timed(launch(B, 2 * steps, precond))
        per_step, per_it = (t2 - t1) / steps, (t2 - t1) / (i2 - i1)
        rows.append(f"| {name} | {B} | {2 * steps} | {2 * steps / t2:.1f} | {B * 2 * steps / t2:.1f} | "
                    f"{i2 / (2 * steps):.1f} | {1e6 * per_step:.1f} | {1e6 * per_it:.2f} |")
        print(rows[-1], flush=True)
        return per_it

    def loop_step():
        U = Uo = U0[0]
        its = 0
        for _ in range(args.loop):
            U, Uo = m.step(U, Uo), U
            its += m.last_iters
        return its

    try:
        for B in batches:
            pc = one_launch(f"`run_batch(precond=\"{args.kind}\")`", B, args.steps, args.kind)
            cg = one_launch("`run_batch`, plain", B, args.plain_steps, None)
            rows.append(f"| one application of M (difference of the two) | {B} | | | | | | "
                        f"{1e6 * (pc - cg):.2f} |")
            print(rows[-1], flush=True)
        dt, its = timed(loop_step)
        rows.append(f"| `step` loop, `precond=\"{args.kind}\"` | 1 | {args.loop} | {args.loop / dt:.1f} | "
                    f"{args.loop / dt:.1f} | {its / args.loop:.1f} | {1e6 * dt / args.loop:.1f} | "
                    f"{1e6 * dt / its:.2f} |")
        print(rows[-1], flush=True)
    finally:
        s.close()
        m.close()
    text = "\n".join([f"## shlin_resident_precond_probe: {ny} x {nx}, h = {h}, k = {k}, r = {r}, "
                      f"g = {g}, {args.kind}", "",
                      "| leg | B | steps | steps/s per member | steps/s in total | "
                      "CG iterations/step (member 0) | us per step | us per CG iteration |",
                      "|---|---|---|---|---|---|---|---|"] + rows) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
