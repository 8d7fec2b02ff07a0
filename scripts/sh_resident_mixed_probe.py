#!/usr/bin/env python3
"""What the on-chip mixed-radix preconditioner (SwiftHohenberg.run_batch(precond="spectral-mixed"),
csrc/sh_resident_pcm.hip) does to the implicit SH stepper on small grids with sides 2^a 3^b 5^c.

In one process, at k = 0.2, r = 0.01, g = 1 (sh_scipy_nk.py's constants), default f_tol, from
seeded 0.5 * standard_normal states, for one grid and mesh spacing per run:

  mixed    run_batch(precond="spectral-mixed"), --steps steps in one launch, each B in --batches
  plain    run_batch, --plain-steps steps in one launch with --inner-maxiter (raise it on a stiff
           mesh, where a plain solve takes thousands of iterations), each B in --batches
  step     SwiftHohenberg(jvp="analytic", inner_M="spectral-mixed").step in a loop of --loop calls

Every leg is warmed up with the launches it times and timed with device events around calls that
end in a device synchronise; best of --reps.  Reports steps/s per member, Newton and CG iterations
per step (member 0) and microseconds per CG iteration (the leg's time over the CG iterations of
member 0: members run side by side).  Microseconds per application of M: the mixed leg's per
iteration minus the plain leg's at the same B (one application per iteration).  Prints a markdown
table (and appends it to --out).

    python scripts/sh_resident_mixed_probe.py --ny 96 --nx 96 --h 0.625
    python scripts/sh_resident_mixed_probe.py --ny 96 --nx 96 --h 0.0625 --plain-steps 1 \\
        --inner-maxiter 20000

Run each grid as a command of its own under a time limit and chain them with &&, so that a failed
leg starts nothing more on the GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "iterative-solvers-summer-2020_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=96)
    ap.add_argument("--nx", type=int, default=96)
    ap.add_argument("--h", type=float, default=0.625)
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--steps", type=int, default=50, help="steps of the mixed launch")
    ap.add_argument("--plain-steps", type=int, default=50, help="steps of the plain launch")
    ap.add_argument("--inner-maxiter", type=int, default=1000, help="the plain leg's CG cap")
    ap.add_argument("--loop", type=int, default=20, help="calls of the `step` loop")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import nkhip

    ny, nx, h = args.ny, args.nx, args.h
    batches = [int(b) for b in args.batches.split(",") if b]
    U0 = torch.as_tensor(0.5 * np.random.default_rng(2020).standard_normal((max(batches),
                                                                            ny * nx)), device="cuda")
    kw = dict(N=nx, ny=ny, d=h * nx, k=0.2, r=0.01, g=1.0)
    rows = []

    def timed(fn):
        fn()  # warm-up: the same launches as the timed ones
        torch.cuda.synchronize()
        best = None
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            its = fn()
            b.record()
            torch.cuda.synchronize()
            dt = a.elapsed_time(b) * 1e-3
            best = dt if best is None else min(best, dt)
        return best, its

    def row(name, B, steps, dt, its):
        nit, cg = its
        rows.append(f"| {name} | {B} | {steps} | {steps / dt:.1f} | {B * steps / dt:.1f} | "
                    f"{nit / steps:.1f} | {cg / steps:.1f} | {1e6 * dt / steps:.1f} | "
                    f"{1e6 * dt / cg:.2f} |")
        print(rows[-1], flush=True)
        return dt / cg

    def launch(s, B, steps, pc, cap):
        def fn():
            s.run_batch(U0[:B], nsteps=steps, precond=pc, inner_maxiter=cap)
            return int(s.last_batch["nit"][0]), int(s.last_batch["iters"][0])
        return fn

    s = nkhip.SwiftHohenberg(**kw)
    try:
        for B in batches:
            pc = row('`run_batch(precond="spectral-mixed")`', B, args.steps,
                     *timed(launch(s, B, args.steps, "spectral-mixed", 1000)))
            cg = row(f"`run_batch`, plain (`inner_maxiter={args.inner_maxiter}`)", B,
                     args.plain_steps,
                     *timed(launch(s, B, args.plain_steps, None, args.inner_maxiter)))
            rows.append(f"| one application of M (difference of the two) | {B} | | | | | | | "
                        f"{1e6 * (pc - cg):.2f} |")
            print(rows[-1], flush=True)
    finally:
        s.close()
    m = nkhip.SwiftHohenberg(jvp="analytic", inner_M="spectral-mixed", **kw)
    try:
        def loop_step():
            U, nit, inner = U0[0].reshape(ny, nx), 0, 0
            for _ in range(args.loop):
                U = m.step(U)
                nit += m.last_stats["nit"]
                inner += m.last_stats["njvp"]
            return nit, inner
        row('`step` loop, `inner_M="spectral-mixed"` (inner column: JVPs)', 1, args.loop,
            *timed(loop_step))
    finally:
        m.close()
    text = "\n".join([f"## sh_resident_mixed_probe: {ny} x {nx}, h = {h}, k = 0.2, r = 0.01, g = 1",
                      "",
                      "| leg | B | steps | steps/s per member | steps/s in total | Newton its/step | "
                      "CG its/step (member 0) | us per step | us per CG iteration |",
                      "|---|---|---|---|---|---|---|---|---|"] + rows) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
