#!/usr/bin/env python3
"""What the spectral preconditioner (precond="spectral") does to the semi-implicit SH stepper.

In one process: warm-up steps, then timed steps of SHLinearised once with precond=None (the
stepper as it is without the option) and once with precond="spectral", both from the same start
state; steps/s, CG iterations and applications of M per step for both legs, and the HIP-event
time of one application of M with and without the fused dot (nk_debug_shlin_precond_time).
Prints a markdown report (and appends it to --out).

    python scripts/shlin_precond_probe.py [--n 4096] [--h 0.625] [--out profiles/...md]

--start bench is bench.py's seeded state, --start smooth a smooth field of amplitude 0.5 (the
stiff h = 0.0625 case is meaningful only from a resolved state).  --maxiter bounds the CG
iterations of the unpreconditioned leg; a leg whose step does not converge within it is reported
as such instead of timed.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "iterative-solvers-summer-2020_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(nkhip, torch, U0, n, h, k, r, g, precond, warmup, steps, maxiter):
    s = nkhip.SHLinearised(N=n, d=h * n, k=k, r=r, g=g, precond=precond, maxiter=maxiter)
    U = Uo = U0.reshape(-1).clone()
    try:
        for i in range(warmup):
            try:
                U, Uo = s.step(U, Uo), U
            except nkhip.NoConvergence:
                return {"failed": f"step {i}: no convergence in {s.last_iters} CG iterations "
                                  f"(relative residual {s.last_relres:.3e})"}
            print(f"  [{precond}] warm-up step {i}: its {s.last_iters}, M applications "
                  f"{s.last_precond}, shift {s.last_shift:.4g}, relres {s.last_relres:.2e}",
                  flush=True)
        its = napp = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            U, Uo = s.step(U, Uo), U
            its += s.last_iters
            napp += s.last_precond
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"steps_per_s": steps / dt, "its": its / steps, "napp": napp / steps,
                "shift": s.last_shift, "relres": s.last_relres, "last": U}
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--h", type=float, default=0.625, help="mesh spacing (bench.py: 0.625)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20, help="applications of M between two events")
    ap.add_argument("--maxiter", type=int, default=1000, help="of the unpreconditioned leg")
    ap.add_argument("--start", choices=["bench", "smooth"], default="bench")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import nkhip

    n, h, k, r, g = args.n, args.h, 0.2, 0.2, 0.0
    if args.start == "bench":
        U0 = torch.as_tensor(bench.slab_of_seeded_grid(2020, n, 0, n), device="cuda")
    else:
        x = 2 * np.pi * np.arange(n) / n
        U0 = torch.as_tensor(0.5 * np.cos(3 * x)[:, None] * np.sin(2 * x)[None, :],
                             device="cuda")
    res, failed = {}, []
    for name, pc, mi in (("spectral", "spectral", 1000), ("none", None, args.maxiter)):
        v = run(nkhip, torch, U0, n, h, k, r, g, pc, args.warmup, args.steps, mi)
        if "failed" in v:
            failed.append(f"precond = {name} (maxiter {mi}): {v['failed']}")
        else:
            res[name] = v
    lines = [f"## shlin_precond_probe: {n} x {n}, h = {h}, k = {k}, r = {r}, g = {g}; "
             f"{args.warmup} warm-up steps, {args.steps} timed, start = {args.start}", "",
             "| precond | steps/s | CG iterations/step | M applications/step | last shift | "
             "last relative residual |", "|---|---|---|---|---|---|"]
    for name in ("none", "spectral"):
        if name in res:
            v = res[name]
            lines.append(f"| {name} | {v['steps_per_s']:.3f} | {v['its']:.1f} | {v['napp']:.1f} | "
                         f"{v['shift']:.4g} | {v['relres']:.2e} |")
    if len(res) == 2:
        d = float((res["none"]["last"] - res["spectral"]["last"]).abs().max())
        lines += ["", f"Last timed step, |U_spectral - U_none|inf = {d:.3e} "
                      f"(max|U| {float(res['none']['last'].abs().max()):.3g})."]
    ms_p, ms_d = C.c_double(), C.c_double()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nkhip._lib.check(nkhip.lib.nk_debug_shlin_precond_time(n, n, h, r, k, 0.2, args.reps,
                                                           C.byref(ms_p), C.byref(ms_d), st),
                     "nk_debug_shlin_precond_time")
    pts = float(n) * n
    lines += ["", "| one application of M (HIP events) | ms | algorithmic B/point | TB/s | "
                  "of 8 TB/s |", "|---|---|---|---|---|"]
    base = 80.0 if n > 4096 else 48.0  # columns longer than 4096 are split: five passes, not three
    for nm, ms, bpp in (("five passes" if n > 4096 else "three passes", ms_p.value, base),
                        ("with the fused dot", ms_d.value, base + 8.0)):
        rate = bpp * pts / (ms * 1e-3) / 1e12
        lines.append(f"| {nm} | {ms:.4f} | {bpp:.0f} | {rate:.3f} | {rate / 8.0:.3f} |")
    lines.append("")
    lines += [f"Not timed -- {f}." for f in failed]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
