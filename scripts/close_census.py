#!/usr/bin/env python3
"""How the LGMRES cycles of one run ended, from the solver's launch log (NKHIP_LAUNCH_LOG).

    python scripts/close_census.py <launch log> [grid points, default 4096*4096] [inner_m, 30]

Every LGMRES call ends with the combination that forms dx (the last krylov_combo before the line
search's first sh_trial).  What precedes it tells how the cycle ended (csrc/lgmres.cpp):
  closed      krylov_combo, reduce_final, dx of 3 vectors: a closing pass, confirmed;
              `at m` when its step was the last the call may take (the augmentation count of a
              call is the number of calls since the time step's sh_bold, at most 10)
  discarded   arnoldi_fused / JVP + multi-dot, reduce_final, dx: the stop was not predicted and
              the step issued past it was thrown away
  exact       krylov_combo, reduce_final, dx of j + 2 vectors: the exact-norm step ended it
A closing pass inside a call (krylov_combo, reduce_final, krylov_combo that is not dx) is a
misprediction "last" whose step went on through the exact-norm path.
Prints one JSON object; `launches` lists (kind, log line) of the closing launches in order.
"""
import json
import sys


def census(path, n=4096 * 4096, inner_m=30, outer_k=10):
    log = []
    for line in open(path):
        c, b = line.split()
        log.append((c, float(b)))
    vec = 8.0 * n
    res = {"calls": 0, "closed_residual": 0, "closed_at_m": 0, "discarded": 0, "exact_end": 0,
           "mispredicted_last": 0, "other": 0, "closing_launches": [], "discarded_launches": [],
           "dx_launches": []}
    n_o = 0
    start = 0  # first launch of the current call (after the previous sh_trial)
    i = 0
    while i < len(log):
        c = log[i][0]
        if c == "sh_bold":
            n_o = 0
        if c != "sh_trial":
            i += 1
            continue
        # the dx combination: the last krylov_combo before this sh_trial
        d = i - 1
        while d >= start and log[d][0] != "krylov_combo":
            d -= 1
        if d < start:  # the initial evaluation of a time step, a backtracking trial
            start = i + 1
            i += 1
            continue
        res["calls"] += 1
        res["dx_launches"].append(d)
        body = [k for k in range(start, d) if log[k][0] != "reduce_final"]
        prev = body[-1] if body else None
        nz = round(log[d][1] / vec) - 1
        if prev is not None and log[prev][0] == "krylov_combo" and nz == 2:
            nc = round(log[prev][1] / vec) - 2
            j = nc - 2 - n_o
            at_m = j + 1 >= inner_m + n_o
            res["closed_at_m" if at_m else "closed_residual"] += 1
            res["closing_launches"].append(("at_m" if at_m else "residual", prev))
        elif prev is not None and log[prev][0] == "krylov_combo":
            res["exact_end"] += 1
        elif prev is not None and log[prev][0] in ("arnoldi_fused", "krylov_mdot"):
            res["discarded"] += 1
            if log[prev][0] == "arnoldi_fused":
                res["discarded_launches"].append(prev)
        else:
            res["other"] += 1
        # closing passes inside the call that were not confirmed
        for a, b in zip(body[:-1], body[1:]):
            if (log[a][0] == "krylov_combo" and log[b][0] == "krylov_combo"
                    and not (a == prev and nz == 2)):
                res["mispredicted_last"] += 1
                res["closing_launches"].append(("mispredicted", a))
        n_o = min(n_o + 1, outer_k)
        start = i + 1
        i += 1
    res["closing_launches"].sort(key=lambda t: t[1])
    return res, log


if __name__ == "__main__":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096 * 4096
    m = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    print(json.dumps(census(sys.argv[1], n, m)[0]))
