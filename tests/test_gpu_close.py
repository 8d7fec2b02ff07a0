"""GPU: the closing pass of an LGMRES cycle (csrc/krylov.hip close_launch, csrc/lgmres.cpp).

The kernel against a torch fp64 reference, and the solver with the closing pass off
(NKHIP_CLOSE=0), on (1) and forced at the first step of every LGMRES call (2: the prediction is
wrong there, so the fallback to the exact-norm step runs).
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
# 2048-element chunk boundary, one past it, a partial last block, a ragged grid
LENGTHS = [1, 2047, 2048, 2049, 4097, 40 * 130]
NVECS = [1, 2, 3, 20, 37]


def _inputs(n, nvec):
    g = torch.Generator(device="cpu").manual_seed(1000 * nvec + n)
    P = torch.randn(nvec, n, generator=g, dtype=torch.float64)
    c = torch.randn(3, nvec, generator=g, dtype=torch.float64)
    c[torch.rand(3, nvec, generator=g) < 0.25] = 0.0  # exact zeros: multiplied and added too
    if nvec >= 3:
        c[:, 1] = 0.0  # a vector none of the three sums takes
    return P, c


@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("n", LENGTHS)
def test_close_kernel_matches_fp64_reference(n, nvec):
    from nkhip.ops import lgmres_close
    P, c = _inputs(n, nvec)
    vecs = [P[i].cuda() for i in range(nvec)]  # distinct allocations, like the solver's pool
    A, B, nrm = lgmres_close(vecs, c[0].tolist(), c[1].tolist(), c[2].tolist())
    ref = (c[:, :, None] * P[None]).sum(1)              # (3, n): N, A, B
    mag = (c[:, :, None] * P[None]).abs().sum(1)        # sum_i |c_i p_i|
    for name, got, k in (("A", A, 1), ("B", B, 2)):
        err = (got.cpu() - ref[k]).abs()
        tol = 4 * nvec * EPS * mag[k]
        worst = float((err - tol).max())
        print(f"n={n} nvec={nvec} {name}: max err {float(err.max()):.3e}, "
              f"max err/tol {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert worst <= 0.0, (name, n, nvec, float(err.max()))
    ref2 = float((ref[0] * ref[0]).sum())
    print(f"n={n} nvec={nvec} norm2: rel err {abs(nrm - ref2) / max(ref2, 1e-300):.3e}")
    assert abs(nrm - ref2) <= 1e-13 * ref2, (nrm, ref2)
    # the next call walks the chunks in the opposite direction: the same bits
    A2, B2, nrm2 = lgmres_close(vecs, c[0].tolist(), c[1].tolist(), c[2].tolist())
    assert torch.equal(A, A2) and torch.equal(B, B2) and nrm == nrm2


def test_close_wrapper_rejects_a_vector_listed_twice():
    from nkhip.ops import lgmres_close
    p = torch.ones(64, dtype=torch.float64, device="cuda")
    q = torch.ones(64, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        lgmres_close([p, q, p], [1.0] * 3, [1.0] * 3, [1.0] * 3)
    import ctypes as C

    from nkhip import _lib
    ptrs = (C.c_void_p * 2)(p.data_ptr(), p.data_ptr())
    one = (C.c_double * 2)(1.0, 1.0)
    r = C.c_double()
    rc = _lib.lib.nk_debug_close(ptrs, one, one, one, 2, 64, C.c_void_p(q.data_ptr()),
                                 C.c_void_p(torch.empty_like(q).data_ptr()), C.byref(r), None)
    assert rc == _lib.NK_EINVAL


# ------------------------------------------------------------------------------------- solver
GRIDS = {"64x64": (64, 64), "96x130": (96, 130)}
# Max-abs disagreement of the final fields allowed between NKHIP_CLOSE=0, 1 and 2: ten times what
# the parent commit's own two exact paths (NKHIP_LAGNORM=0 against 1, one process each) disagree
# by on the same case -- one decimal of headroom for a third summation order.  Measured on an
# MI355X with the library built from the parent's solver sources (profiles/lgmres_close.md
# section 3), max|U_lag0 - U_lag1| after the two steps, max|U| = 2.74 / 2.78:
PARENT_LAG_DISAGREEMENT = {("64x64", "fd"): 5.218048e-15, ("64x64", "analytic"): 5.551115e-15,
                           ("96x130", "fd"): 5.773160e-15, ("96x130", "analytic"): 6.439294e-15}
FIELD_BOUND = {k: 10 * v for k, v in PARENT_LAG_DISAGREEMENT.items()}


@functools.lru_cache(maxsize=None)
def _solve(grid, jvp):
    """Two steps per NKHIP_CLOSE mode: {mode: (final field, [stats per step], jvp launches)}."""
    import nkhip
    ny, nx = GRIDS[grid]
    U0 = np.random.default_rng(2020).standard_normal(ny * nx).reshape(ny, nx)
    out = {}
    old = os.environ.get("NKHIP_CLOSE")
    try:
        for mode in ("0", "1", "2"):
            os.environ["NKHIP_CLOSE"] = mode  # read per LGMRES call
            m = nkhip.SwiftHohenberg(N=nx, ny=ny, d=0.625 * nx, k=0.2, r=0.01, g=1.0,
                                     f_tol=1e-10, jvp=jvp)
            U = torch.as_tensor(U0, device="cuda")
            stats = []
            for _ in range(2):
                U = m.step(U)
                stats.append(m.last_stats)
            prof = m.kernel_profile()
            m.close()
            passes = sum(prof.get(k, {}).get("launches", 0)
                         for k in ("arnoldi_fused", "sh_fdjvp", "sh_ajvp"))
            out[mode] = (U.cpu().numpy(), stats, passes)
    finally:
        if old is None:
            os.environ.pop("NKHIP_CLOSE", None)
        else:
            os.environ["NKHIP_CLOSE"] = old
    return out


@pytest.mark.parametrize("jvp", ["fd", "analytic"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_solver_same_iterations_with_and_without_closing_pass(grid, jvp):
    runs = _solve(grid, jvp)
    for s in range(2):
        st = {mode: runs[mode][1][s] for mode in runs}
        print(grid, jvp, "step", s, {mode: (v["nit"], v["nfev"] + v["njvp"])
                                    for mode, v in st.items()})
        assert all(v["status"] == 0 for v in st.values())
        assert st["0"]["nit"] == st["1"]["nit"] == st["2"]["nit"], st
        calls = [v["nfev"] + v["njvp"] for v in st.values()]
        assert max(calls) - min(calls) <= 1, st


@pytest.mark.parametrize("jvp", ["fd", "analytic"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_solver_same_fields_with_and_without_closing_pass(grid, jvp):
    runs = _solve(grid, jvp)
    for mode in ("1", "2"):
        diff = float(np.abs(runs[mode][0] - runs["0"][0]).max())
        bound = FIELD_BOUND[(grid, jvp)]
        print(f"{grid} {jvp} NKHIP_CLOSE={mode} vs 0: max|dU| = {diff:.3e} (bound {bound:.3e})")
        assert diff <= bound, (grid, jvp, mode, diff, bound)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_closing_pass_replaces_discarded_steps(grid):
    """A cycle that ends in a closing pass issues no step past its last one: fewer JVP-carrying
    launches than with NKHIP_CLOSE=0, where every cycle that stops on its residual test has run
    one.  FD mode: the pass is taken where the step past the last one would be a fused launch,
    and the analytic JVP has no fused step (there the three modes are one path)."""
    runs = _solve(grid, "fd")
    print(grid, "JVP-carrying launches", {mode: runs[mode][2] for mode in runs})
    assert runs["1"][2] < runs["0"][2]
    ana = _solve(grid, "analytic")
    assert ana["1"][2] == ana["0"][2] == ana["2"][2]


@pytest.mark.parametrize("jvp", ["fd", "analytic"])
def test_forced_misprediction_solves_golden_case(jvp, monkeypatch):
    """NKHIP_CLOSE=2 on the 61 x 61 fixture, held to the tolerance test_gpu_nk.py applies to it.
    (An odd grid has no fused step, so no closing pass is applicable here and the switch must
    change nothing; the forced misprediction itself -- a closing pass at the first step of every
    LGMRES call that finds the process going on and falls back to the exact-norm step -- runs in
    the NKHIP_CLOSE=2 legs of the 64 x 64 and 96 x 130 FD cases above.)"""
    import nkhip
    monkeypatch.setenv("NKHIP_CLOSE", "2")
    z = load_golden("nk_n61_tight")
    N = int(z["N"])
    m = nkhip.SwiftHohenberg(N=N, d=float(z["d"]), k=float(z["k"]), r=float(z["r"]),
                             g=float(z["g"]), f_tol=float(z["f_tol"]), jvp=jvp)
    U = m.step(torch.as_tensor(z["traj"][0].reshape(N, N), device="cuda"))
    st = m.last_stats
    m.close()
    assert st["status"] == 0
    ref = z["traj"][1]
    err = float(np.abs(U.cpu().numpy().reshape(-1) - ref).max())
    print(f"forced fallback, {jvp}: |dU|inf vs scipy = {err:.3e}")
    assert err <= 1e-8 * max(1.0, float(np.abs(ref).max()))
