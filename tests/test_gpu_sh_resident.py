"""GPU: SwiftHohenberg.run_batch, whole implicit steps of small grids on chip (csrc/sh_resident.hip:
Newton-CG with the analytic Jacobian, plain or with the spectral preconditioner).

Bounds are the project's parity bars (tests/test_gpu_nk.py): 1e-8 max(1, |U|inf)
where f_tol is tight, 1e-5 max(1, |U|inf) at the default f_tol = eps^(1/3)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import sh_oracle

gpu = pytest.mark.gpu
K, R, G = 0.2, 0.01, 1.0
F_TOL_DEFAULT = np.finfo(float).eps ** (1 / 3)
BOTH = (None, "spectral")


def pow2(v):
    return v >= 8 and v & (v - 1) == 0


def stepper(ny, nx, h, **kw):
    import nkhip
    kw.setdefault("r", R)
    kw.setdefault("g", G)
    return nkhip.SwiftHohenberg(N=nx, ny=ny, d=h * nx, k=K, **kw)


def close(u, ref, rel):
    err, bound = np.abs(u - ref).max(), rel * max(1.0, np.abs(ref).max())
    print(f"max|u - ref| = {err:.3e}, bound {bound:.3e}")
    return err <= bound


def start(ny, nx, seed, noise=0.5):
    """A few long waves and white noise on top."""
    y, x = np.meshgrid(np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    smooth = 0.5 * np.cos(6 * np.pi * x) * np.sin(4 * np.pi * y)
    return (smooth + noise * np.random.default_rng(seed).standard_normal((ny, nx))).reshape(-1)


GOLDENS = [("nk_n5_d2_tight", 1e-8), ("nk_n61_tight", 1e-8), ("nk_n64_h0625_tight", 1e-8),
           ("nk_n96_h0625_tight", 1e-8), ("nk_n64_default", 1e-5), ("nk_n61_amp3_backtrack", 1e-5)]


@gpu
@pytest.mark.parametrize("name,rel,precond", [(n, t, p) for n, t in GOLDENS for p in BOTH
                                              if p is None or "n64" in n])
def test_golden_one_step(name, rel, precond):
    z = load_golden(name)
    N, h = int(z["N"]), float(z["h"])
    f_tol = None if np.isnan(z["f_tol"]) else float(z["f_tol"])
    s = stepper(N, N, h, r=float(z["r"]), g=float(z["g"]), f_tol=f_tol)
    try:
        u = s.run_batch(z["traj"][0], precond=precond).cpu().numpy()[0]
        lb = s.last_batch
    finally:
        s.close()
    F = sh_oracle.residual(u, z["traj"][0], N, N, h, float(z["r"]), K, float(z["g"]))
    print({k: v.tolist() for k, v in lb.items()}, "max|F| =", np.abs(F).max())
    assert int(lb["status"][0]) == 0 and int(lb["steps"][0]) == 1
    assert np.abs(F).max() <= (f_tol or F_TOL_DEFAULT)
    assert 1 <= int(lb["nit"][0]) <= 20
    assert close(u, z["traj"][1], rel)


def dense_root(U0, ny, nx, h):
    """Newton with the assembled Jacobian and a direct solve, until max|F| stops falling."""
    u, eye, best, keep = U0.copy(), np.eye(U0.size), np.inf, U0
    for _ in range(50):
        F = sh_oracle.residual(u, U0, ny, nx, h, R, K, G)
        if not np.abs(F).max() < best:
            break
        best, keep = np.abs(F).max(), u
        J = np.stack([sh_oracle.jvp(u, e, ny, nx, h, R, K, G) for e in eye], axis=1)
        u = u - np.linalg.solve(J, F)
    return keep


@gpu
@pytest.mark.parametrize("ny,nx,precond", [(8, 16, None), (8, 16, "spectral"), (16, 8, None),
                                           (16, 8, "spectral"), (5, 7, None), (32, 8, None),
                                           (32, 8, "spectral")])
def test_rectangles_against_dense_newton(ny, nx, precond):
    U0 = start(ny, nx, 7)
    s = stepper(ny, nx, 0.625, f_tol=1e-10)
    try:
        u = s.step_batch(U0, precond=precond).cpu().numpy()[0]
        assert int(s.last_batch["status"][0]) == 0
    finally:
        s.close()
    assert close(u, dense_root(U0, ny, nx, 0.625), 1e-8)


@gpu
@pytest.mark.parametrize("ny,nx", [(128, 64), (64, 128)])
def test_preconditioned_cap(ny, nx):
    # amplitude 0.01: at this h the stencil's terms are 1.3e6 |u|, so F carries rounding of about
    # 13 * 1.3e6 * |u| * 2^-53 ~ 2e-9 |u|; a state of order one could not reach f_tol at all
    h, U0 = 0.0625, 0.02 * start(ny, nx, 13, noise=0.01)
    # step's own solve preconditioned too: a stiff mesh (set_precond has no effect on run_batch)
    s = stepper(ny, nx, h, f_tol=1e-10, jvp="analytic", inner_M="spectral")
    try:
        u = s.run_batch(U0, precond="spectral").cpu().numpy()[0]
        lb = s.last_batch
        ref = s.step(torch.as_tensor(U0.reshape(ny, nx), device="cuda")).cpu().numpy().reshape(-1)
    finally:
        s.close()
    F = sh_oracle.residual(u, U0, ny, nx, h, R, K, G)
    print({k: v.tolist() for k, v in lb.items()}, "max|F| =", np.abs(F).max())
    assert int(lb["status"][0]) == 0 and np.abs(F).max() <= 1e-10
    assert int(lb["precond"][0]) == int(lb["iters"][0]) > 0
    assert close(u, ref, 1e-8)


@gpu
@pytest.mark.parametrize("precond", BOTH)
def test_ten_steps_in_one_launch(precond):
    z = load_golden("nk_n64_traj100")
    assert int(z["steps"][1]) == 10
    s = stepper(64, 64, float(z["h"]))
    try:
        u10 = s.run_batch(z["traj"][0], nsteps=10, precond=precond)
        lb = s.last_batch
        u = torch.as_tensor(z["traj"][0])
        for _ in range(10):
            u = s.run_batch(u, precond=precond)
    finally:
        s.close()
    assert int(lb["steps"][0]) == 10 and int(lb["status"][0]) == 0
    assert close(u10.cpu().numpy()[0], z["traj"][1], 1e-5)
    assert torch.equal(u, u10)


@gpu
@pytest.mark.parametrize("precond", BOTH)
def test_members(precond):
    B, ny, nx, h = 3, 16, 16, 0.625
    U = np.stack([start(ny, nx, 20 + b) for b in range(B)])
    r, g = np.array([0.01, 0.2, -0.1]), np.array([1.0, 0.0, 0.5])
    s = stepper(ny, nx, h, f_tol=1e-10)
    try:
        u = s.run_batch(U, nsteps=2, r=r, g=g, precond=precond)
        solo = [s.run_batch(U[b], nsteps=2, r=r[b:b + 1], g=g[b:b + 1], precond=precond)[0]
                for b in range(B)]
    finally:
        s.close()
    assert torch.equal(u, torch.stack(solo))
    for b in range(B):
        own = stepper(ny, nx, h, f_tol=1e-10, r=r[b], g=g[b])
        try:
            assert torch.equal(own.run_batch(U[b], nsteps=2, precond=precond)[0], u[b]), b
        finally:
            own.close()


@gpu
@pytest.mark.parametrize("precond", BOTH)
def test_failing_and_refused_members(precond):
    import nkhip
    B, ny, nx, h = 3, 16, 16, 0.625
    U = np.stack([start(ny, nx, 40 + b) for b in range(B)])
    bad = U.copy()
    bad[1, 100] = np.nan
    s = stepper(ny, nx, h)
    try:
        good = s.run_batch(U, nsteps=3, precond=precond)
        for Uin, g in ((bad, None), (U, np.array([G, 6.0, G]))):
            with pytest.raises(ValueError, match="non-finite"):
                s.run_batch(Uin, nsteps=3, g=g, precond=precond)
            lb, got = s.last_batch, s.last_batch_state
            assert lb["status"].tolist() == [0, nkhip._lib.NK_NONFINITE, 0]
            assert lb["steps"].tolist() == [3, 0, 3]
            assert torch.equal(got[0], good[0]) and torch.equal(got[2], good[2])
            assert np.array_equal(got[1].cpu().numpy(), Uin[1], equal_nan=True)  # its input
        s.set_options(maxiter=1)
        with pytest.raises(nkhip.NoConvergence):
            s.run_batch(U, precond=precond)
        assert s.last_batch["status"].tolist() == [nkhip._lib.NK_NO_CONVERGENCE] * B
        assert s.last_batch["steps"].tolist() == [0] * B
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("N,precond,opts", [(97, None, {}), (96, "spectral", {}),
                                            (64, "spectral-mixed", {}), (64, None, {"x_tol": 1e-9})])
def test_value_errors_leave_the_stepper_usable(N, precond, opts):
    U0 = start(N, N, 3, noise=0.1)
    s = stepper(N, N, 0.625, **opts)
    try:
        with pytest.raises(ValueError):
            s.run_batch(U0, precond=precond)
        u = s.step(torch.as_tensor(U0.reshape(N, N), device="cuda")).cpu().numpy().reshape(-1)
    finally:
        s.close()
    assert np.abs(sh_oracle.residual(u, U0, N, N, 0.625, R, K, G)).max() <= F_TOL_DEFAULT
