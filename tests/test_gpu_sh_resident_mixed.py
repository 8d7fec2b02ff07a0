"""GPU: SwiftHohenberg.run_batch(precond="spectral-mixed"), the implicit Newton-CG step on chip
with the mixed-radix preconditioner (csrc/sh_resident_pcm.hip), on grid sides 2^a 3^b 5^c.

Bounds are tests/test_gpu_sh_resident.py's: 1e-8 max(1, |U|inf) at a tight f_tol, and
max|F| <= f_tol against the oracle's residual."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import sh_oracle
from test_gpu_sh_resident import F_TOL_DEFAULT, G, K, R, close, dense_root, start, stepper

gpu = pytest.mark.gpu
MIXED = "spectral-mixed"


@gpu
def test_golden_step_at_the_cap():
    z = load_golden("nk_n96_h0625_tight")
    N, h, f_tol = int(z["N"]), float(z["h"]), float(z["f_tol"])
    s = stepper(N, N, h, r=float(z["r"]), g=float(z["g"]), f_tol=f_tol)
    try:
        u = s.run_batch(z["traj"][0], precond=MIXED).cpu().numpy()[0]
        lb = s.last_batch
    finally:
        s.close()
    F = sh_oracle.residual(u, z["traj"][0], N, N, h, float(z["r"]), K, float(z["g"]))
    print({k: v.tolist() for k, v in lb.items()}, "max|F| =", np.abs(F).max())
    assert int(lb["status"][0]) == 0 and int(lb["steps"][0]) == 1
    assert 1 <= int(lb["nit"][0]) <= 20
    assert int(lb["precond"][0]) == int(lb["iters"][0]) > 0
    assert np.abs(F).max() <= f_tol
    assert close(u, z["traj"][1], 1e-8)


@gpu
@pytest.mark.parametrize("ny,nx", [(6, 6), (12, 10), (10, 12), (8, 6), (6, 8), (20, 18), (36, 30)])
def test_small_grids_against_dense_newton(ny, nx):
    U0 = start(ny, nx, 7)
    s = stepper(ny, nx, 0.625, f_tol=1e-10)
    try:
        u = s.step_batch(U0, precond=MIXED).cpu().numpy()[0]
        lb = s.last_batch
    finally:
        s.close()
    assert int(lb["status"][0]) == 0 and int(lb["precond"][0]) == int(lb["iters"][0]) > 0
    assert close(u, dense_root(U0, ny, nx, 0.625), 1e-8)


@gpu
@pytest.mark.parametrize("ny,nx", [(128, 72), (72, 128)])
def test_widest_footprints_on_a_stiff_mesh(ny, nx):
    # amplitude 0.01, as in test_preconditioned_cap: F's own rounding is about 2e-9 |u| at this h
    h, U0 = 0.0625, 0.02 * start(ny, nx, 13, noise=0.01)
    s = stepper(ny, nx, h, f_tol=1e-10, jvp="analytic", inner_M=MIXED)
    try:
        u = s.run_batch(U0, precond=MIXED).cpu().numpy()[0]
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
def test_members_and_launches_are_bitwise_reproducible():
    B, ny, nx, h = 3, 12, 10, 0.625
    U = np.stack([start(ny, nx, 20 + b) for b in range(B)])
    r, g = np.array([0.01, 0.2, -0.1]), np.array([1.0, 0.0, 0.5])
    s = stepper(ny, nx, h, f_tol=1e-10)
    try:
        u = s.run_batch(U, nsteps=2, r=r, g=g, precond=MIXED)
        solo = [s.run_batch(U[b], nsteps=2, r=r[b:b + 1], g=g[b:b + 1], precond=MIXED)[0]
                for b in range(B)]
        u3 = s.run_batch(U, nsteps=3, precond=MIXED)
        v = torch.as_tensor(U)
        for _ in range(3):
            v = s.run_batch(v, precond=MIXED)
    finally:
        s.close()
    assert torch.equal(u, torch.stack(solo))
    assert torch.equal(u3, v)
    for b in range(B):
        own = stepper(ny, nx, h, f_tol=1e-10, r=r[b], g=g[b])
        try:
            assert torch.equal(own.run_batch(U[b], nsteps=2, precond=MIXED)[0], u[b]), b
        finally:
            own.close()


@gpu
@pytest.mark.parametrize("ny,nx", [(14, 14), (9, 12), (128, 80), (16, 16)])
def test_refused_grids_leave_the_stepper_usable(ny, nx):
    U0 = start(ny, nx, 3, noise=0.1)
    s = stepper(ny, nx, 0.625)
    try:
        with pytest.raises(ValueError, match=r"2\^a 3\^b 5\^c|power-of-two"):  # the grid, not the name
            s.run_batch(U0, precond=MIXED)
        u = s.step(torch.as_tensor(U0.reshape(ny, nx), device="cuda")).cpu().numpy().reshape(-1)
    finally:
        s.close()
    assert np.abs(sh_oracle.residual(u, U0, ny, nx, 0.625, R, K, G)).max() <= F_TOL_DEFAULT


@gpu
def test_refused_member():
    """A member with k r_m >= 2 never starts; the others equal a clean run bit for bit."""
    import nkhip
    B, ny, nx = 3, 12, 10
    U = np.stack([start(ny, nx, 40 + b) for b in range(B)])
    r = np.array([R, 2.0 / K, R])
    s = stepper(ny, nx, 0.625)
    try:
        good = s.run_batch(U, nsteps=2, precond=MIXED)
        with pytest.raises(ValueError, match="non-finite"):
            s.run_batch(U, nsteps=2, r=r, precond=MIXED)
        lb, got = s.last_batch, s.last_batch_state
    finally:
        s.close()
    assert lb["status"].tolist() == [0, nkhip._lib.NK_NONFINITE, 0]
    assert lb["steps"].tolist() == [2, 0, 2]
    assert torch.equal(got[0], good[0]) and torch.equal(got[2], good[2])
    assert np.array_equal(got[1].cpu().numpy(), U[1])  # its input
