"""GPU: SHLinearised.run_batch, the on-chip CG solve of the semi-implicit step for small grids and
ensembles (csrc/shlin_resident.hip), against plain CG in np.longdouble run to a relative residual
of 1e-17.  Bound: the stepper's own, max|u - ref| <= 1e-11 max|ref| (tests/test_gpu_shlin.py); a
float64 CG with the stepper's stopping rule lands 5e-15 to 8e-14 from that reference on these
grids."""
import numpy as np
import pytest
import torch

from conftest import load_golden

gpu = pytest.mark.gpu
K, R = 0.2, 0.2


def ref_step(U, Uo, ny, nx, h, r, g):
    from oracle.sh_oracle import sh13
    U, Uo = np.asarray(U, np.longdouble), np.asarray(Uo, np.longdouble)
    D = (5 * U - Uo) ** 2 * K / 16 - g * K * U
    A = lambda v: v + D * v - K / 2 * sh13(v, ny, nx, h, r, dtype=np.longdouble)  # noqa: E731
    b = U + K / 2 * sh13(U, ny, nx, h, r, dtype=np.longdouble)
    x = U.copy()
    res = b - A(x)
    p, rho = res.copy(), res @ res
    for _ in range(5000):
        if np.sqrt(rho) <= 1e-17 * np.sqrt(b @ b):
            break
        q = A(p)
        a = rho / (p @ q)
        x, res = x + a * p, res - a * q
        rho, old = res @ res, rho
        p = res + rho / old * p
    return x


def states(seed, B, n):
    rng = np.random.default_rng(seed)
    return 0.5 * rng.standard_normal((B, n)), 0.5 * rng.standard_normal((B, n))


def close(u, ref):
    err = np.abs(u - ref).max()
    print(f"max|u - ref| = {float(err):.3e}, bound {1e-11 * float(np.abs(ref).max()):.3e}")
    return err <= 1e-11 * np.abs(ref).max()


# the issue's grids, and the two sides of each switch between the kernel's three variants
# (1024 and 4096 points: 31 x 33 fills the small variant, 17 x 241 is the first grid of the large)
@gpu
@pytest.mark.parametrize("ny,nx,d,g", [(5, 5, 2.0, 0), (5, 7, 2.8, 0), (61, 61, 40, 0),
                                       (48, 64, 40, 1), (64, 64, 40, 0), (96, 96, 60, 1),
                                       (9, 1024, 640, 0), (31, 33, 20.625, 0),
                                       (17, 241, 150.625, 1)])
def test_one_step_against_reference(ny, nx, d, g):
    import nkhip
    U, Uo = states(11, 1, ny * nx)
    s = nkhip.SHLinearised(N=nx, ny=ny, d=d, k=K, r=R, g=g)
    try:
        u = s.step_batch(U, Uo).cpu().numpy()[0]
        lb = s.last_batch
    finally:
        s.close()
    assert close(u, ref_step(U[0], Uo[0], ny, nx, d / nx, R, g))
    assert int(lb["status"][0]) == 0 and float(lb["relres"][0]) <= 1e-14
    assert 0 < int(lb["iters"][0]) <= 1000 and int(lb["steps"][0]) == 1


@gpu
def test_reference_six_steps():
    import nkhip
    z = load_golden("shlin_steps")
    s = nkhip.SHLinearised(N=int(z["N"]), d=float(z["d"]), k=float(z["k"]), r=float(z["r"]),
                           g=float(z["g"]))
    try:
        new, prev = s.run_batch(z["U0"], nsteps=6)
        iters6 = int(s.last_batch["iters"][0])
        assert int(s.last_batch["steps"][0]) == 6
        u, uo, iters = torch.as_tensor(z["U0"]), None, 0
        for _ in range(6):
            u, uo = s.run_batch(u, uo, nsteps=1)
            iters += int(s.last_batch["iters"][0])
    finally:
        s.close()
    assert close(new.cpu().numpy()[0], z["U"][5])
    assert torch.equal(u, new) and torch.equal(uo, prev) and iters == iters6


@gpu
@pytest.mark.parametrize("B,ny,nx,d", [(5, 61, 61, 40), (300, 5, 7, 2.8)])
def test_ensemble(B, ny, nx, d):
    import nkhip
    U, Uo = states(23, B, ny * nx)
    rng = np.random.default_rng(5)
    r, g = rng.uniform(0.05, 0.3, B), rng.integers(0, 2, B).astype(np.float64)
    s = nkhip.SHLinearised(N=nx, ny=ny, d=d, k=K, r=R, g=0.0)
    try:
        u = s.step_batch(U, Uo, r=r, g=g)
        assert torch.equal(u, s.step_batch(U, Uo, r=r, g=g))
        solo = [s.step_batch(U[b], Uo[b], r=r[b:b + 1], g=g[b:b + 1])[0] for b in range(B)]
    finally:
        s.close()
    assert torch.equal(u, torch.stack(solo))
    for b in range(B):
        assert close(u[b].cpu().numpy(), ref_step(U[b], Uo[b], ny, nx, d / nx, r[b], g[b])), b


@gpu
def test_member_isolation_and_stopping():
    import nkhip
    B, n = 4, 64 * 64
    U, Uo = states(31, B, n)
    s = nkhip.SHLinearised(N=64, d=40.0, k=K, r=R, maxiter=3)
    try:
        with pytest.raises(nkhip.NoConvergence):
            s.step_batch(U, Uo)
        assert s.last_batch["status"].tolist() == [nkhip._lib.NK_NO_CONVERGENCE] * B
        assert s.last_batch["iters"].tolist() == [3] * B
    finally:
        s.close()
    bad = U.copy()
    bad[2, 1000] = np.nan
    s = nkhip.SHLinearised(N=64, d=40.0, k=K, r=R)
    try:
        solo = [s.run_batch(U[b], Uo[b], nsteps=n_)[0] for n_ in (1, 4) for b in range(B)]
        for j, nsteps in enumerate((1, 4)):
            with pytest.raises(ValueError, match="non-finite"):
                s.run_batch(bad, Uo, nsteps=nsteps)
            lb, got = s.last_batch, s.last_batch_state[0]
            assert lb["status"].tolist() == [0, 0, nkhip._lib.NK_NONFINITE, 0]
            assert lb["steps"].tolist() == [nsteps, nsteps, 0, nsteps]
            for b in (0, 1, 3):
                assert torch.equal(got[b], solo[j * B + b][0]), (nsteps, b)
    finally:
        s.close()


def test_cap():
    import nkhip
    assert nkhip.SHLinearised.resident_max_points >= 9216


@gpu
def test_refusals():
    import nkhip
    P = nkhip.SHLinearised.resident_max_points
    N = 128 if P < 16384 else int(np.sqrt(P)) + 1
    U, Uo = states(3, 1, N * N)
    s = nkhip.SHLinearised(N=N, d=0.625 * N, k=K, r=R)
    try:
        with pytest.raises(nkhip.NKError):
            s.run_batch(U, Uo)
        u = s.step(U[0], Uo[0]).cpu().numpy()  # refused, and still an ordinary stepper
        assert np.isfinite(u).all() and s.last_relres <= 1e-14
    finally:
        s.close()
    s = nkhip.SHLinearised(N=5, d=2.0, k=K, r=R)
    try:
        with pytest.raises(nkhip.NKError):
            s.run_batch(np.zeros(25), nsteps=0)
        with pytest.raises(ValueError):
            s.run_batch(np.zeros((0, 25)))
    finally:
        s.close()
