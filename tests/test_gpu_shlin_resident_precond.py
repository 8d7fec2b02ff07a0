"""GPU: SHLinearised.run_batch(precond="spectral"), preconditioned CG with the FFT preconditioner
applied inside the resident workgroup (csrc/shlin_resident_pc.hip).

Reference: preconditioned CG with operator, residual and dots in np.longdouble, run to a relative
residual of 1e-17; its M is shlin_pcg_ref.shift_np on the float64 cast of the residual, which only
steers the search.  Bounds are those of tests/test_gpu_shlin_precond.py: max|u - ref| <= 1e-11
max|ref|, the oracle's |b - A u| / |b| <= 2e-14, iteration counts within 2 of the float64 pcg's
(shlin_pcg_ref.RECORDS), sigma within 1e-14 relative."""
import functools

import numpy as np
import pytest
import torch

import shlin_pcg_ref as sp
from conftest import load_golden

gpu = pytest.mark.gpu
K, R, LD = sp.K, sp.R, np.longdouble
# the five cases of shlin_pcg_ref, and the cap in its other orientation (ny < nx)
NAMES = list(sp.CASES) + ["stiff64x128"]


def state(name):
    if name in sp.CASES:
        return sp.state(name)
    rng = np.random.default_rng(16)
    return 0.5 * rng.standard_normal(8192), 0.5 * rng.standard_normal(8192), 64, 128, 0.0625, 0.0


def ref_solve(U, Uo, ny, nx, h, r, g):
    from oracle.sh_oracle import sh13
    U, Uo = np.asarray(U, LD), np.asarray(Uo, LD)
    D = (5 * U - Uo) ** 2 * LD(K) / 16 - LD(g) * LD(K) * U
    A = lambda v: v + D * v - LD(K) / 2 * sh13(v, ny, nx, h, r, dtype=LD)  # noqa: E731
    b = U + LD(K) / 2 * sh13(U, ny, nx, h, r, dtype=LD)
    sigma = max(float(D.mean()), 0.0)
    M = lambda v: sp.shift_np(np.asarray(v, np.float64).reshape(ny, nx), h, r, K,  # noqa: E731
                              sigma).reshape(-1).astype(LD)
    x = U.copy()
    res = b - A(x)
    z = M(res)
    p, rho = z.copy(), res @ z
    for _ in range(200):
        if np.sqrt(res @ res) <= 1e-17 * np.sqrt(b @ b):
            break
        q = A(p)
        a = rho / (p @ q)
        x, res = x + a * p, res - a * q
        z = M(res)
        rho, old = res @ z, rho
        p = z + rho / old * p
    return x


@functools.lru_cache(maxsize=None)
def case_ref(name):
    U, Uo, ny, nx, h, g = state(name)
    return ref_solve(U, Uo, ny, nx, h, R, g)


def close(u, ref):
    err = np.abs(u - ref).max()
    print(f"max|u - ref| = {float(err):.3e}, bound {1e-11 * float(np.abs(ref).max()):.3e}")
    return err <= 1e-11 * np.abs(ref).max()


def stepper(ny, nx, h, g=0.0, **kw):
    import nkhip
    return nkhip.SHLinearised(N=nx, ny=ny, d=nx * h, k=K, r=R, g=g, **kw)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_step_against_reference(name):
    U, Uo, ny, nx, h, g = state(name)
    record = sp.RECORDS[name] if name in sp.RECORDS else sp.pcg(U, Uo, ny, nx, h, g=g)[1]
    s = stepper(ny, nx, h, g)
    try:
        u = s.step_batch(U, Uo, precond="spectral").cpu().numpy()[0]
        lb = s.last_batch
    finally:
        s.close()
    its, napp, shift = int(lb["iters"][0]), int(lb["precond"][0]), float(lb["shift"][0])
    A, b, _ = sp.system(U, Uo, ny, nx, h, R, K, g)
    rel = float(np.sqrt(((b - A(u)) ** 2).sum()) / np.sqrt(b @ b))
    want = float(sp.shift(U, Uo, K, g))
    print(f"{name}: PCG {its} (record {record}), M applications {napp}, oracle relres {rel:.2e}, "
          f"shift {shift!r} (numpy {want!r})")
    assert close(u, case_ref(name))
    assert rel <= 2e-14
    assert int(lb["status"][0]) == 0 and int(lb["steps"][0]) == 1
    assert abs(its - record) <= 2 and its <= napp <= its + 1
    assert abs(shift - want) <= 1e-14 * want
    if name == "negD64":
        assert shift == 0.0


@gpu
def test_reference_six_steps():
    import nkhip
    z = load_golden("shlin_steps")
    s = nkhip.SHLinearised(N=int(z["N"]), d=float(z["d"]), k=float(z["k"]), r=float(z["r"]),
                           g=float(z["g"]))
    try:
        new, prev = s.run_batch(z["U0"], nsteps=6, precond="spectral")
        iters6 = int(s.last_batch["iters"][0])
        assert int(s.last_batch["steps"][0]) == 6
        u, uo, iters = torch.as_tensor(z["U0"]), None, 0
        for _ in range(6):
            u, uo = s.run_batch(u, uo, nsteps=1, precond="spectral")
            iters += int(s.last_batch["iters"][0])
    finally:
        s.close()
    print(f"golden: {iters6} iterations, records {sp.RECORDS['golden']}")
    assert close(new.cpu().numpy()[0], z["U"][5].reshape(-1))
    assert torch.equal(u, new) and torch.equal(uo, prev) and iters == iters6
    assert abs(iters6 - sum(sp.RECORDS["golden"])) <= 2 * 6


B, NY, NX, H = 5, 64, 64, 0.0625


def ensemble():
    rng = np.random.default_rng(23)
    U, Uo = 0.5 * rng.standard_normal((B, NY * NX)), 0.5 * rng.standard_normal((B, NY * NX))
    return U, Uo, rng.uniform(0.05, 0.3, B), rng.integers(0, 2, B).astype(np.float64)


@gpu
def test_ensemble():
    import nkhip
    U, Uo, r, g = ensemble()
    # rtol 1e-15: the last member (g = 1, min D = -0.085) amplifies its residual a thousandfold --
    # NumPy's float64 pcg stopped at 1e-14 lands 1.14e-11 max|ref| from the reference on it (1.1e-12
    # at 1e-15; 7e-13 to 1.6e-12 on the g = 0 members either way), so there the stopping rule, not
    # the arithmetic, would set the distance that the 1e-11 bound measures
    s = stepper(NY, NX, H, rtol=1e-15)
    try:
        u = s.step_batch(U, Uo, r=r, g=g, precond="spectral")
        assert torch.equal(u, s.step_batch(U, Uo, r=r, g=g, precond="spectral"))
        solo = [s.step_batch(U[b], Uo[b], r=r[b:b + 1], g=g[b:b + 1], precond="spectral")[0]
                for b in range(B)]
    finally:
        s.close()
    assert torch.equal(u, torch.stack(solo))
    for b in range(B):
        assert close(u[b].cpu().numpy(), ref_solve(U[b], Uo[b], NY, NX, H, r[b], g[b])), b
    s = stepper(NY, NX, H, maxiter=2)
    try:
        with pytest.raises(nkhip.NoConvergence):
            s.step_batch(U, Uo, r=r, g=g, precond="spectral")
        assert s.last_batch["status"].tolist() == [nkhip._lib.NK_NO_CONVERGENCE] * B
        assert s.last_batch["iters"].tolist() == [2] * B
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("fault", ["nan", "kr2"])
def test_member_isolation(fault):
    """A member with a NaN, or with k r_m >= 2, stops before its first step; the others go on."""
    import nkhip
    U, Uo, r, g = ensemble()
    Ub, rb = U.copy(), r.copy()
    if fault == "nan":
        Ub[2, 1000] = np.nan
    else:
        rb[2] = 2.0 / K
    s = stepper(NY, NX, H)
    try:
        for nsteps in (1, 3):
            solo = [s.run_batch(U[b], Uo[b], nsteps, r[b:b + 1], g[b:b + 1], "spectral")[0][0]
                    for b in (0, 1, 3, 4)]
            with pytest.raises(ValueError, match="non-finite"):
                s.run_batch(Ub, Uo, nsteps, rb, g, "spectral")
            lb, got = s.last_batch, s.last_batch_state[0]
            assert lb["status"].tolist() == [0, 0, nkhip._lib.NK_NONFINITE, 0, 0]
            assert lb["steps"].tolist() == [nsteps, nsteps, 0, nsteps, nsteps]
            assert torch.equal(got[[0, 1, 3, 4]], torch.stack(solo)), nsteps
            if fault == "kr2":  # its outputs are its inputs
                assert np.array_equal(got[2].cpu().numpy(), U[2]) and int(lb["iters"][2]) == 0
    finally:
        s.close()


@gpu
def test_off_is_exact():
    z = load_golden("shlin_steps")
    U = z["U0"].reshape(-1)
    s, t = stepper(64, 64, 0.625), stepper(64, 64, 0.625, precond="spectral")
    try:
        a = s.run_batch(U, nsteps=2)
        plain_iters = s.last_batch["iters"].clone()
        b = s.run_batch(U, nsteps=2, precond=None)
        s.run_batch(U, precond="spectral")
        assert int(s.last_batch["precond"][0]) > 0 and float(s.last_batch["shift"][0]) > 0
        c = s.run_batch(U, nsteps=2, precond="none")
        assert int(s.last_batch["precond"][0]) == 0 and float(s.last_batch["shift"][0]) == 0
        d = t.run_batch(U, nsteps=2)  # set_precond has no say here: plain CG
        assert torch.equal(t.last_batch["iters"], plain_iters)
        for other in (b, c, d):
            assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    finally:
        s.close()
        t.close()


def test_cap():
    import nkhip
    assert nkhip.SHLinearised.resident_precond_max_points == 8192


@gpu
@pytest.mark.parametrize("ny,nx,precond", [(96, 96, "spectral"), (61, 61, "spectral"),
                                           (8, 5, "spectral"), (128, 128, "spectral"),
                                           (64, 64, "spectral-mixed")])
def test_refusals(ny, nx, precond):
    import nkhip
    rng = np.random.default_rng(3)
    U = 0.5 * rng.standard_normal(ny * nx)
    s = stepper(ny, nx, 0.625)
    try:
        with pytest.raises((nkhip.NKError, ValueError)):
            s.run_batch(U, precond=precond)
        if ny * nx <= nkhip.SHLinearised.resident_max_points:  # still a plain resident stepper
            s.run_batch(U)
            assert int(s.last_batch["status"][0]) == 0
        u = s.step(U, U).cpu().numpy()  # and an ordinary one
        assert np.isfinite(u).all() and s.last_relres <= 1e-14
    finally:
        s.close()
