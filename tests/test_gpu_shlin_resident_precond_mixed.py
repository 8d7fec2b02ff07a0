"""GPU: SHLinearised.run_batch(precond="spectral-mixed"), the resident preconditioned CG on grids
whose sides are 2^a 3^b 5^c (csrc/shlin_resident_pcm.hip: wave-local mixed-radix transforms).

Reference and bounds are those of tests/test_gpu_shlin_resident_precond.py: the longdouble PCG
(ref_solve), max|u - ref| <= 1e-11 max|ref|, the oracle's |b - A u| / |b| <= 2e-14, iterations
within 2 of shlin_pcg_ref.pcg on the same state, sigma within 1e-14 relative.  NumPy's pcg itself
sits at most 2.7e-12 max|ref| from the reference on these shapes, with an oracle residual of at
most 4e-15."""
import numpy as np
import pytest
import torch

import shlin_pcg_ref as sp
from test_gpu_shlin_resident_precond import close, ref_solve, stepper

gpu = pytest.mark.gpu
K, R = sp.K, sp.R
MIXED = "spectral-mixed"
# (ny, nx, h, g): see the kernel's header for what each shape reaches
CASES = [(6, 6, 0.625, 0), (10, 6, 0.0625, 0), (12, 18, 0.0625, 0), (30, 50, 0.0625, 0),
         (48, 80, 0.0625, 0), (64, 96, 0.0625, 0), (100, 90, 0.0625, 0), (96, 96, 0.0625, 0),
         (96, 96, 0.625, 1), (128, 72, 0.0625, 0), (72, 128, 0.0625, 0)]


def state(ny, nx, g=0, B=None):
    """0.5 standard_normal, or shlin_pcg_ref's negD64 recipe where g = 1."""
    rng = np.random.default_rng(1000 * ny + nx)
    shape = ny * nx if B is None else (B, ny * nx)
    if g:
        U = 0.5 + 0.05 * rng.standard_normal(shape)
        return U, U + 0.01 * rng.standard_normal(shape)
    return 0.5 * rng.standard_normal(shape), 0.5 * rng.standard_normal(shape)


@gpu
@pytest.mark.parametrize("ny,nx,h,g", CASES)
def test_one_step_against_reference(ny, nx, h, g):
    U, Uo = state(ny, nx, g)
    record = sp.pcg(U, Uo, ny, nx, h, g=g)[1]
    s = stepper(ny, nx, h, g)
    try:
        u = s.step_batch(U, Uo, precond=MIXED).cpu().numpy()[0]
        lb = s.last_batch
    finally:
        s.close()
    its, napp, shift = int(lb["iters"][0]), int(lb["precond"][0]), float(lb["shift"][0])
    A, b, _ = sp.system(U, Uo, ny, nx, h, R, K, g)
    rel = float(np.sqrt(((b - A(u)) ** 2).sum()) / np.sqrt(b @ b))
    want = float(sp.shift(U, Uo, K, g))
    print(f"{ny}x{nx}: PCG {its} (numpy {record}), M applications {napp}, oracle relres "
          f"{rel:.2e}, shift {shift!r} (numpy {want!r})")
    assert close(u, ref_solve(U, Uo, ny, nx, h, R, g))
    assert rel <= 2e-14
    assert int(lb["status"][0]) == 0 and int(lb["steps"][0]) == 1
    assert abs(its - record) <= 2 and its <= napp <= its + 1
    assert abs(shift - want) <= 1e-14 * want
    if g:
        assert shift == 0.0


@gpu
def test_ensemble():
    B, ny, nx, h = 5, 30, 50, 0.0625
    U, Uo = state(ny, nx, B=B)
    rng = np.random.default_rng(23)
    r, g = rng.uniform(0.05, 0.3, B), rng.integers(0, 2, B).astype(np.float64)
    s = stepper(ny, nx, h, rtol=1e-15)  # the power-of-two ensemble test says why
    try:
        u = s.step_batch(U, Uo, r=r, g=g, precond=MIXED)
        assert torch.equal(u, s.step_batch(U, Uo, r=r, g=g, precond=MIXED))
        solo = [s.step_batch(U[b], Uo[b], r=r[b:b + 1], g=g[b:b + 1], precond=MIXED)[0]
                for b in range(B)]
    finally:
        s.close()
    assert torch.equal(u, torch.stack(solo))
    for b in range(B):
        assert close(u[b].cpu().numpy(), ref_solve(U[b], Uo[b], ny, nx, h, r[b], g[b])), b


@gpu
def test_steps_in_one_launch_and_global_kernels():
    ny, nx, h = 96, 96, 0.0625
    U, _ = state(ny, nx)
    s, t = stepper(ny, nx, h), stepper(ny, nx, h, precond=MIXED)
    try:
        new, prev = s.run_batch(U, nsteps=3, precond=MIXED)
        iters3 = int(s.last_batch["iters"][0])
        assert int(s.last_batch["steps"][0]) == 3
        u, uo, iters = torch.as_tensor(U), None, 0
        for _ in range(3):
            u, uo = s.run_batch(u, uo, nsteps=1, precond=MIXED)
            iters += int(s.last_batch["iters"][0])
        assert torch.equal(u, new) and torch.equal(uo, prev) and iters == iters3
        v = t.run(U, 3)[-1].cpu().numpy()  # three `step` calls: the global mixed-radix kernels
    finally:
        s.close()
        t.close()
    assert close(new.cpu().numpy()[0], v)


@gpu
@pytest.mark.parametrize("ny,nx", [(14, 12), (9, 12), (96, 100), (160, 48)])
def test_refusals(ny, nx):
    import nkhip
    U, _ = state(ny, nx)
    s = stepper(ny, nx, 0.625)
    try:
        with pytest.raises((nkhip.NKError, ValueError)):
            s.run_batch(U, precond=MIXED)
        if ny * nx <= nkhip.SHLinearised.resident_max_points:  # still a plain resident stepper
            s.run_batch(U)
            assert int(s.last_batch["status"][0]) == 0
        u = s.step(U, U).cpu().numpy()  # and an ordinary one
        assert np.isfinite(u).all() and s.last_relres <= 1e-14
    finally:
        s.close()


@gpu
def test_member_isolation():
    """A member with k r_m >= 2 never starts; the others equal their solo runs."""
    import nkhip
    ny, nx = 12, 18
    U, Uo = state(ny, nx, B=3)
    r = np.array([R, 2.0 / K, 0.1])
    s = stepper(ny, nx, 0.0625)
    try:
        solo = [s.run_batch(U[b], Uo[b], 1, r[b:b + 1], None, MIXED)[0][0] for b in (0, 2)]
        with pytest.raises(ValueError, match="non-finite"):
            s.run_batch(U, Uo, 1, r, None, MIXED)
        lb, got = s.last_batch, s.last_batch_state[0]
    finally:
        s.close()
    assert lb["status"].tolist() == [0, nkhip._lib.NK_NONFINITE, 0]
    assert lb["steps"].tolist() == [1, 0, 1] and int(lb["iters"][1]) == 0
    assert torch.equal(got[[0, 2]], torch.stack(solo))
    assert np.array_equal(got[1].cpu().numpy(), U[1])


def test_cap():
    import nkhip
    assert nkhip.SHLinearised.resident_precond_mixed_max_points == 9216
