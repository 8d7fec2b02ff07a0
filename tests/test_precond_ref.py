"""CPU: the NumPy restatements of the spectral preconditioner M = (I/k - L/2)^-1 (precond_ref.py).

The longdouble reference is checked against the extended-precision 13-point stencil of
oracle/stencil_ref.py (A0 (M v) = v), for symmetry, and as SciPy's own ``inner_M``: SciPy's
newton_krylov with it converges on the 64 x 64 fixture state, and its Newton iteration and
F-evaluation counts are the records the GPU test compares against (precond_ref.SCIPY_WITH_M).
"""
import numpy as np
import pytest

import precond_ref as pr
from conftest import load_golden
from oracle import sh_oracle, stencil_ref

GRIDS = [(8, 8), (16, 8), (8, 16), (64, 64), (128, 64), (64, 256)]
H, R, K = 0.0625, 0.01, 0.2  # the bench constants: cond(A0) ~ 4e5


def _A0(w, h, r, k):
    """A0 w = w/k - L w/2 with L from the extended-precision stencil reference."""
    w = np.asarray(w, dtype=pr.LD)
    return w / pr.LD(k) - stencil_ref.sh13(w, h, r)[0] / 2


@pytest.mark.parametrize("ny,nx", GRIDS)
def test_inverse_identity(ny, nx):
    """A0 (M v) = v.  Everything is longdouble (eps 1.1e-19); the stencil sums 13 terms of size
    |L| ~ 2 lam_max |z| and M divides by at least lam_min, so the identity holds to about
    cond(A0) eps ~ 4e5 * 1.1e-19 = 4e-14 of |v|; 1e-13 (the project's operator parity bound)
    covers it with the transforms' own rounding."""
    for name, v in pr.inputs(ny, nx).items():
        z = pr.precond_ld(v, H, R, K, keep=True)
        err = pr.rel_err(_A0(z, H, R, K), v.astype(pr.LD))
        assert err <= 1e-13, (name, err)


@pytest.mark.parametrize("ny,nx", GRIDS)
def test_symmetry(ny, nx):
    """<M v, w> = <v, M w>: the symbol is real and even."""
    rng = np.random.default_rng(7)
    v, w = rng.standard_normal((2, ny, nx))
    Mv, Mw = pr.precond_ld(v, H, R, K, keep=True), pr.precond_ld(w, H, R, K, keep=True)
    a, b = float((Mv * w).sum()), float((v * Mw).sum())
    scale = float(np.sqrt((Mv * Mv).sum() * (w * w).sum()))
    assert abs(a - b) <= 1e-15 * scale, (a, b, scale)


def test_double_fft_realisation_close_to_reference():
    """NumPy's double FFT realisation, the GPU kernel's yardstick, against the reference."""
    for ny, nx in GRIDS:
        for name, v in pr.inputs(ny, nx).items():
            err = pr.rel_err(pr.precond_np(v, H, R, K), pr.precond_ld(v, H, R, K))
            assert err <= 1e-13, (ny, nx, name, err)


def test_lam_min():
    assert pr.lam_min(64, 64, 0.625, 0.01, 0.2) >= 1 / 0.2 - 0.01 / 2
    assert pr.lam_min(64, 64, H, R, K) >= 1 / K - R / 2


def scipy_solve(ny, nx):
    """SciPy's newton_krylov with inner_M = the longdouble M, from start_state(ny, nx)."""
    from scipy.optimize import newton_krylov
    from scipy.sparse.linalg import LinearOperator
    z = load_golden("nk_n64_default")
    h, r, k, g = (float(z[q]) for q in "hrkg")
    U0 = pr.start_state(z["traj"][0], ny, nx).reshape(-1)
    calls, its = [0], [0]

    def F(u):
        calls[0] += 1
        return sh_oracle.residual(u, U0, ny, nx, h, r, k, g)

    M = LinearOperator((ny * nx, ny * nx), dtype=np.float64,
                       matvec=lambda v: pr.precond_ld(v.reshape(ny, nx), h, r, k).reshape(-1))

    def cb(x, f):
        its[0] += 1

    U = newton_krylov(F, U0, inner_M=M, callback=cb)
    return U, U0, its[0], calls[0], (h, r, k, g)


@pytest.mark.parametrize("ny,nx", [(64, 64), (128, 64)])
def test_scipy_converges_with_M(ny, nx):
    U, U0, nit, nfev, (h, r, k, g) = scipy_solve(ny, nx)
    res = np.abs(sh_oracle.residual(U, U0, ny, nx, h, r, k, g)).max()
    assert res <= 6.06e-6, res  # scipy's default f_tol = eps^(1/3)
    print(f"{ny}x{nx}: scipy with M: nit {nit}, F calls {nfev}, |F|inf {res:.3e}")
    rec = pr.SCIPY_WITH_M[(ny, nx)]
    assert nit == rec["nit"], (nit, rec)
    # F calls: the record, give or take the one LGMRES step FD rounding can move
    assert abs(nfev - rec["nfev"]) <= 1, (nfev, rec)
