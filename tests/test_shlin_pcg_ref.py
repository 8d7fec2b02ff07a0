"""CPU: the NumPy restatement of the stepper's preconditioned CG solve (shlin_pcg_ref.py).

* shift_ld, the longdouble reference of M_sigma = ((1 + sigma) I - (k/2) L)^-1, against a direct
  longdouble evaluation of the symbol on 8 x 8 and 16 x 8;
* the restatement's iteration counts are the records the GPU test compares with;
* its solutions against the reference's direct solve (oracle.shlin_oracle.step, spsolve) on the
  square cases: measured <= 1.7e-12 of max|ref| (stiff64), bound 1e-11 (the parity bound of
  tests/test_gpu_shlin.py).
"""
import numpy as np
import pytest

import precond_ref as pr
import shlin_pcg_ref as sp
from conftest import load_golden
from oracle import shlin_oracle
from oracle.sh_oracle import csr_L

LD = pr.LD


@pytest.mark.parametrize("ny,nx", [(8, 8), (16, 8)])
@pytest.mark.parametrize("sigma", [0.0, 0.37, 9.0])
def test_shift_ld_is_the_shifted_symbol(ny, nx, sigma):
    """DFT, divide by (1 + sigma) - (k/2) L^ written out directly, inverse DFT, all in
    longdouble (eps 1.1e-19): the two differ by a few roundings of cond ~ 1e5-sized quotients."""
    h, r, k = 0.0625, 0.2, 0.2
    sym = (1 + LD(sigma)) - LD(k) / 2 * sp.lhat(ny, nx, h, r)
    assert float(sym.min()) > 0
    Wy, Wx = pr.dft_ld(ny), pr.dft_ld(nx)
    for name, v in pr.inputs(ny, nx).items():
        V = Wy @ v.astype(pr.CLD) @ Wx
        direct = (np.conj(Wy) @ (V / sym) @ np.conj(Wx)).real / LD(nx * ny)
        got = sp.shift_ld(v, h, r, k, sigma, keep=True)
        assert pr.rel_err(got, direct) <= 1e-17, (name, pr.rel_err(got, direct))
        assert pr.rel_err(sp.shift_np(v, h, r, k, sigma), direct) <= 1e-13, name


def test_shift_zero_is_the_newton_krylov_operator():
    v = pr.inputs(16, 8)["random"]
    a = sp.shift_ld(v, 0.0625, 0.2, 0.2, 0.0, keep=True)
    b = pr.precond_ld(v, 0.0625, 0.2, 0.2, keep=True) / LD(0.2)
    assert pr.rel_err(a, b) <= 1e-18


@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_records(name):
    U, Uo, ny, nx, h, g = sp.state(name)
    x, it, sigma, relres, napp = sp.pcg(U, Uo, ny, nx, h, g=g)
    print(f"{name}: PCG its {it}, sigma {sigma:.6g}, relres {relres:.2e}, M applications {napp}")
    assert it == sp.RECORDS[name], (it, sp.RECORDS[name])
    assert relres <= sp.RTOL and napp == it
    if name == "negD64":
        D = sp.diag(U, Uo, sp.K, g)
        assert D.mean() < 0 and sigma == 0.0
    if ny == nx:
        ref = shlin_oracle.step(csr_L(nx, h, sp.R).tocsc(), U, Uo, sp.K, g)
        err = np.abs(x - ref).max() / np.abs(ref).max()
        print(f"{name}: vs spsolve {err:.2e}")
        assert err <= 1e-11, err


def test_records_golden_steps():
    z = load_golden("shlin_steps")
    N, d, k, r, g = int(z["N"]), float(z["d"]), float(z["k"]), float(z["r"]), float(z["g"])
    U = Uo = np.asarray(z["U0"], dtype=np.float64).reshape(-1)
    its = []
    for ref in z["U"]:
        x, it, sigma, relres, _ = sp.pcg(U, Uo, N, N, d / N, r=r, k=k, g=g)
        assert np.abs(x - ref.reshape(-1)).max() <= 1e-11 * np.abs(ref).max()
        assert relres <= sp.RTOL
        its.append(it)
        U, Uo = x, U
    assert its == sp.RECORDS["golden"], its


def test_plain_cg_needs_far_more():
    """The case the option is for: without M the refined grid does not converge in the stepper's
    default 1000 iterations."""
    U, Uo, ny, nx, h, g = sp.state("stiff64")
    _, it, _, relres, _ = sp.pcg(U, Uo, ny, nx, h, g=g, precond=False)
    assert it == 1000 and relres > sp.RTOL
    U, Uo, ny, nx, h, g = sp.state("small8")
    _, it, _, _, _ = sp.pcg(U, Uo, ny, nx, h, g=g, precond=False)
    assert abs(it - sp.CG_RECORDS["small8"]) <= 2
