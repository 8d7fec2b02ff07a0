"""GPU: the spectral preconditioner of the semi-implicit SH stepper's CG solve
(SHLinearised(precond="spectral"), ops.shlin_precond; csrc/shlin.cpp, csrc/fftpc.hip).

M_sigma = ((1 + sigma) I - (k/2) L)^-1 with sigma = max(mean(D), 0), the constant-coefficient part
of the step's matrix A = I + D - (k/2) L, applied in Fourier space; references and records in
shlin_pcg_ref.py (checked on the CPU by test_shlin_pcg_ref.py).

Operator bound: the rule of test_gpu_precond.py, max(4 x NumPy's double-FFT score on the same input,
1e-13) against the longdouble dense-DFT reference; 1e-13 against NumPy's realisation on the two
long grids.  Fused dot w.z: |dot - sum w_i z_ref,i (longdouble)| <= (1e-13 + n 2.2e-16) |w|_1
max|z_ref| -- 1e-13 is the operator bound on z, n eps the worst-case summation error in any order.
"""
import numpy as np
import pytest
import torch

import precond_ref as pr
import shlin_pcg_ref as sp
from conftest import load_golden
from oracle import shlin_oracle
from oracle.sh_oracle import csr_L

pytestmark = pytest.mark.gpu

H, R, K = 0.0625, 0.2, 0.2
GRIDS = [(8, 8), (16, 8), (8, 16), (64, 64), (128, 64), (64, 256)]
LONG = [(8, 4096), (4096, 8)]
SIGMAS = [0.0, 0.37, 9.0]
PARITY = 1e-13
LD = pr.LD


def _gpu(v):
    if isinstance(v, torch.Tensor):
        return v
    return torch.as_tensor(np.ascontiguousarray(v), device="cuda")


def _apply(v, sigma, **kw):
    import nkhip
    return nkhip.ops.shlin_precond(_gpu(v), H, R, K, sigma=sigma, **kw)


# ------------------------------------------------------------------------------- 1. operator
@pytest.mark.parametrize("ny,nx", GRIDS)
def test_operator_against_longdouble(ny, nx):
    import nkhip
    worst = 0.0
    for sigma in SIGMAS:
        for name, v in pr.inputs(ny, nx).items():
            ref = sp.shift_ld(v, H, R, K, sigma)
            e_np = pr.rel_err(sp.shift_np(v, H, R, K, sigma), ref)
            z = _apply(v, sigma).cpu().numpy()
            e = pr.rel_err(z, ref)
            print(f"{ny}x{nx} sigma {sigma} {name}: kernel {e:.2e}, numpy {e_np:.2e}")
            worst = max(worst, e)
            bound = max(4 * e_np, PARITY)
            assert e <= bound, (sigma, name, e, e_np)
            if sigma == 0.0:  # ties the new entry to the Newton-Krylov operator
                old = nkhip.ops.sh_precond(_gpu(v), H, R, K).cpu().numpy() / K
                assert pr.rel_err(z, old) <= bound, (name, pr.rel_err(z, old))
    print(f"{ny}x{nx}: worst {worst:.2e}")


@pytest.mark.parametrize("ny,nx", LONG)
def test_longest_transforms(ny, nx):
    import nkhip
    for sigma in SIGMAS:
        for name, v in pr.inputs(ny, nx).items():
            z = _apply(v, sigma).cpu().numpy()
            e = pr.rel_err(z, sp.shift_np(v, H, R, K, sigma))
            print(f"{ny}x{nx} sigma {sigma} {name}: vs numpy {e:.2e}")
            assert e <= PARITY, (sigma, name, e)
            if sigma == 0.0:
                old = nkhip.ops.sh_precond(_gpu(v), H, R, K).cpu().numpy() / K
                assert pr.rel_err(z, old) <= PARITY, (name, pr.rel_err(z, old))


# ------------------------------------------------------------------------------ 2. fused dot
@pytest.mark.parametrize("ny,nx", GRIDS + LONG)
def test_fused_dot(ny, nx):
    sigma = 0.37
    v = pr.inputs(ny, nx)["random"]
    w = np.random.default_rng(5 + ny + 7 * nx).standard_normal((ny, nx))
    vg, wg = _gpu(v), _gpu(w)
    plain = _apply(v, sigma)
    z, dot = _apply(v, sigma, dot_with=wg)
    assert torch.equal(z, plain)
    if max(ny, nx) <= 256:
        zref = sp.shift_ld(v, H, R, K, sigma, keep=True)
    else:
        zref = sp.shift_np(v, H, R, K, sigma).astype(LD)
    ref = float((w.astype(LD) * zref).sum())
    n = ny * nx
    bound = (1e-13 + n * 2.2e-16) * float(np.abs(w).sum()) * float(np.abs(zref).max())
    print(f"{ny}x{nx}: dot {dot!r}, ref {ref!r}, err {abs(dot - ref):.2e}, bound {bound:.2e}")
    assert abs(dot - ref) <= bound
    z2, dot2 = _apply(v, sigma, dot_with=wg)
    assert torch.equal(z2, z) and dot2 == dot
    x = vg.clone()
    z3, dot3 = _apply(x, sigma, dot_with=wg, out=x)
    assert z3.data_ptr() == x.data_ptr()
    assert torch.equal(x, z) and dot3 == dot


# ---------------------------------------------------------------------------------- 3. shift
@pytest.mark.parametrize("name", ["small8", "stiff128x64", "negD64"])
def test_shift(name):
    import nkhip
    U, Uo, ny, nx, h, g = sp.state(name)
    s = nkhip.SHLinearised(N=nx, ny=ny, d=nx * h, k=sp.K, r=sp.R, g=g, precond="spectral")
    try:
        s.step(U, Uo)
        want = float(sp.shift(U, Uo, sp.K, g, dtype=LD))
        print(f"{name}: last_shift {s.last_shift!r}, longdouble {want!r}")
        if name == "negD64":
            assert want == 0.0 and s.last_shift == 0.0
        else:
            assert abs(s.last_shift - want) <= 1e-14 * want
    finally:
        s.close()


def test_shift_reported_without_convergence():
    """A step that ends in NoConvergence still reports its sigma and its applications of M."""
    import nkhip
    U, Uo, ny, nx, h, g = sp.state("stiff64")
    s = nkhip.SHLinearised(N=nx, ny=ny, d=nx * h, k=sp.K, r=sp.R, g=g, precond="spectral",
                           maxiter=2)
    try:
        with pytest.raises(nkhip.NoConvergence):
            s.step(U, Uo)
        want = float(sp.shift(U, Uo, sp.K, g, dtype=LD))
        print(f"stiff64, maxiter 2: last_shift {s.last_shift!r}, longdouble {want!r}, "
              f"iterations {s.last_iters}, M applications {s.last_precond}")
        assert want > 0.0 and abs(s.last_shift - want) <= 1e-14 * want
        assert s.last_iters == 2 and s.last_precond == 3  # the start's and one per iteration
    finally:
        s.close()


# ------------------------------------------------------------------------ 4. reference parity
def test_golden_steps_with_preconditioner():
    import nkhip
    z = load_golden("shlin_steps")
    kw = dict(N=int(z["N"]), d=float(z["d"]), k=float(z["k"]), r=float(z["r"]), g=float(z["g"]))
    s = nkhip.SHLinearised(precond="spectral", **kw)
    plain = nkhip.SHLinearised(**kw)
    try:
        U = Uo = torch.as_tensor(z["U0"], device="cuda").reshape(-1)
        Up = Uop = U
        for i, ref in enumerate(z["U"]):
            U, Uo = s.step(U, Uo), U
            its, napp = s.last_iters, s.last_precond
            Up, Uop = plain.step(Up, Uop), Up
            err = np.abs(U.cpu().numpy() - ref.reshape(-1)).max() / np.abs(ref).max()
            print(f"step {i}: PCG {its} (record {sp.RECORDS['golden'][i]}), CG {plain.last_iters}, "
                  f"M applications {napp}, shift {s.last_shift:.6g}, relres {s.last_relres:.2e}, "
                  f"vs spsolve {err:.2e}")
            assert err <= 1e-11, (i, err)
            assert s.last_relres <= 1e-14
            assert abs(its - sp.RECORDS["golden"][i]) <= 2, (i, its)
            assert 4 * its < plain.last_iters, (i, its, plain.last_iters)
            assert its <= napp <= its + 1, (i, its, napp)
            assert plain.last_precond == 0 and plain.last_shift == 0.0
    finally:
        s.close()
        plain.close()


# ------------------------------------------------------------- 5. the case the option is for
def _oracle_relres(u, U, Uo, ny, nx, h, g):
    A, b, _ = sp.system(U, Uo, ny, nx, h, sp.R, sp.K, g)
    res = b - A(u)
    return float(np.sqrt(res @ res) / np.sqrt(b @ b))


def _spectral_step(name):
    import nkhip
    U, Uo, ny, nx, h, g = sp.state(name)
    s = nkhip.SHLinearised(N=nx, ny=ny, d=nx * h, k=sp.K, r=sp.R, g=g, precond="spectral")
    try:
        u = s.step(U, Uo).cpu().numpy()
        its, napp = s.last_iters, s.last_precond
    finally:
        s.close()
    rel = _oracle_relres(u, U, Uo, ny, nx, h, g)
    print(f"{name}: PCG {its} (record {sp.RECORDS[name]}), M applications {napp}, "
          f"oracle |b - A u|/|b| {rel:.2e}")
    assert abs(its - sp.RECORDS[name]) <= 2, its
    assert its <= napp <= its + 1
    return u, rel, (U, Uo, ny, nx, h, g)


def test_stiff_grid_needs_the_preconditioner():
    import nkhip
    U, Uo, ny, nx, h, g = sp.state("stiff64")
    plain = nkhip.SHLinearised(N=nx, ny=ny, d=nx * h, k=sp.K, r=sp.R, g=g)
    try:
        with pytest.raises(nkhip.NoConvergence):
            plain.step(U, Uo)
        assert plain.last_iters == 1000
    finally:
        plain.close()
    u, rel, _ = _spectral_step("stiff64")
    assert rel <= 2e-14, rel
    ref = shlin_oracle.step(csr_L(nx, h, sp.R).tocsc(), U, Uo, sp.K, g)
    err = np.abs(u - ref).max() / np.abs(ref).max()
    print(f"stiff64: vs spsolve {err:.2e}")
    assert err <= 1e-11, err


@pytest.mark.parametrize("name", ["stiff128x64", "small16x8"])
def test_stiff_counts_and_residual(name):
    _, rel, _ = _spectral_step(name)
    assert rel <= 2e-14, rel


# ---------------------------------------------------------------------------------- 6. g != 0
def test_negative_mean_diagonal():
    u, rel, (U, Uo, ny, nx, h, g) = _spectral_step("negD64")
    assert rel <= 2e-14, rel
    ref = shlin_oracle.step(csr_L(nx, h, sp.R).tocsc(), U, Uo, sp.K, g)
    err = np.abs(u - ref).max() / np.abs(ref).max()
    print(f"negD64: vs spsolve {err:.2e}")
    assert err <= 1e-11, err


# ------------------------------------------------------------------------------ 7. off is exact
def test_off_is_exact():
    import nkhip
    z = load_golden("shlin_steps")
    kw = dict(N=int(z["N"]), d=float(z["d"]), k=float(z["k"]), r=float(z["r"]), g=float(z["g"]))
    U = torch.as_tensor(z["U"][2], device="cuda").reshape(-1)
    Uo = torch.as_tensor(z["U"][1], device="cuda").reshape(-1)
    never = nkhip.SHLinearised(**kw)
    s = nkhip.SHLinearised(**kw)
    try:
        a = never.step(U, Uo)
        s.set_precond("spectral")
        assert s.precond == "spectral"
        s.step(U, Uo)
        assert s.last_precond > 0 and s.last_shift > 0
        s.set_precond(None)
        assert s.precond is None
        b = s.step(U, Uo)
        assert torch.equal(a, b)
        assert s.last_iters == never.last_iters and s.last_relres == never.last_relres
        assert s.last_precond == 0 and s.last_shift == 0.0
        s.set_precond(nkhip._lib.NK_PC_SPECTRAL)  # by code, as SwiftHohenberg.set_precond
        s.step(U, Uo)
        assert s.last_precond > 0
    finally:
        never.close()
        s.close()


# -------------------------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("case", ["nx96", "ny61", "kr2"])
def test_refusals(case):
    import nkhip
    kw = {"nx96": dict(N=96, ny=64, d=0.625 * 96), "ny61": dict(N=64, ny=61, d=40.0),
          "kr2": dict(N=64, d=40.0, k=0.2, r=10.0)}[case]
    with pytest.raises(nkhip.NKError):
        nkhip.SHLinearised(precond="spectral", **kw)
    s = nkhip.SHLinearised(**kw)
    try:
        with pytest.raises(nkhip.NKError):
            s.set_precond("spectral")
        assert s.precond is None
        zero = torch.zeros(s.ny, s.N, dtype=torch.float64, device="cuda")
        with pytest.raises(nkhip.NKError):
            nkhip.ops.shlin_precond(zero, s.h, s.r, s.k)
        out = s.step(zero, zero)
        assert float(out.abs().max()) == 0.0
        assert s.last_iters == 0 and s.last_precond == 0 and s.last_shift == 0.0
    finally:
        s.close()
