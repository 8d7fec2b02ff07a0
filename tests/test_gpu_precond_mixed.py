"""GPU: the spectral preconditioner on grid sides 2^a 3^b 5^c, the kind "spectral-mixed"
(NK_PC_SPECTRAL_MIXED; csrc/fftpc_mixed.hip), and the solves that use it.

Bounds, those of the existing preconditioner tests:
* against the longdouble dense-DFT reference (precond_ref.py, sides up to 256): max(4 x NumPy's
  double-FFT score on the same input, 1e-13), the rule of test_gpu_precond.py;
* sides above 256 (test_gpu_precond_large.py): 1e-13 against NumPy's realisation, and the inverse
  identity |z/K - L z/2 - v| / |v| (L from ops.sh13_apply) at most 4 x NumPy's own.  The two pure
  Nyquist modes are held to 1e-13 against their closed form instead: each is an eigenvector of A0,
  so M v = v / A0^(Nyquist), and on sides 2^a 3^b 5^c NumPy itself misses 1e-13 on them
  (profiles/precond_mixed.md);
* the fused dot: |dot - sum w_i z_ref,i (longdouble)| <= (1e-13 + n 2.2e-16) |w|_1 max|z_ref|
  (test_gpu_shlin_precond.py);
* the two solves: f_tol / lam_min(A0) between the steps with and without M (test_gpu_precond.py),
  1e-11 relative between the PCG and CG steps (test_gpu_shlin_precond.py).
Measured figures: profiles/precond_mixed.md.
"""
import numpy as np
import pytest
import torch

import precond_ref as pr

pytestmark = pytest.mark.gpu

H, R, K = 0.0625, 0.01, 0.2  # the bench constants: cond(A0) ~ 4e5
PARITY = 1e-13
EPS = float(np.finfo(np.float64).eps)
LD = pr.LD
# each the smallest grid at which one thing can go wrong: a single radix-3 stage and odd nx/2;
# a single radix-5 stage and 2 x 3; 3 x 3 with a twiddle between and 3 x 5; 5 x 5; radix 4 beside
# 3; all three factors with a ragged column tile and a ragged row group; one side a power of two.
# 24 x 18, 20 x 50, 80 x 96, 160 x 8 and 192 x 16 stand beside 30 x 18, 50 x 20, 90 x 96, 150 x 8 and
# 240 x 16 because NumPy alone misses 1e-13 on the latter (profiles/precond_mixed.md); three of
# those stay, for the column transforms of 3 x 5 and 5 x 5 and the two ragged edges at once: their
# bound carries NumPy's score on the same input
GRIDS = [(6, 6), (10, 12), (12, 10), (18, 30), (24, 18), (30, 18), (20, 50), (50, 20), (36, 60),
         (80, 96), (90, 96), (96, 90), (160, 8), (8, 150), (192, 16)]
LONG = [(8, 3072), (3072, 8), (8, 3750), (3840, 12)]


def _gpu(v):
    return torch.as_tensor(np.ascontiguousarray(v), device="cuda")


@pytest.mark.parametrize("ny,nx", GRIDS)
def test_operator_against_longdouble(ny, nx):
    import nkhip
    worst = 0.0
    for name, v in pr.inputs(ny, nx).items():
        ref = pr.precond_ld(v, H, R, K)
        e_np = pr.rel_err(pr.precond_np(v, H, R, K), ref)
        e = pr.rel_err(nkhip.ops.sh_precond(_gpu(v), H, R, K, mixed=True).cpu().numpy(), ref)
        print(f"{ny}x{nx} {name}: kernel {e:.2e}, numpy {e_np:.2e}")
        worst = max(worst, e)
        assert e <= max(4 * e_np, PARITY), (name, e, e_np)
    print(f"{ny}x{nx}: worst {worst:.2e}")


@pytest.mark.parametrize("ny,nx", [(18, 30), (96, 90)])
def test_shifted_operator_and_fused_dot(ny, nx):
    """M_sigma = ((1 + sigma) I - (k/2) L)^-1 = M(k / (1 + sigma)) / k, with w a third vector,
    then w = v, then in place."""
    import nkhip
    sigma = 0.37
    v = pr.inputs(ny, nx)["random"]
    zref = pr.precond_ld(v, H, R, K / (1.0 + sigma), keep=True) / LD(K)
    e_np = pr.rel_err(pr.precond_np(v, H, R, K / (1.0 + sigma)) / K, zref)
    n = ny * nx
    vg = _gpu(v)
    plain = nkhip.ops.shlin_precond(vg, H, R, K, sigma=sigma, mixed=True)
    e = pr.rel_err(plain.cpu().numpy(), zref)
    print(f"{ny}x{nx}: kernel {e:.2e}, numpy {e_np:.2e}")
    assert e <= max(4 * e_np, PARITY), (e, e_np)
    third = np.random.default_rng(5 + ny + 7 * nx).standard_normal((ny, nx))
    for name, w in {"third": third, "w=v": v}.items():
        ref = float((w.astype(LD) * zref).sum())
        bound = (1e-13 + n * 2.2e-16) * float(np.abs(w).sum()) * float(np.abs(zref).max())
        wg = vg if name == "w=v" else _gpu(w)
        z, dot = nkhip.ops.shlin_precond(vg, H, R, K, sigma=sigma, dot_with=wg, mixed=True)
        z2, dot2 = nkhip.ops.shlin_precond(vg, H, R, K, sigma=sigma, dot_with=wg, mixed=True)
        print(f"{ny}x{nx} {name}: dot {dot!r}, ref {ref!r}, err {abs(dot - ref):.2e}, "
              f"bound {bound:.2e}")
        assert torch.equal(z, plain) and torch.equal(z2, plain) and dot2 == dot
        assert abs(dot - ref) <= bound
    x = vg.clone()
    z3, dot3 = nkhip.ops.shlin_precond(x, H, R, K, sigma=sigma, dot_with=x, out=x, mixed=True)
    assert z3.data_ptr() == x.data_ptr() and torch.equal(x, plain) and dot3 == dot


def test_powers_of_two_are_routed_to_the_radix2_kernels():
    import nkhip
    v = _gpu(pr.inputs(16, 8)["random"])
    assert torch.equal(nkhip.ops.sh_precond(v, H, R, K, mixed=True),
                       nkhip.ops.sh_precond(v, H, R, K))
    a, da = nkhip.ops.shlin_precond(v, H, R, K, sigma=0.37, dot_with=v, mixed=True)
    b, db = nkhip.ops.shlin_precond(v, H, R, K, sigma=0.37, dot_with=v)
    assert torch.equal(a, b) and da == db


@pytest.mark.parametrize("ny,nx", LONG)
def test_long_sides(ny, nx):
    """3072 = 2^10 3, 3750 = 2 3 5^4 (nx/2 = 1875 odd), 3840 = 2^8 3 5 on a short other side."""
    import nkhip
    lam = pr.symbol(ny, nx, H, R, K)
    eigen = {"nyq_x": lam[0, nx // 2], "nyq_y": lam[ny // 2, 0]}
    for name, v in pr.inputs(ny, nx).items():
        z_np = pr.precond_np(v, H, R, K)
        z = nkhip.ops.sh_precond(_gpu(v), H, R, K, mixed=True).cpu().numpy()
        ref = (v / eigen[name]).astype(np.float64) if name in eigen else z_np
        e = pr.rel_err(z, ref)

        def ident(zz):
            Lz = nkhip.ops.sh13_apply(_gpu(zz), H, R).cpu().numpy()
            return pr.rel_err(zz / K - Lz / 2, v)

        i_k, i_np = ident(z), ident(z_np)
        print(f"{ny}x{nx} {name}: vs {'closed form' if name in eigen else 'numpy'} {e:.2e} "
              f"(numpy vs the same {pr.rel_err(z_np, ref):.2e}); identity kernel {i_k:.2e}, numpy {i_np:.2e}")
        assert e <= PARITY, (name, e)
        # NumPy scores exactly 0.0 on the pure Nyquist mode along y at 3072 x 8 (its z there is the
        # one correctly rounded quotient, and the identity returns v to the bit); four times nothing
        # is no tolerance, so the score counts as at least the half ulp the identity resolves
        assert i_k <= 4 * max(i_np, EPS / 2), (name, i_k, i_np)


def _start(ny, nx):
    """A seeded smooth start: M applied to the random field (M damps wavenumber by wavenumber, by up
    to cond(A0) ~ 4e5), scaled to amplitude 0.5."""
    z = pr.precond_np(pr.inputs(ny, nx)["random"], H, R, K)
    return _gpu(0.5 * z / np.abs(z).max())


def test_preconditioned_newton_krylov_step():
    import nkhip
    ny, nx = 60, 96
    kw = dict(N=nx, ny=ny, d=0.625 * nx)
    U = _start(ny, nx)
    plain = nkhip.SwiftHohenberg(**kw)
    Up = plain.step(U).cpu().numpy()
    sp = dict(plain.last_stats)
    plain.close()
    m = nkhip.SwiftHohenberg(inner_M="spectral-mixed", **kw)
    assert m.inner_M == "spectral-mixed"
    Um = m.step(U).cpu().numpy()
    st = dict(m.last_stats)
    tol = float(np.finfo(np.float64).eps) ** (1.0 / 3.0) / pr.lam_min(ny, nx, m.h, m.r, m.k)
    m.close()
    diff = float(np.abs(Um - Up).max())
    print(f"{ny}x{nx}: with M {st}, plain njvp {sp['njvp']}, |U_M - U_plain|inf {diff:.3e} "
          f"(tol {tol:.3e})")
    assert st["status"] == 0 and sp["status"] == 0
    assert diff <= tol, (diff, tol)
    assert st["n_precond"] > 0
    assert st["njvp"] < sp["njvp"], (st, sp)


def test_preconditioned_semi_implicit_step():
    import nkhip
    ny, nx = 60, 96
    U = _start(ny, nx).reshape(-1)
    s = nkhip.SHLinearised(N=nx, ny=ny, precond="spectral-mixed")
    plain = nkhip.SHLinearised(N=nx, ny=ny)
    try:
        assert s.precond == "spectral-mixed"
        a, b = s.step(U, U), plain.step(U, U)
        err = float((a - b).abs().max() / b.abs().max())
        print(f"{ny}x{nx}: PCG {s.last_iters}, CG {plain.last_iters}, M applications "
              f"{s.last_precond}, shift {s.last_shift:.6g}, PCG vs CG {err:.2e}")
        assert s.last_relres <= 1e-14 and err <= 1e-11, (s.last_relres, err)
        assert 0 < s.last_precond and s.last_iters < plain.last_iters
    finally:
        s.close()
        plain.close()


@pytest.mark.parametrize("case", ["ny61", "ny14", "ny45", "ny6144", "kr2"])
def test_refusals(case):
    """A prime side, a factor 7, an odd side, a side above 4096 that is no power of two, k r >= 2."""
    import nkhip
    kw = {"ny61": dict(ny=61), "ny14": dict(ny=14), "ny45": dict(ny=45), "ny6144": dict(ny=6144),
          "kr2": dict(ny=60, r=10.0)}[case]
    kw = dict(N=96, d=0.625 * 96, k=0.2, **kw)
    with pytest.raises(nkhip.NKError):
        nkhip.SwiftHohenberg(inner_M="spectral-mixed", **kw)
    with pytest.raises(nkhip.NKError):
        nkhip.SHLinearised(precond="spectral-mixed", **kw)
    m = nkhip.SwiftHohenberg(**kw)
    try:
        zero = torch.zeros(m.ny, m.nx, dtype=torch.float64, device="cuda")
        with pytest.raises(nkhip.NKError):
            m.set_precond("spectral-mixed")
        with pytest.raises(nkhip.NKError):
            nkhip.ops.sh_precond(zero, m.h, m.r, m.k, mixed=True)
        with pytest.raises(nkhip.NKError):
            nkhip.ops.shlin_precond(zero, m.h, m.r, m.k, mixed=True)
        U = m.step(zero)  # still usable: one more step from the zero state (a root)
        assert m.last_stats["status"] == 0 and float(U.abs().max()) == 0.0
        assert m.last_stats["n_precond"] == 0 and m.inner_M is None
    finally:
        m.close()
