"""GPU: the spectral preconditioner M = (I/k - L/2)^-1 (csrc/fftpc.hip) and the solves that use it.

Operator bound (max-norm of the error over max-norm of the reference): NumPy's double-precision
FFT realisation of M scores, against the longdouble dense-DFT reference (precond_ref.py) over the
test inputs,
    8x8 6.8e-16, 16x8 6.1e-16, 8x16 5.4e-16, 64x64 2.2e-15, 128x64 3.1e-15, 64x256 3.1e-15;
the kernel is allowed 4x that or the project's operator parity bound 1e-13, whichever is larger --
1e-13 on every grid here.  The kernel itself measured (MI355X), worst input per grid:
    8x8 6.8e-16, 16x8 6.2e-16, 8x16 5.4e-16, 64x64 5.9e-15, 128x64 9.8e-15, 64x256 9.8e-15
(on the larger grids the random field and the one-hots: the kernel forms 2 cos + 2 cos - 4 from
double-precision cosines, which loses digits at the lowest wavenumbers; NumPy's yardstick takes
the symbol from longdouble);
    8x4096 and 4096x8 against NumPy's realisation: 1.4e-14 and 7.6e-15 (random field).
Inverse identity A0 (M v) = v through ops.sh13_apply on the longest transforms, kernel / NumPy:
random 3.6e-12 / 3.4e-12 (8x4096) and 3.7e-12 / 3.6e-12 (4096x8), one-hots 4.5e-13 / 3.1e-13 at
worst, constant 1.6e-11 / 1.6e-11 (cond(A0) ~ 4e5 amplifies the rounding of z); the bound is 4x
NumPy's score on the same input.
"""
import math

import numpy as np
import pytest
import torch

import precond_ref as pr
from conftest import load_golden, run_slabs
from oracle import sh_oracle

pytestmark = pytest.mark.gpu

H, R, K = 0.0625, 0.01, 0.2  # the bench constants: cond(A0) ~ 4e5
GRIDS = [(8, 8), (16, 8), (8, 16), (64, 64), (128, 64), (64, 256)]
LONG = [(8, 4096), (4096, 8)]
PARITY = 1e-13  # the project's operator parity bound


def _gpu(v):
    return torch.as_tensor(np.ascontiguousarray(v), device="cuda")


def _apply(v):
    import nkhip
    return nkhip.ops.sh_precond(_gpu(v), H, R, K).cpu().numpy()


@pytest.mark.parametrize("ny,nx", GRIDS)
def test_operator_against_longdouble(ny, nx):
    worst = 0.0
    for name, v in pr.inputs(ny, nx).items():
        ref = pr.precond_ld(v, H, R, K)
        e_np = pr.rel_err(pr.precond_np(v, H, R, K), ref)
        e = pr.rel_err(_apply(v), ref)
        print(f"{ny}x{nx} {name}: kernel {e:.2e}, numpy {e_np:.2e}")
        worst = max(worst, e)
        assert e <= max(4 * e_np, PARITY), (name, e, e_np)
    print(f"{ny}x{nx}: worst {worst:.2e}")


@pytest.mark.parametrize("ny,nx", LONG)
def test_longest_transforms(ny, nx):
    """4096-long rows / columns on 8 of the other.  No longdouble reference at this length: the
    kernel is compared with NumPy's realisation, whose own error (3.1e-15 at most on the small
    grids, growing with log n) is far inside the 1e-13 the rule above allows; and both are put
    through the same inverse identity, v = A0 z with L from ops.sh13_apply."""
    import nkhip
    for name, v in pr.inputs(ny, nx).items():
        z_np = pr.precond_np(v, H, R, K)
        z = _apply(v)
        e = pr.rel_err(z, z_np)

        def ident(zz):
            Lz = nkhip.ops.sh13_apply(_gpu(zz), H, R).cpu().numpy()
            return pr.rel_err(zz / K - Lz / 2, v)

        i_k, i_np = ident(z), ident(z_np)
        print(f"{ny}x{nx} {name}: vs numpy {e:.2e}; identity kernel {i_k:.2e}, numpy {i_np:.2e}")
        assert e <= PARITY, (name, e)
        assert i_k <= 4 * i_np, (name, i_k, i_np)


@pytest.mark.parametrize("ny,nx", [(64, 256), (8, 4096), (4096, 8)])
def test_deterministic_and_in_place(ny, nx):
    import nkhip
    v = _gpu(pr.inputs(ny, nx)["random"])
    a = nkhip.ops.sh_precond(v, H, R, K)
    b = nkhip.ops.sh_precond(v, H, R, K)
    assert torch.equal(a, b)
    w = v.clone()
    nkhip.ops.sh_precond(w, H, R, K, out=w)
    assert torch.equal(a, w)


def _usable(m, ny, nx):
    """One more step from the zero state (a root: F(0) = 0) still runs."""
    U = m.step(torch.zeros(ny, nx, dtype=torch.float64, device="cuda"))
    assert m.last_stats["status"] == 0 and float(U.abs().max()) == 0.0
    assert m.last_stats["n_precond"] == 0 and m.inner_M is None


@pytest.mark.parametrize("case", ["nx96", "ny61", "kr2"])
def test_refusals(case):
    import nkhip
    kw = {"nx96": dict(N=96, ny=64, d=0.625 * 96), "ny61": dict(N=64, ny=61, d=40.0),
          "kr2": dict(N=64, d=40.0, k=0.2, r=10.0)}[case]
    with pytest.raises(nkhip.NKError):
        nkhip.SwiftHohenberg(inner_M="spectral", **kw)
    m = nkhip.SwiftHohenberg(**kw)
    with pytest.raises(nkhip.NKError):
        m.set_precond("spectral")
    with pytest.raises(nkhip.NKError):
        nkhip.ops.sh_precond(torch.zeros(m.ny, m.nx, dtype=torch.float64, device="cuda"),
                             m.h, m.r, m.k)
    _usable(m, m.ny, m.nx)
    m.close()


def test_refusal_with_communicator():
    """A slab stepper with a communicator (a loopback world of one) has no spectral M."""
    import nkhip
    comms = nkhip.loopback_comms(1)

    def run(p):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            m = nkhip.SwiftHohenberg(N=64, d=40.0, comm=comms[p], ny_local=64, stream=stream)
            with pytest.raises(nkhip.NKError):
                m.set_precond("spectral")
            _usable(m, 64, 64)
            stream.synchronize()
            m.close()

    run_slabs(comms, run)


def _start(ny):
    z = load_golden("nk_n64_default")
    U0 = pr.start_state(z["traj"][0], ny, 64)
    return z, U0, tuple(float(z[q]) for q in "hrkg")


def test_switching_back_is_exact():
    import nkhip
    z, U0, (h, r, k, g) = _start(64)
    m = nkhip.SwiftHohenberg(N=64, d=float(z["d"]), k=k, r=r, g=g)
    U = _gpu(U0)
    a = m.step(U).clone()
    sa = dict(m.last_stats)
    m.set_precond(nkhip._lib.NK_PC_SPECTRAL)
    m.step(U)
    assert m.last_stats["n_precond"] > 0
    m.set_precond(nkhip._lib.NK_PC_NONE)
    b = m.step(U)
    sb = dict(m.last_stats)
    m.close()
    assert torch.equal(a, b)
    assert sa == sb, (sa, sb)
    assert sb["n_precond"] == 0


@pytest.mark.parametrize("ny", [64, 128])
def test_preconditioned_step(ny):
    """One Crank-Nicolson step with inner_M='spectral' from the 64 x 64 fixture state (tiled in y
    for 128 x 64), SciPy's default f_tol.

    Two roots to f_tol: F(u1) - F(u2) = J (u1 - u2) to first order, |F(u_i)|inf <= f_tol, and the
    Jacobian's linear part A0 = I/k - L/2 has no eigenvalue below lam_min(A0), so the steps may
    differ by f_tol / lam_min(A0) (about 6.06e-6 / 5 = 1.2e-6 here).
    """
    import nkhip
    z, U0, (h, r, k, g) = _start(ny)
    f_tol = float(np.finfo(np.float64).eps) ** (1.0 / 3.0)
    U = _gpu(U0)
    plain = nkhip.SwiftHohenberg(N=64, ny=ny, d=float(z["d"]), k=k, r=r, g=g)
    Up = plain.step(U).cpu().numpy()
    sp = dict(plain.last_stats)
    plain.close()
    m = nkhip.SwiftHohenberg(N=64, ny=ny, d=float(z["d"]), k=k, r=r, g=g, inner_M="spectral")
    Um = m.step(U).cpu().numpy()
    st = dict(m.last_stats)
    m.close()
    rec = pr.SCIPY_WITH_M[(ny, 64)]
    F = sh_oracle.residual(Um.reshape(-1), U0.reshape(-1), ny, 64, h, r, k, g)
    diff = float(np.abs(Um - Up).max())
    tol = f_tol / pr.lam_min(ny, 64, h, r, k)
    print(f"{ny}x64: |F|inf {np.abs(F).max():.3e}, stats {st}, scipy {rec}, plain njvp "
          f"{sp['njvp']}, |U_M - U_plain|inf {diff:.3e} (tol {tol:.3e})")
    assert st["status"] == 0
    assert np.abs(F).max() <= f_tol
    assert st["n_precond"] > 0
    assert st["nit"] == rec["nit"], (st, rec)
    calls = st["nfev"] + st["njvp"]
    assert abs(calls - rec["nfev"]) <= math.ceil(0.05 * rec["nfev"]), (calls, rec)
    assert diff <= tol, (diff, tol)
    assert st["njvp"] < sp["njvp"], (st, sp)


class _Hooked:
    """An inner_M with SciPy's optional hooks (KrylovJacobian calls setup once, update per step)."""

    def __init__(self, h, r, k):
        self.h, self.r, self.k = h, r, k
        self.setups, self.updates = [], []

    def setup(self, x, f, func):
        self.setups.append((x.shape, f.shape, callable(func)))

    def update(self, x, f):
        self.updates.append((x.shape, float(f.abs().max())))

    def matvec(self, v):
        import nkhip
        return nkhip.ops.sh_precond(v.contiguous(), self.h, self.r, self.k)


def test_generic_newton_krylov_with_inner_M(monkeypatch):
    """newton_krylov(F, x0, inner_M=callable) over the torch residual of the generic tests, at
    their f_tol = 1e-10: the same host loop as the stepper's with NKHIP_FUSED=0, so the same
    iterate to 1e-12.  (The two difference quotients round differently at the 1e-8 relative level
    of an FD JVP, so the iterates agree only as far as both resolve the root: at SciPy's default
    f_tol = 6e-6 they stop 4.6e-12 apart, measured, with |F|inf 8.5e-9 each.)"""
    import nkhip
    monkeypatch.setenv("NKHIP_FUSED", "0")
    z, U0, (h, r, k, g) = _start(64)
    uo = _gpu(U0)

    def residual(u):
        return nkhip.sh_residual(u.contiguous(), uo, h, r, k, g, 64, 64)

    m = nkhip.SwiftHohenberg(N=64, d=float(z["d"]), k=k, r=r, g=g, f_tol=1e-10,
                             inner_M="spectral")
    ref = m.step(uo).clone()
    st = dict(m.last_stats)
    m.close()
    U, info = nkhip.newton_krylov(residual, uo, full_output=True, f_tol=1e-10,
                                  inner_M=lambda v: nkhip.ops.sh_precond(v.contiguous(), h, r, k))
    d = float((U - ref).abs().max())
    print(f"generic vs stepper: {d:.3e}; generic {info}; stepper {st}")
    assert info["status"] == 0 and info["nit"] == st["nit"]
    assert d <= 1e-12, d
    hooked = _Hooked(h, r, k)
    U2, info2 = nkhip.newton_krylov(residual, uo, full_output=True, f_tol=1e-10, inner_M=hooked)
    assert torch.equal(U2, U)
    assert len(hooked.setups) == 1 and hooked.setups[0] == (uo.shape, uo.shape, True)
    assert len(hooked.updates) == info2["nit"], (hooked.updates, info2)
    assert hooked.updates[-1][1] == pytest.approx(info2["fnorm_inf"])
