"""GPU: the spectral preconditioner on grid sides of 8192 and 16384 (csrc/fftpc.hip): columns
transformed in two factors (the four-step form, three trips over the half spectrum), rows of 64 and
128 KB held by one block, and the solves that use them.

NKHIP_FFTPC_SPLIT (read when a plan is built) is the longest column kept on chip; at 16 or 32 the
short grids of the longdouble dense-DFT reference (precond_ref.py, lengths <= 256) go through the
split-column kernels.

Bounds, all set before the kernels ran:
* against longdouble: max(4 x NumPy's double-FFT score on the same input, 1e-13), the rule of
  test_gpu_precond.py;
* where no longdouble reference exists (lengths above 256): 1e-13 against NumPy's realisation, and
  the inverse identity |z/K - L z/2 - v| / |v| (L from ops.sh13_apply) at most 4 x NumPy's own;
* the fused dot: |dot - torch.dot(w, z)| <= 64 eps sum |w_i z_i| (on the grids here a thread adds
  8 products in turn and the rest is trees -- the wave, the block, reduce_final -- so a product
  meets fewer than 32 roundings on its way into either sum).

Measured (MI355X), worst input per grid.  Split columns against longdouble: 64x64 5.8e-15,
256x8 6.4e-15 (6.1e-15 with the knob at 32), 128x64 1.0e-14, 32x16 5.7e-16.  New lengths against
NumPy's realisation (random field; identity kernel / NumPy): 8x8192 9.4e-15 (4.0e-12 / 3.8e-12),
8x16384 9.7e-15 (4.2e-12 / 4.6e-12), 8192x8 1.1e-14 (3.9e-12 / 3.4e-12), 16384x8 8.4e-15
(4.5e-12 / 4.2e-12), 16384x16 7.8e-15 (3.1e-12 / 2.4e-12).  16384^2: the tiled field 3.4e-16 from
the longdouble tile; identity 2.2e-15 beside 2.4e-15 at 4096^2.  Fused dot: 7.1e-15, 3.6e-15 and
2.2e-16 from torch.dot (bounds 6.3e-11, 6.4e-11, 8.5e-13).  8192x64 step: 34 JVPs with M, 109
without, the two results 5.4e-10 apart (tolerance 1.2e-6); SHLinearised: 16-17 PCG iterations
beside 90-92, the steps 1.4e-13 apart.
"""
import math

import numpy as np
import pytest
import torch

import precond_ref as pr
from conftest import load_golden
from oracle import sh_oracle

pytestmark = pytest.mark.gpu

H, R, K = 0.0625, 0.01, 0.2  # the bench constants: cond(A0) ~ 4e5
PARITY = 1e-13
EPS = float(np.finfo(np.float64).eps)
KNOB = "NKHIP_FFTPC_SPLIT"


def _gpu(v):
    return torch.as_tensor(np.ascontiguousarray(v), device="cuda")


def _apply(v, h=H):
    import nkhip
    return nkhip.ops.sh_precond(_gpu(v), h, R, K).cpu().numpy()


def _against_longdouble(ny, nx):
    worst = 0.0
    for name, v in pr.inputs(ny, nx).items():
        ref = pr.precond_ld(v, H, R, K)
        e_np = pr.rel_err(pr.precond_np(v, H, R, K), ref)
        e = pr.rel_err(_apply(v), ref)
        print(f"{ny}x{nx} {name}: kernel {e:.2e}, numpy {e_np:.2e}")
        worst = max(worst, e)
        assert e <= max(4 * e_np, PARITY), (name, e, e_np)
    print(f"{ny}x{nx}: worst {worst:.2e}")


# --------------------------------------------------------- 1. split columns against longdouble
@pytest.mark.parametrize("split,ny,nx", [(16, 64, 64), (16, 256, 8), (16, 128, 64), (16, 32, 16),
                                         (32, 256, 8)])
def test_split_columns_against_longdouble(monkeypatch, split, ny, nx):
    """ny = 16 x 4, 16 x 16, 16 x 8, 16 x 2 (the smallest split) and 32 x 8."""
    monkeypatch.setenv(KNOB, str(split))
    _against_longdouble(ny, nx)


# ------------------------------------------------------------------------- 2. the new lengths
@pytest.mark.parametrize("ny,nx", [(8, 8192), (8, 16384), (8192, 8), (16384, 8), (16384, 16)])
def test_new_lengths(ny, nx):
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


# ------------------------------------------------------------- 3. knob off is the old path
@pytest.mark.parametrize("ny,nx", [(64, 256), (4096, 8)])
def test_knob_off_is_the_old_path(monkeypatch, ny, nx):
    import nkhip
    v = pr.inputs(ny, nx)["random"]
    vg = _gpu(v)
    monkeypatch.delenv(KNOB, raising=False)
    a = nkhip.ops.sh_precond(vg, H, R, K)
    monkeypatch.setenv(KNOB, "4096")
    assert torch.equal(a, nkhip.ops.sh_precond(vg, H, R, K))
    monkeypatch.setenv(KNOB, "24")  # not a power of two: ignored
    assert torch.equal(a, nkhip.ops.sh_precond(vg, H, R, K))
    monkeypatch.setenv(KNOB, "16")
    b = nkhip.ops.sh_precond(vg, H, R, K)
    assert not torch.equal(a, b)  # the knob is read: other kernels, other roundings
    if ny <= 256:
        ref = pr.precond_ld(v, H, R, K)
        e_np = pr.rel_err(pr.precond_np(v, H, R, K), ref)
        e = pr.rel_err(b.cpu().numpy(), ref)
        print(f"{ny}x{nx}: split {e:.2e}, numpy {e_np:.2e}")
        assert e <= max(4 * e_np, PARITY), (e, e_np)
    else:  # no longdouble reference at this length: the rule of test_new_lengths
        e = pr.rel_err(b.cpu().numpy(), pr.precond_np(v, H, R, K))
        print(f"{ny}x{nx}: split vs numpy {e:.2e}")
        assert e <= PARITY, e


# ------------------------------------------------------------- 4. deterministic and in place
@pytest.mark.parametrize("ny,nx", [(16384, 8), (8, 16384)])
def test_deterministic_and_in_place(ny, nx):
    import nkhip
    v = _gpu(pr.inputs(ny, nx)["random"])
    a = nkhip.ops.sh_precond(v, H, R, K)
    b = nkhip.ops.sh_precond(v, H, R, K)
    assert torch.equal(a, b)
    w = v.clone()
    nkhip.ops.sh_precond(w, H, R, K, out=w)
    assert torch.equal(a, w)


# ------------------------------------------------------------------------------ 5. fused dot
@pytest.mark.parametrize("split,ny,nx", [(None, 16384, 8), (None, 8, 16384), (16, 256, 8)])
def test_fused_dot(monkeypatch, split, ny, nx):
    import nkhip
    if split is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(split))
    v = _gpu(pr.inputs(ny, nx)["random"])
    w = _gpu(np.random.default_rng(5 + ny + 7 * nx).standard_normal((ny, nx)))
    plain = nkhip.ops.shlin_precond(v, H, R, K, sigma=0.3)
    z, dot = nkhip.ops.shlin_precond(v, H, R, K, sigma=0.3, dot_with=w)
    assert torch.equal(z, plain)
    z2, dot2 = nkhip.ops.shlin_precond(v, H, R, K, sigma=0.3, dot_with=w)
    assert torch.equal(z2, z) and dot2 == dot
    ref = float(torch.dot(w.reshape(-1), z.reshape(-1)))
    bound = 64 * EPS * float((w * z).abs().sum())
    print(f"{ny}x{nx}: dot {dot!r}, torch {ref!r}, err {abs(dot - ref):.2e}, bound {bound:.2e}")
    assert abs(dot - ref) <= bound


# ------------------------------------------------------------------- 6. the whole grid, once
def test_whole_16384_grid():
    """16384 x 16384 at h = 0.625, everything on the GPU (v, z, L z and the plan's half spectrum:
    4 x 2 GiB).  (a) The operator commutes with periodic tiling at equal h, so a tiled 64 x 64
    field must come back as the tiling of the longdouble result of the 64 x 64 field: an address
    that wraps at 2^31 cannot pass.  (b) The inverse identity on a random field, against the same
    score of a 4096 x 4096 application (the three-pass kernels)."""
    import nkhip
    h, n, t = 0.625, 16384, 64
    tile = np.random.default_rng(16384).standard_normal((t, t))
    ref = _gpu(pr.precond_ld(tile, h, R, K))
    v = _gpu(tile).repeat(n // t, n // t)
    z = nkhip.ops.sh_precond(v, h, R, K)
    zt = z.view(n // t, t, n // t, t)
    zt.sub_(ref[None, :, None, :])
    e = float(z.abs().max() / ref.abs().max())
    print(f"16384^2 tiled: {e:.2e} from the longdouble tile")
    assert e <= PARITY, e

    def ident(v, z, lz):
        nkhip.ops.sh13_apply(z, h, R, out=lz)
        lz.mul_(-0.5).add_(z, alpha=1.0 / K).sub_(v)
        return float(lz.abs().max() / v.abs().max())

    gen = torch.Generator(device="cuda").manual_seed(6)
    vs = torch.randn(4096, 4096, dtype=torch.float64, device="cuda", generator=gen)
    i_small = ident(vs, nkhip.ops.sh_precond(vs, h, R, K), torch.empty_like(vs))
    v.normal_(generator=gen)
    nkhip.ops.sh_precond(v, h, R, K, out=z)
    lz = torch.empty_like(v)
    i_big = ident(v, z, lz)
    print(f"identity: 16384^2 {i_big:.2e}, 4096^2 {i_small:.2e}")
    assert i_big <= 4 * i_small, (i_big, i_small)


# ----------------------------------------------------------------------------------- 7. solves
def _start(ny):
    z = load_golden("nk_n64_default")
    U0 = pr.start_state(z["traj"][0], ny, 64)
    return z, U0, tuple(float(z[q]) for q in "hrkg")


def _step_pair(ny):
    """One Crank-Nicolson step from the fixture state tiled to ny x 64, plain and with M."""
    import nkhip
    z, U0, (h, r, k, g) = _start(ny)
    U = _gpu(U0)
    plain = nkhip.SwiftHohenberg(N=64, ny=ny, d=float(z["d"]), k=k, r=r, g=g)
    Up = plain.step(U).cpu().numpy()
    sp = dict(plain.last_stats)
    plain.close()
    m = nkhip.SwiftHohenberg(N=64, ny=ny, d=float(z["d"]), k=k, r=r, g=g, inner_M="spectral")
    Um = m.step(U).cpu().numpy()
    st = dict(m.last_stats)
    m.close()
    f_tol = EPS ** (1.0 / 3.0)
    F = sh_oracle.residual(Um.reshape(-1), U0.reshape(-1), ny, 64, h, r, k, g)
    diff = float(np.abs(Um - Up).max())
    tol = f_tol / pr.lam_min(ny, 64, h, r, k)
    print(f"{ny}x64: |F|inf {np.abs(F).max():.3e}, stats {st}, plain njvp {sp['njvp']}, "
          f"|U_M - U_plain|inf {diff:.3e} (tol {tol:.3e})")
    assert st["status"] == 0
    assert np.abs(F).max() <= f_tol
    assert st["n_precond"] > 0
    assert diff <= tol, (diff, tol)
    return st, sp


def test_preconditioned_step_split_columns(monkeypatch):
    """test_gpu_precond.py::test_preconditioned_step at 128 x 64 with the columns split 16 x 8:
    the same checks against SciPy's record."""
    monkeypatch.setenv(KNOB, "16")
    st, sp = _step_pair(128)
    rec = pr.SCIPY_WITH_M[(128, 64)]
    assert st["nit"] == rec["nit"], (st, rec)
    calls = st["nfev"] + st["njvp"]
    assert abs(calls - rec["nfev"]) <= math.ceil(0.05 * rec["nfev"]), (calls, rec)
    assert st["njvp"] < sp["njvp"], (st, sp)


def test_preconditioned_step_8192_rows():
    _step_pair(8192)


def test_shlin_8192_rows():
    """SHLinearised(precond="spectral") on 8192 x 64 (the golden start tiled in y), two steps
    beside the unpreconditioned stepper.  Both solve to a relative residual of 1e-14; the
    tolerance is the 1e-11 test_gpu_shlin_precond.py allows either of them from the direct solve."""
    import nkhip
    z = load_golden("shlin_steps")
    N, ny = int(z["N"]), 8192
    assert N == 64
    kw = dict(N=N, ny=ny, d=float(z["d"]), k=float(z["k"]), r=float(z["r"]), g=float(z["g"]))
    U0 = _gpu(np.tile(np.asarray(z["U0"], dtype=np.float64).reshape(N, N), (ny // N, 1)))
    s = nkhip.SHLinearised(precond="spectral", **kw)
    plain = nkhip.SHLinearised(**kw)
    try:
        U = Uo = Up = Uop = U0.reshape(-1)
        for i in range(2):
            U, Uo = s.step(U, Uo), U
            Up, Uop = plain.step(Up, Uop), Up
            err = float((U - Up).abs().max() / Up.abs().max())
            print(f"step {i}: PCG {s.last_iters}, CG {plain.last_iters}, M applications "
                  f"{s.last_precond}, shift {s.last_shift:.6g}, PCG vs CG {err:.2e}")
            assert s.last_precond > 0
            assert s.last_relres <= 1e-14
            assert err <= 1e-11, (i, err)
    finally:
        s.close()
        plain.close()


# -------------------------------------------------------------------------------- 8. refusals
def test_refusal_above_16384():
    import nkhip
    with pytest.raises(nkhip.NKError):
        nkhip.ops.sh_precond(torch.zeros(8, 32768, dtype=torch.float64, device="cuda"), H, R, K)
    with pytest.raises(nkhip.NKError):
        nkhip.ops.shlin_precond(torch.zeros(32768, 8, dtype=torch.float64, device="cuda"), H, R, K)
    m = nkhip.SwiftHohenberg(N=64, d=40.0, inner_M="spectral")
    try:
        z = load_golden("nk_n64_default")
        m.step(_gpu(np.asarray(z["traj"][0]).reshape(64, 64)))
        assert m.last_stats["status"] == 0 and m.last_stats["n_precond"] > 0
    finally:
        m.close()
