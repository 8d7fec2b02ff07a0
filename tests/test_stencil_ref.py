"""CPU: the extended-precision stencil reference (oracle/stencil_ref.py) and its per-point bound.

Three things are pinned here, without a GPU:

* the reference computes the operators the project already pins -- ``sh_oracle.sh13`` /
  ``residual`` / ``jvp`` and the reference's own golden vectors -- to the tolerances those tests use;
* a plain fp64 evaluation of every mode in the kernel's layout (``emulate64``) stays inside
  ``64 eps mag`` at every point.  Largest ratio |out - ref| / bound seen over the shapes below
  (seeded inputs, periodic and slab layouts): LAP5 0.019, SH13 0.024, RESID 0.022, BOLD 0.029,
  TRIAL 0.030, FDJVP 0.035, AJVP 0.030, LINOP 0.021 -- the bound has room, as a worst-case
  bound over a mean-zero rounding walk should;
* deliberate mutants of that evaluation leave the bound by at least 1000x, so the bound is
  tight enough to see a wrong column, a missing alpha, swapped coefficients or a wrong 1/k.
  ("1/k for ik" is read as a wrong VALUE of that factor -- k itself: dividing by k where the
  kernels multiply by the rounded 1/k is a legitimate rounding of the same expression and must
  stay inside the bound, which test_division_by_k_is_a_legitimate_order pins.)
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import sh_oracle
from oracle import stencil_ref as sr

H, R, K, G = 0.625, 0.01, 0.2, 1.0
SHAPES = [(2, 2), (3, 4), (5, 7), (1, 6), (7, 254), (13, 256), (8, 258), (9, 600)]
ALPHA, THETA, SC = 0.37, 0.1, 1e-4


def _inputs(ny, nx, seed=0):
    rng = np.random.default_rng(1000 * ny + nx + seed)
    return tuple(rng.standard_normal((ny, nx)) for _ in range(3))


def _case(mode, ny, nx, mutant=None, halo=False):
    """[(out, ref, mag), ...] of one fp64 evaluation against the reference; halo: as the middle
    slab of a grid three times as tall, its halo rows cut from the global arrays."""
    gy = 3 * ny if halo else ny
    a, b, p0 = _inputs(gy, nx)
    row0 = ny if halo else 0
    cut = (lambda x: sr.rows(x, row0, ny)) if halo else (lambda x: x)
    kw = dict(h=H, r=R, k=K, g=G, mutant=mutant)
    if halo:
        kw.update(a_halo=sr.halo_of(a, row0, ny), b_halo=sr.halo_of(b, row0, ny))
    la, lb, lp = a[row0:row0 + ny], b[row0:row0 + ny], p0[row0:row0 + ny]
    if mode == sr.LAP5:
        out = sr.emulate64(mode, la, e=1 / H ** 2, **kw)
        ref, mag = sr.lap5(a, 1 / H ** 2)
    elif mode == sr.SH13:
        out = sr.emulate64(mode, la, **kw)
        ref, mag = sr.sh13(a, H, R)
    elif mode == sr.RESID:
        out = sr.emulate64(mode, la, lb, **kw)
        ref, mag = sr.resid(a, b, H, R, K, G)
    elif mode == sr.BOLD:
        out = sr.emulate64(mode, la, **kw)
        ref, mag = sr.bold(a, H, R, K, G)
    elif mode == sr.TRIAL:
        out = sr.emulate64(mode, la, lb, lp, alpha=ALPHA, **kw)
        ref, mag = sr.trial(a, b, ALPHA, p0, H, R, K, G)
    elif mode == sr.FDJVP:
        zs = 1.0 / np.linalg.norm(b)
        out = sr.emulate64(mode, la, lb, lp, alpha=SC * zs, sc=SC, **kw)
        ref, mag = sr.fdjvp(a, b, SC * zs, p0, SC, H, R, K, G)
    elif mode == sr.AJVP:
        out = sr.emulate64(mode, la, None, lp, alpha=ALPHA, **kw)
        ref, mag = sr.ajvp(a, p0, ALPHA, H, R, K, G)
    else:
        out = sr.emulate64(mode, la, lb, lp, alpha=ALPHA, theta=THETA, **kw)
        ref, mag = sr.linop(a, b, ALPHA, p0, THETA, H, R)
    if not isinstance(out, tuple):
        out, ref, mag = (out,), (ref,), (mag,)
    return [(o, cut(f), cut(m)) for o, f, m in zip(out, ref, mag)]


def _worst(mode, ny, nx, **kw):
    return max(sr.ratio(o, f, m) for o, f, m in _case(mode, ny, nx, **kw))


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize("name", ["ops_n5_d2", "ops_n61", "ops_n64", "ops_n128_h0625"])
def test_reference_operators_match_golden(name):
    z = load_golden(name)
    N, h, r = int(z["N"]), float(z["h"]), float(z["r"])
    v = z["v"].reshape(N, N)
    lap, _ = sr.lap5(v, 1.0 / h ** 2)
    L, _ = sr.sh13(v, h, r)
    assert np.abs(lap.reshape(-1) - z["lap_v"]).max() <= 1e-13 * np.abs(z["lap_v"]).max()
    assert np.abs(L.reshape(-1) - z["L_v"]).max() <= 1e-13 * np.abs(z["L_v"]).max()


def test_reference_residual_matches_golden():
    z = load_golden("residual_n61")
    F, _ = sr.resid(z["u"].reshape(61, 61), z["uo"].reshape(61, 61), float(z["h"]), float(z["r"]),
                    float(z["k"]), float(z["g"]))
    assert np.abs(F.reshape(-1) - z["F"]).max() <= 1e-12 * np.abs(z["F"]).max()


@pytest.mark.parametrize("ny,nx", [(5, 7), (13, 256), (61, 61)])
def test_reference_matches_sh_oracle(ny, nx):
    u, uo, v = _inputs(ny, nx)
    f = (lambda x: np.asarray(x, dtype=np.float64).reshape(-1))

    def rel(x, y):
        return np.abs(f(x) - y).max() / np.abs(y).max()

    assert rel(sr.sh13(v, H, R)[0], sh_oracle.sh13(v.reshape(-1), ny, nx, H, R)) <= 1e-13
    assert rel(sr.lap5(v, 2.56)[0], sh_oracle.lap5(v.reshape(-1), ny, nx, 2.56)) <= 1e-13
    assert rel(sr.resid(u, uo, H, R, K, G)[0],
               sh_oracle.residual(u.reshape(-1), uo.reshape(-1), ny, nx, H, R, K, G)) <= 1e-12
    assert rel(sr.ajvp(v, u, 1.0, H, R, K, G)[0],
               sh_oracle.jvp(u.reshape(-1), v.reshape(-1), ny, nx, H, R, K, G)) <= 1e-12
    # the pieces the solver composes: F(u) = G(u) + B(uo) (TRIAL at alpha = 0 over BOLD)
    B, _ = sr.bold(uo, H, R, K, G)
    (F, Gw, w), _ = sr.trial(u, u, 0.0, B, H, R, K, G)
    assert rel(F, sh_oracle.residual(u.reshape(-1), uo.reshape(-1), ny, nx, H, R, K, G)) <= 1e-12
    assert np.array_equal(f(w), u.reshape(-1))
    # the FD quotient against the oracle's (two G evaluations in fp64): its own noise is
    # ~eps |G| / sc = 1e-9 of the result at this step
    sc = 1e-4
    q, _ = sr.fdjvp(u, v, sc, Gw, sc, H, R, K, G)
    assert rel(q, sh_oracle.fd_quotient(u.reshape(-1), v.reshape(-1), sc, sc, ny, nx, H, R, K,
                                        G)) <= 1e-7


def test_magnitude_dominates_value():
    for mode in range(8):
        for out, ref, mag in _case(mode, 5, 7):
            assert (np.abs(ref) <= mag * (1 + 1e-15)).all(), sr.MODE_NAMES[mode]


def test_scales():
    a, s = sr.dev_scale(sr.FDJVP, 4.0, 1e-6)
    assert float(a) == 5e-7 and float(s) == 1e-6
    a, _ = sr.dev_scale(sr.AJVP, 16.0, 0.0)
    assert float(a) == 0.25
    go, a, s = sr.spec_scale((1.0, 4.0, 8.0), 2.0, 1e-9, 1e-3, 2.0, 0.5)
    assert go and abs(float(s) - 1e-3) < 1e-18 and abs(float(a) - 5e-4) < 1e-18
    assert not sr.spec_scale((float("nan"), 4.0, 8.0), 2.0, 1e-9, 1e-3, 2.0, 0.5)[0]
    assert not sr.spec_scale((3.0, 4.0, 8.0), 2.0, 1e-9, 1e-3, 2.0, 0.5)[0]
    assert not sr.spec_scale((1.0, 1e-10, 8.0), 2.0, 1e-9, 1e-3, 2.0, 0.5)[0]


@pytest.mark.parametrize("halo", [False, True], ids=["periodic", "slab"])
@pytest.mark.parametrize("mode", range(8), ids=sr.MODE_NAMES)
def test_fp64_evaluation_is_within_the_bound(mode, halo):
    worst = 0.0
    for ny, nx in SHAPES:
        if halo and ny < 2:
            continue
        worst = max(worst, _worst(mode, ny, nx, halo=halo))
    print(f"{sr.MODE_NAMES[mode]} {'slab' if halo else 'periodic'}: max ratio {worst:.4f}")
    assert worst <= 1.0


def test_division_by_k_is_a_legitimate_order():
    """w / k for w * (1/k) is another rounding of the same expression: inside the bound (this
    is NOT the "ik" mutant, which has the wrong value there)."""
    a, _, _ = _inputs(9, 600)
    f8 = np.float64
    ref, mag = sr.bold(a, H, R, K, G)
    out = sr.emulate64(sr.BOLD, a, h=H, r=R, k=K, g=G)
    alt = out + a * (f8(1.0) / f8(K)) - a / f8(K)
    assert sr.ratio(alt, ref, mag) <= 1.0


# which modes a mutant changes at all
_HITS = {
    "wrap": range(1, 8),  # LAP5 has radius 1: no column c + 2
    "halo_alpha": (sr.TRIAL, sr.FDJVP, sr.LINOP),
    "swap": (sr.SH13, sr.RESID, sr.BOLD, sr.TRIAL, sr.FDJVP, sr.AJVP, sr.LINOP),
    "ik": (sr.BOLD, sr.TRIAL, sr.FDJVP, sr.AJVP),
}


@pytest.mark.parametrize("mutant", sr.MUTANTS)
@pytest.mark.parametrize("halo", [False, True], ids=["periodic", "slab"])
def test_mutants_leave_the_bound(mutant, halo):
    for mode in _HITS[mutant]:
        for ny, nx in [(5, 7), (13, 256), (9, 600)]:
            got = _worst(mode, ny, nx, mutant=mutant, halo=halo)
            assert got >= 1000.0, (mutant, sr.MODE_NAMES[mode], ny, nx, got)
