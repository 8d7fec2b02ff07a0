"""TEST INFRASTRUCTURE ONLY -- the droplet kernels' reference values, and the bars they are held
to, on grids other than the reference's 91 x 61.

Input: ``droplet_oracle.deformed_state`` (a mesh far from the identity, so the cross terms count).
Reference: ``droplet_oracle`` evaluated in np.longdouble on that fp64 input.  Yardstick: the same
oracle in fp64.  The mesh and Laplace fields amplify the rounding of Q by 1/h^2 to 1/h^4, and no
fixed operation count bounds that the way it bounds a stencil pass, so the fp64 oracle's own
distance from the longdouble one,

    e64 = max|fp64 - longdouble| / max|longdouble|        (per grid and quantity),

is the scale: another summation order of the same ill-conditioned sum lands within a small
multiple of it.  A kernel is compared with the longdouble values at

    bar = min(CAP, max(FACTOR * e64, FLOOR)),   FACTOR = 16,   FLOOR = 64 eps64,

CAP being what tests/test_gpu_droplet.py applies at 91 x 61.  The floor keeps a lucky near-exact
fp64 reference on a tiny grid from turning into an unmeetable bar; the cap is never raised.

The PMA loop is judged by its increment dQ5 = Q5 - Q0 (5 loops move Q ~ 18 by ~1e-4; a bound on
Q5 relative to max|Q| would pass a 1e-5 relative error of the mesh velocity).  Where the
subtraction itself costs more than the cap -- ulp(Q) / |dQ| on the 7-wide grids -- the bound is on
Q5 directly: |Q5 - (Q0 + dQ_ref)| <= CAP max|dQ_ref| + 2 ulp(max|Q|)  (``pma_error``).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from . import droplet_oracle as O

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)

# (nx, ny): what each is the smallest case of is tabulated in profiles/droplet_grids.md
GRIDS = [(7, 7), (12, 7), (7, 13), (32, 32), (48, 23), (97, 65), (112, 60), (91, 61)]
DEFAULT = (91, 61)

MESH = ["d2ksi", "d2eta", "dksideta", "J", "A11", "A22", "A12", "Q_dksi", "Q_deta"]
OLD = ["U_xx", "U_yy", "F"]
# the same three with the perturbed u1 as the old-time state: deformed_state's U is the flat film
# wherever the droplets do not reach, the boundary ring and the top strips of the larger grids
# included, and U_xx, U_yy and F vanish there; u1 carries noise to every point
OLD1 = ["U_xx1", "U_yy1", "F1"]
CAP = {**{k: 1e-10 for k in MESH + OLD + OLD1}, "Q_dksi": 1e-13, "Q_deta": 1e-13, "F": 1e-9,
       "F1": 1e-9, "R": 1e-11, "dQ5": 1e-10}
FACTOR = 16
FLOOR = 64 * EPS64

DT = 1e-4        # the residual's and the solve's time step
DTMESH = 3e-9    # pma(DTMESH, LOOPS)
LOOPS = 5


def short_strip(nx, ny):
    """Rows of the last (short) strip of the kernels' 5-row strip walk over the interior, 0 if the
    strips are all full."""
    return (ny - 6) % 5


def evaluate(u, q, u1, dtype):
    """Every compared quantity from the oracle as configured now, inputs cast to `dtype`."""
    u, q, u1 = (np.asarray(a, dtype=dtype) for a in (u, q, u1))
    Q = O.q_ders(q)
    A11, A22, A12 = O.metric(Q)
    F, U = O.step_rhs(u, Q)
    R = O.residual(u1, F, DT, u, Q)
    F1, U1 = O.step_rhs(u1, Q)
    q5 = O.loop_pma(q, u, DTMESH, LOOPS, Q=Q, U=U)
    return {"d2ksi": Q.d2ksi, "d2eta": Q.d2eta, "dksideta": Q.dksideta, "J": Q.J, "A11": A11,
            "A22": A22, "A12": A12, "Q_dksi": Q.dksi, "Q_deta": Q.deta, "U_xx": U.xx,
            "U_yy": U.yy, "F": F, "U_xx1": U1.xx, "U_yy1": U1.yy, "F1": F1, "R": R,
            "dQ5": q5 - q, "Q5": q5}


def rel(a, ref):
    """max|a - ref| / max|ref|, the difference taken in ref's precision."""
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(a, dtype=ref.dtype) - ref).max() / np.abs(ref).max())


def pma_ulp_form(nx, ny):
    """The grids whose dQ5 takes the bound on Q5 itself (module docstring)."""
    return min(nx, ny) == 7


@functools.lru_cache(maxsize=None)
def reference(nx, ny):
    """The input state, both oracle evaluations, e64 and the bars of one grid (computed once and
    shared; treat the arrays as read-only).  Leaves the oracle configured for 91 x 61 in fp64."""
    try:
        u, q, u1 = O.deformed_state(nx, ny)
        f64 = evaluate(u, q, u1, np.float64)
        O.configure(nx, ny, LD)
        ld = evaluate(u, q, u1, LD)
    finally:
        O.configure(*DEFAULT)
    e64 = {k: rel(f64[k], ld[k]) for k in CAP}
    bar = {k: min(CAP[k], max(FACTOR * e64[k], FLOOR)) for k in CAP}
    for a in (u, q, u1, *f64.values(), *ld.values()):
        a.setflags(write=False)
    return SimpleNamespace(nx=nx, ny=ny, U=u, Q=q, u1=u1, f64=f64, ld=ld, e64=e64, bar=bar)


def pma_error(ref, q5):
    """(error, bound) of a kernel's Q after pma(DTMESH, LOOPS) from ref.Q, both as multiples of
    max|dQ_ref|: the increment's distance from the reference increment against its bar, or on
    the 7-wide grids Q5's distance from Q0 + dQ_ref against CAP plus 2 ulp(max|Q|)."""
    return increment_error(ref.Q, ref.ld["dQ5"], q5, ref.bar["dQ5"],
                           pma_ulp_form(ref.nx, ref.ny))


def increment_error(q0, dq_ref, q_end, bar, ulp_form):
    """(error, bound) of a kernel's final Q against q0 + dq_ref, as multiples of max|dq_ref|: the
    two forms of the module docstring."""
    scale = float(np.abs(dq_ref).max())
    q_end = np.asarray(q_end, dtype=np.float64)
    if ulp_form:
        err = float(np.abs(q_end.astype(LD) - (q0.astype(LD) + dq_ref)).max())
        bound = CAP["dQ5"] * scale + 2 * float(np.spacing(np.abs(q0).max()))
        return err / scale, bound / scale
    return rel(q_end - q0, dq_ref), bar


COAL = dict(vsteps=2, loops=2)  # initialise_coalescing: the second step's two loops move Q


@functools.lru_cache(maxsize=None)
def coalescing_reference(nx, ny):
    """init_coalescing(vsteps=2, loops=2) from the flat film, in both precisions.  U: cap 1e-10
    (tests/test_gpu_droplet.py's bar on the full run); Q: its increment, as the PMA loop's."""
    try:
        O.configure(nx, ny)
        _, q0 = O.initial_mesh()
        u64, q64 = O.init_coalescing(**COAL)
        O.configure(nx, ny, LD)
        uld, qld = O.init_coalescing(**COAL)
    finally:
        O.configure(*DEFAULT)
    dq = qld - q0
    e64 = {"U": rel(u64, uld), "dQ": rel(q64 - q0, dq)}
    bar = {k: min(1e-10, max(FACTOR * v, FLOOR)) for k, v in e64.items()}
    return SimpleNamespace(nx=nx, ny=ny, Q0=q0, U64=u64, Q64=q64, U=uld, Q=qld, dQ=dq, e64=e64,
                           bar=bar)


def root_residual(ref, root, dt=DT):
    """(max|R|, bound) of the longdouble residual at a fixed-mesh Newton-Krylov root from
    (ref.U, ref.Q): bound = f_tol + bar[R] * max|terms|, f_tol = 1e-7 what the solver stopped its
    own fp64 residual at, the second term what that residual may be off by -- the residual's
    bar at this grid, relative to the largest of the terms it subtracts (u - U.val, dt F2 / 2,
    dt F / 2)."""
    try:
        O.configure(ref.nx, ref.ny, LD)
        u, q, w = (np.asarray(a, dtype=LD) for a in (ref.U, ref.Q, root))
        Q = O.q_ders(q)
        F, _ = O.step_rhs(u, Q)
        R = O.residual(w, F, dt, u, Q)
        F2 = -(R - (w - u)) * 2 / dt - F
    finally:
        O.configure(*DEFAULT)
    terms = max(float(np.abs(w - u).max()), float(np.abs(dt * F2 / 2).max()),
                float(np.abs(dt * F / 2).max()))
    return float(np.abs(R).max()), 1e-7 + ref.bar["R"] * terms
