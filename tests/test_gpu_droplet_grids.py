"""GPU: the droplet and MEMS kernels (csrc/droplet.hip) on grids other than the reference's
91 x 61, point by point against the oracle in extended precision.

Grids (oracle/droplet_grids.py GRIDS, profiles/droplet_grids.md): the 7-wide ones the C-ABI
accepts (an interior of one point, FastDiv(1)), a short last strip of 1, 2 and 4 rows, a second
trip of the strip loop, a second round of DCT tile tasks, DCT tiles exactly full and with one row,
even sides, and a grid that takes the global-memory kernels by its size.  Input: the oracle's
deformed_state (J in [0.59, 1.46], max|dksideta| ~ 0.13: the cross terms count).

Bars (oracle/droplet_grids.py): the kernel against the longdouble oracle, relative to max|ref|,
at min(cap, max(16 e64, 64 eps)), e64 the fp64 oracle's own distance from the longdouble one on
the same input and cap the bar tests/test_gpu_droplet.py applies at 91 x 61.  The PMA loop is
bounded in its increment Q5 - Q0 relative to max|dQ_ref| -- on the 7-wide grids, where
ulp(Q)/|dQ| alone exceeds the 1e-10 cap, as |Q5 - (Q0 + dQ_ref)| <= 1e-10 max|dQ_ref| +
2 ulp(max|Q|).  Every test prints its error-to-bar ratio before asserting.
"""
import numpy as np
import pytest
import torch

from oracle import droplet_grids as G

pytestmark = pytest.mark.gpu

IDS = {g: f"{g[0]}x{g[1]}" for g in G.GRIDS}
# which kernels each grid runs on: asserted, not assumed (nk_drop_lds_fits)
LDS = {g: g != (112, 60) for g in G.GRIDS}


def _grids(gs=G.GRIDS):
    return pytest.mark.parametrize("grid", gs, ids=[IDS.get(g, f"{g[0]}x{g[1]}") for g in gs])


def _np(t):
    return t.detach().cpu().numpy()


def _check(grid, name, err, bar):
    print(f"RATIO {IDS[grid]:>7} {name:<10} err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    assert err <= bar, (name, err, bar)


@pytest.fixture
def drop(grid):
    import nkhip
    from nkhip.droplet import lds_fits
    assert lds_fits(*grid) == LDS[grid]
    ref = G.reference(*grid)
    d = nkhip.Droplet(nx=grid[0], ny=grid[1])
    try:
        d.set_state(ref.U.copy(), ref.Q.copy())  # (the shared arrays are read-only)
        d.prepare()
        yield d, ref
    finally:
        d.close()


@_grids()
def test_mesh_fields(drop, grid):
    d, ref = drop
    for name in G.MESH:
        _check(grid, name, G.rel(_np(d.field(name)), ref.ld[name]), ref.bar[name])


@_grids()
def test_old_time_fields(drop, grid):
    d, ref = drop
    for name in G.OLD:
        _check(grid, name, G.rel(_np(d.field(name)), ref.ld[name]), ref.bar[name])


@_grids()
def test_old_time_fields_of_the_perturbed_state(grid):
    """U_xx, U_yy and F with u1 as the old-time state.  deformed_state's U is the flat film
    wherever the droplets do not reach -- the boundary ring, and the top strips of the larger
    grids -- and there its three fields are 0 whatever the closures' weights; u1 carries noise
    to every point (tests/test_oracle_droplet_grids.py shows the difference on a stale strip)."""
    import nkhip
    ref = G.reference(*grid)
    d = nkhip.Droplet(nx=grid[0], ny=grid[1])
    try:
        d.set_state(ref.u1.copy(), ref.Q.copy())
        d.prepare()
        for name in G.OLD:
            _check(grid, name + "1", G.rel(_np(d.field(name)), ref.ld[name + "1"]),
                   ref.bar[name + "1"])
    finally:
        d.close()


@_grids()
def test_residual_at_every_point(drop, grid):
    d, ref = drop
    out = torch.full((d.n,), float("nan"), dtype=torch.float64, device="cuda")
    R = d.residual(ref.u1.copy(), G.DT, out=out)
    assert R is out
    R = _np(R)
    assert np.isfinite(R).all(), np.flatnonzero(~np.isfinite(R))[:8]  # a point never written
    _check(grid, "R", G.rel(R, ref.ld["R"]), ref.bar["R"])


def _pma(d, ref, grid, name):
    d.pma(G.DTMESH, G.LOOPS)
    q5 = _np(d.field("Q_val"))
    assert G.rel(q5, ref.ld["Q5"]) <= 1e-10  # (what the 91 x 61 tests have always asserted)
    _check(grid, name, *G.pma_error(ref, q5))


@_grids()
def test_pma_increment(drop, grid):
    """5 loops of the persistent PMA kernel: the increment of Q against the reference's, relative
    to max|dQ_ref|; on the 7-wide grids the ulp form (module docstring)."""
    d, ref = drop
    _pma(d, ref, grid, "dQ5")


@_grids([(48, 23), (97, 65)])
def test_pma_increment_forced_global(drop, grid, monkeypatch):
    """The global-memory PMA kernel's plain dense DCT at sizes other than the default one."""
    monkeypatch.setenv("NKHIP_DROP_GLOBAL", "1")
    d, ref = drop
    _pma(d, ref, grid, "dQ5/global")


@_grids([(12, 7), (48, 23), (112, 60)])
def test_initialise_coalescing(grid):
    """drop_u2_kernel on block counts other than the default grid's 22, and the PMA loop's first
    iteration from the caller's fields, against init_coalescing(vsteps=2, loops=2)."""
    import nkhip
    c = G.coalescing_reference(*grid)
    d = nkhip.Droplet(nx=grid[0], ny=grid[1])
    try:
        U, Q = d.initialise_coalescing(**G.COAL)
        U, Q = _np(U), _np(Q)
    finally:
        d.close()
    assert G.rel(Q, c.Q) <= 1e-12
    _check(grid, "coal U", G.rel(U, c.U), c.bar["U"])
    _check(grid, "coal dQ", *G.increment_error(c.Q0, c.dQ, Q, c.bar["dQ"],
                                                G.pma_ulp_form(*grid)))


@_grids([(48, 23), (97, 65)])
def test_fixed_mesh_solve_is_a_root_of_the_reference(drop, grid):
    """solve(1e-4), judged by the reference and not by a second solver: the longdouble residual at
    the returned root is within f_tol = 1e-7 plus what the kernel's own residual may be off by
    (oracle/droplet_grids.py root_residual).  The only cover the finite-difference JVP mode of
    the residual kernel gets off the default grid."""
    d, ref = drop
    root = _np(d.solve(G.DT))
    assert d.last_stats["fnorm_inf"] <= 1e-7
    assert np.abs(root - ref.U).max() > 1e-4  # (the step moved: U itself is no root)
    rmax, bound = G.root_residual(ref, root)
    _check(grid, "solve |R|", rmax, bound)


@pytest.mark.parametrize("n", [7, 32])
def test_mems_steps_smallest_and_full_tile_grids(n):
    """PMA2 steps at n = 7 (interior 1 x 1, FastDiv(1) on both axes) and n = 32 (DCT tiles exactly
    full, even) against the oracle at the same size; tolerances of
    test_gpu_mems.py::test_steps_other_grids_vs_oracle."""
    import nkhip
    from oracle import pma2_oracle as O
    O.configure(n)
    try:
        unew, qval = O.initial_state()
        m = nkhip.Mems(n=n)
        try:
            m.set_state(unew, qval)
            for i in range(2):
                dt = m.step()
                unew, qval, dto = O.step(unew, qval)
                U, Q = m.state()
                errU = float(np.abs(_np(U) - unew).max())
                errQ = float(np.abs(_np(Q) - qval).max() / np.abs(qval).max())
                print(f"RATIO mems n={n} step {i}: |dt - dto| {abs(dt - dto):.1e} U {errU:.3e} "
                      f"(1e-9) Q {errQ:.3e} (1e-12)")
                assert abs(dt - dto) <= 1e-17, i
                assert errU <= 1e-9, i
                assert errQ <= 1e-12, i
        finally:
            m.close()
    finally:
        O.configure(51)
