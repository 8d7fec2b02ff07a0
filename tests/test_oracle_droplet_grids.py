"""CPU: the droplet oracle at any grid and in extended precision, the deformed input state, the
bars tests/test_gpu_droplet_grids.py holds the kernels to (oracle/droplet_grids.py) -- and proof
that those bars can fail: each mutant below is a mistake a kernel could make, applied to the fp64
oracle, and must leave the bar by at least 100 times on every grid that has the feature.
"""
import importlib.util

import numpy as np
import pytest

from oracle import droplet_grids as G
from oracle import droplet_oracle as O

GRID_IDS = [f"{nx}x{ny}" for nx, ny in G.GRIDS]
grids = pytest.mark.parametrize("grid", G.GRIDS, ids=GRID_IDS)
KILL = 100  # a mutant must miss its bar by this factor


def test_configure_default_reproduces_the_import_state():
    spec = importlib.util.spec_from_file_location("droplet_oracle_fresh", O.__file__)
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    O.configure(12, 7, np.longdouble)
    O.configure(91, 61)
    for name in ("D1X", "D1Y", "D2X", "D2Y"):
        a, b = getattr(O, name), getattr(fresh, name)
        assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b), name
    for name in ("Left", "Right", "Bottom", "Top", "Boundary"):
        assert np.array_equal(getattr(O.IB, name), getattr(fresh.IB, name)), name
    for name in ("Nx", "Ny", "NN", "dksi", "deta", "dksi2", "deta2"):
        a, b = getattr(O.P, name), getattr(fresh.P, name)
        assert type(a) is type(b) and a == b, name
    # ... and what the module held before configure() existed
    assert O.P.dksi == 9.0 / 90 and O.P.deta == 6.0 / 60 and O.P.dksi2 == O.P.dksi * O.P.dksi
    assert np.array_equal(O.D2X[0, :5], np.array([-415 / 6, 96, -36, 32 / 3, -1.5]) / (12 * O.P.dksi2))
    assert np.array_equal(O.D1Y[1, :5], np.array([-3.0, -10, 18, -6, 1]) / (12 * O.P.deta))


def test_extended_precision_is_extended():
    """The longdouble chain does not pass through fp64 anywhere: every output is longdouble and
    differs from the fp64 evaluation by rounding only (never agrees bit for bit)."""
    ref = G.reference(48, 23)
    for k, v in ref.ld.items():
        assert v.dtype == np.longdouble, k
        assert ref.f64[k].dtype == np.float64, k
    for k in ("U_xx", "F", "R", "dQ5", "A12"):
        low = ref.ld[k].astype(np.float64).astype(np.longdouble)
        assert np.any(low != ref.ld[k]), k


@grids
def test_deformed_state_is_far_from_the_identity(grid):
    ref = G.reference(*grid)
    assert (O.P.Nx, O.P.Ny, O.P.dtype) == (91, 61, np.float64)  # reference() restores the default
    J = ref.f64["J"]
    assert all(np.isfinite(v).all() for v in ref.f64.values())
    assert 0.5 < J.min() and J.max() < 1.6
    assert np.abs(ref.f64["dksideta"]).max() > 0.1
    assert 3e-5 <= np.abs(ref.ld["dQ5"]).max() <= 1.25e-4   # 5 PMA loops move Q measurably
    assert ref.U.min() > 0 and ref.U.max() > 0.5            # two droplets on a wet film


@grids
def test_reference_rounding_is_under_every_cap(grid):
    """e64 <= cap for every quantity, so min(cap, 16 e64) is a bar that fp64 arithmetic can
    meet; the one exception is dQ5 on the 7-wide grids (1.2e-10 to 1.4e-10 against 1e-10: the
    subtraction from Q ~ 18 costs ulp(Q)/|dQ|), which take the bound on Q5 itself, and that bound
    the fp64 oracle meets.

    (16 e64 itself is NOT under the cap everywhere, and need not be: the cap then is the bar.
    Measured: R 1.0e-12 to 1.8e-12 at 97 x 65, 112 x 60 and 91 x 61 (16 e64 = 1.7 to 2.9 caps),
    Q_deta 1.0e-14 to 1.4e-14 there (1.6 to 2.2 caps), dQ5 5.5e-11 to 8.7e-11 on every grid with
    sides over 7 (9 to 14 caps).)"""
    ref = G.reference(*grid)
    for k, cap in G.CAP.items():
        if k == "dQ5" and G.pma_ulp_form(*grid):
            assert ref.e64[k] > cap  # (else the plain form would do)
            err, bound = G.pma_error(ref, ref.f64["Q5"])
            assert err <= bound
            continue
        assert ref.e64[k] <= cap, (k, ref.e64[k])
        assert G.FLOOR <= ref.bar[k] <= cap and ref.bar[k] >= min(cap, G.FACTOR * ref.e64[k])


# ------------------------------------------------------------------------------------ mutants
def _mutant(ref, monkeypatch, **patches):
    """The fp64 oracle's quantities on ref's input with attributes of the oracle replaced."""
    for name, fn in patches.items():
        monkeypatch.setattr(O, name, fn)
    try:
        O.configure(ref.nx, ref.ny)
        return G.evaluate(ref.U, ref.Q, ref.u1, np.float64)
    finally:
        monkeypatch.undo()
        O.configure(*G.DEFAULT)


def _misses(ref, key, value):
    return G.rel(value, ref.ld[key]) >= KILL * ref.bar[key]


@grids
def test_mutant_boundary_weight_of_d2(grid, monkeypatch):
    """Row 1 of the second-derivative closure: 10 -15 -4 14 -6 1 with the 14 taken as 16."""
    ref = G.reference(*grid)
    d2 = O._d2_matrix

    def d2_wrong(n, h2, dtype=np.float64):
        A = d2(n, h2, dtype)
        A[1, 3] = 16 / (12 * h2)
        return A

    m = _mutant(ref, monkeypatch, _d2_matrix=d2_wrong)
    assert _misses(ref, "d2ksi", m["d2ksi"]) and _misses(ref, "d2eta", m["d2eta"])
    assert _misses(ref, "J", m["J"])


@grids
def test_mutant_bottom_quirk_is_not_observable(grid, monkeypatch):
    """compute_u_spatial_ders zeroes U_dksi[Bottom] where U_deta[Bottom] was probably meant
    (droplet.py:722).  No bar can see which: the two derivatives reach the compared quantities
    only as A12 U_deta and A12 U_dksi, the Laplace operator's cross-term inputs, and A12 is zero
    on the boundary because dksideta is zeroed there.  (U.dx / U.dy, which do differ, are never
    read by the stepper, and the kernels do not compute them.)  So the "intended" rule is an
    equivalent mutant, on every grid and state: asserted here bit for bit, lest a later change
    make the rule observable without a test that pins it."""
    ref = G.reference(*grid)
    seen = {}

    def u_ders_intended(uval, Q):
        U = O.SimpleNamespace(val=uval)
        ud, ue = O.dksi(uval), O.deta(uval)
        ud[O.IB.Left] = 0
        ud[O.IB.Right] = 0
        ue[O.IB.Top] = 0
        ue[O.IB.Bottom] = 0
        seen["differs"] = bool(np.any(O.dksi(uval)[O.IB.Bottom] != 0))
        U.xx, U.yy = O.laplace(uval, ud, ue, Q)
        return U

    m = _mutant(ref, monkeypatch, u_ders=u_ders_intended)
    assert seen["differs"]
    A12 = ref.f64["A12"].reshape(ref.ny, ref.nx)
    assert not A12[0].any() and not A12[-1].any() and not A12[:, 0].any() and not A12[:, -1].any()
    for k in G.CAP:
        assert np.array_equal(m[k], ref.f64[k]), k


@grids
def test_mutant_dksideta_kept_on_the_boundary(grid, monkeypatch):
    """Seen in dksideta itself and in A12, which is linear in it.  (The state's two cosine modes
    have a cross derivative that vanishes on the boundary, so what the mutant leaves there is the
    one-sided closures' truncation error, ~1e-6 on the large grids: its square is lost in J.)"""
    ref = G.reference(*grid)
    q_ders = O.q_ders

    def q_ders_wrong(qval):
        Q = q_ders(qval)
        Q.dksideta = O.dksideta(qval)
        Q.J = Q.d2ksi * Q.d2eta - Q.dksideta ** 2
        return Q

    m = _mutant(ref, monkeypatch, q_ders=q_ders_wrong)
    for k in ("dksideta", "A12"):
        assert _misses(ref, k, m[k]), k


@pytest.mark.parametrize("grid", [g for g in G.GRIDS if g[0] % 2 or g[1] % 2],
                         ids=[i for i, g in zip(GRID_IDS, G.GRIDS) if g[0] % 2 or g[1] % 2])
def test_mutant_dct_middle_column_counted_twice(grid, monkeypatch):
    """The folded DCT-II of an odd length N feeds the even frequencies s_mid = 2 x_mid at half
    weight; without the halving the middle sample counts twice."""
    ref = G.reference(*grid)

    def solve_pma_wrong(U, Q, LEIG):
        from scipy.fft import dct, idct

        def fwd(a):
            a = a.copy()
            n = a.shape[-1]
            if n % 2:
                a[..., n // 2] *= 2
            return dct(a, norm="ortho")

        mon = O.monitor(U, Q)
        q_rhs = np.sqrt(mon * np.abs(Q.J)) / O.P.alpha
        temp = fwd(fwd(q_rhs.reshape(O.P.Ny, O.P.Nx).T).T)
        dq = idct(idct((temp / (1 - O.P.gamma * LEIG)).T, norm="ortho").T, norm="ortho")
        return dq.reshape(-1)

    m = _mutant(ref, monkeypatch, solve_pma=solve_pma_wrong)
    err, bound = G.pma_error(ref, m["Q5"])
    assert err >= KILL * bound, (err, bound)


SHORT = [g for g in G.GRIDS if G.short_strip(*g) and g[1] - 6 > 5]


FLAT_TOP = [(97, 65), (112, 60)]  # the film is flat (F ~ 0) in the short strip and the one before


@pytest.mark.parametrize("grid", SHORT, ids=[f"{a}x{b}" for a, b in SHORT])
def test_mutant_short_strip_left_stale(grid):
    """The last (ny - 6) % 5 interior rows of a field keep the previous strip's values: in J
    (mesh_stage stores the mesh fields strip by strip), in R and in F of the perturbed state
    (u1 is perturbed everywhere) on every grid with a short strip.  In F of the unperturbed
    state too, except where it cannot show: the droplets do not reach the top rows of the two
    largest grids, and F is 0 to rounding in both strips there -- which is why the GPU tests
    also take the old-time fields of u1."""
    nx, ny = grid
    ref = G.reference(nx, ny)
    nr = G.short_strip(nx, ny)
    i0 = ny - 3 - nr

    def stale(key):
        v = ref.f64[key].reshape(ny, nx).copy()
        v[i0:i0 + nr, 3:nx - 3] = v[i0 - 5:i0 - 5 + nr, 3:nx - 3]
        return v.reshape(-1)

    for key in ("J", "R", "F1", "U_xx1", "U_yy1"):
        assert _misses(ref, key, stale(key)), key
    if grid in FLAT_TOP:
        F = ref.ld["F"].reshape(ny, nx)
        assert np.abs(F[i0 - 5:ny - 3]).max() <= ref.bar["F"] * np.abs(F).max()
    else:
        assert _misses(ref, "F", stale("F"))


def test_short_strip_grids_are_the_expected_ones():
    assert SHORT == [(7, 13), (32, 32), (48, 23), (97, 65), (112, 60)]
    assert [G.short_strip(*g) for g in SHORT] == [2, 1, 2, 4, 4]
    assert G.short_strip(91, 61) == 0 and G.short_strip(7, 7) == 1


# -------------------------------------------------- the kernels' point walks, restated in NumPy
class FastDiv:
    """droplet.hip FastDiv: q = umulhi(t, ceil(2^32 / d)); `fixed`: m == 0 (d == 1, where the
    32-bit multiplier wraps) means "the quotient is t"."""

    def __init__(self, d, fixed):
        self.m = (0xFFFFFFFF // d + 1) & 0xFFFFFFFF
        self.fixed = fixed

    def __call__(self, t):
        if self.m == 0 and self.fixed:
            return t
        return (t * self.m) >> 32


def _ring_point(u, nx, ny, diy, dnx):
    if u < 6 * nx:
        r = dnx(u)
        return (r if r < 3 else ny - 6 + r), u - r * nx
    u -= 6 * nx
    c = diy(u)
    return 3 + (u - c * (ny - 6)), (c if c < 3 else nx - 6 + c)


def for_points(nx, ny, fixed):
    """The (i, j) that droplet.hip's for_points visits, in thread order."""
    ix, iy = nx - 6, ny - 6
    dix, diy, dnx = FastDiv(ix, fixed), FastDiv(iy, fixed), FastDiv(nx, fixed)
    out = []
    for t in range(nx * ny):
        if t < ix * iy:
            q = dix(t)
            out.append((3 + q, 3 + (t - q * ix)))
        else:
            out.append(_ring_point(t - ix * iy, nx, ny, diy, dnx))
    return out


def for_strips(nx, ny, fixed):
    """The interior (i, j) that for_strips' strips store."""
    ix, iy = nx - 6, ny - 6
    ns = (iy + 4) // 5
    dix = FastDiv(ix, fixed)
    out = []
    for t in range(ns * ix):
        s = dix(t)
        i0, j, nr = 3 + 5 * s, 3 + (t - s * ix), min(5, iy - 5 * s)
        out += [(i0 + k, j) for k in range(nr)]
    return out


@grids
def test_point_walks_visit_every_point_once(grid):
    nx, ny = grid
    every = sorted((i, j) for i in range(ny) for j in range(nx))
    inner = sorted((i, j) for i in range(3, ny - 3) for j in range(3, nx - 3))
    assert sorted(for_points(nx, ny, fixed=True)) == every
    assert sorted(for_strips(nx, ny, fixed=True)) == inner


@pytest.mark.parametrize("grid", [(7, 7), (12, 7), (7, 13)], ids=["7x7", "12x7", "7x13"])
def test_mutant_fastdiv_of_one_is_zero(grid):
    """With ceil(2^32/1) wrapped to m = 0 and the quotient taken as umulhi(t, 0) = 0 the walks
    are no permutation of the grid, and a 7-row grid is indexed past its last row."""
    nx, ny = grid
    pts = for_points(nx, ny, fixed=False)
    assert sorted(pts) != sorted((i, j) for i in range(ny) for j in range(nx))
    if ny == 7 and nx > 7:
        assert max(i for i, _ in pts) == 8 >= ny
    if nx == 7:
        assert max(j for _, j in pts) >= nx or len(set(pts)) < nx * ny
    if nx == 7 and ny > 7:
        inner = for_strips(nx, ny, fixed=False)
        assert max(j for _, j in inner) >= nx - 3 or len(set(inner)) < len(inner)


# ---------------------------------------------------------------------- which path a grid takes
def test_lds_fits_states_each_grids_path():
    """nk_drop_lds_fits is the one expression the three launchers share; a change of the LDS cap
    fails here and cannot silently move a test grid to the other path."""
    import nkhip._lib as L
    for nx, ny in G.GRIDS:
        assert L.lib.nk_drop_lds_fits(nx, ny) == int(ny * (nx | 1) <= 6656), (nx, ny)
    assert L.lib.nk_drop_lds_fits(97, 65) == 1 and L.lib.nk_drop_lds_fits(91, 61) == 1
    assert L.lib.nk_drop_lds_fits(112, 60) == 0
    assert L.lib.nk_drop_lds_fits(6, 60) == L.NK_EINVAL
