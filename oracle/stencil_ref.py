"""TEST INFRASTRUCTURE ONLY -- extended-precision reference of every stencil pass form.

One function per mode of ``SMode`` (csrc/nk_kernels.h), written from the formulas stated there and
in ``finish<M>`` (csrc/stencil.hip), in ``np.longdouble`` with periodic rolls on the GLOBAL grid:
no halo rows, no bands, no pairing of the neighbour sums.  A slab's reference is rows
``[row0, row0 + ny)`` of the global result (``rows``).

Each function returns ``(value, mag)``: ``mag`` is the same expression with every term replaced by
its absolute value -- ``|a| + |alpha| |b|`` for the combined field, ``|p0|`` for the point-wise
input, the division by the step included.  It is the scale of the rounding error of ANY fp64
evaluation order of that expression, which gives the per-point bound the tests assert:

    |out - ref| <= BOUND * mag,   BOUND = 64 * eps64.

The bound is derived, not measured.  The longest rounding chain of a pass (FDJVP) has fewer than
24 operations: the combination a + alpha b (2), the paired neighbour sums (3 each), the four
products and three additions of L w, Gfun's square, cube, g w^2, the two subtractions, the halving
and w/k (8), the subtraction of p0 and the reciprocal step (3).  Each rounds relative to a partial
sum that ``mag`` dominates, so the sum is at most gamma_24 mag ~ 24 eps mag, were w exact.  It is
not: w carries the combination's error, which the cubic triples (d(w^3) = 3 w^2 dw) and L and w/k
pass on once; weighting the chain by that factor (at most ~2.7 on average over its terms) gives
24 * 2.7 ~ 64.  The fp64 coefficients (``sh_coef``: a few eps each, no cancellation at e = 2.56)
and the rounded 1/k are inside the same count.

``emulate64`` is a plain fp64 NumPy evaluation of the same passes in the kernel's data layout
(own rows plus two halo rows either side, the combination formed per row, columns wrapped by
index): the CPU tier checks that it stays inside the bound, and that deliberate mutants of it
(``MUTANTS``) leave it by orders of magnitude.  The one long-band GPU case uses it as its
reference for speed.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:
    raise ImportError(
        f"oracle.stencil_ref: np.longdouble has eps = {np.finfo(LD).eps:.3g} here (>= 1e-18): no "
        "extended precision to reference the fp64 stencil passes against")

EPS64 = float(np.finfo(np.float64).eps)
BOUND = 64 * EPS64

LAP5, SH13, RESID, BOLD, TRIAL, FDJVP, AJVP, LINOP = range(8)
MODE_NAMES = ["LAP5", "SH13", "RESID", "BOLD", "TRIAL", "FDJVP", "AJVP", "LINOP"]


def _ld(x):
    return np.asarray(x, dtype=LD)


def _sh(v, dy, dx):
    return np.roll(v, (dy, dx), axis=(0, 1))


def coef(h, r):
    """c0, c1, c2, c3 of L = -Lap^2 - 2 Lap + (r - 1) I with e = 1/h^2, in extended precision."""
    e = LD(1) / (LD(h) * LD(h))
    return -20 * e * e + 8 * e + LD(r) - 1, 8 * e * e - 2 * e, -2 * e * e, -e * e


def _sums(v):
    ax1 = _sh(v, 1, 0) + _sh(v, -1, 0) + _sh(v, 0, 1) + _sh(v, 0, -1)
    dg = _sh(v, 1, 1) + _sh(v, 1, -1) + _sh(v, -1, 1) + _sh(v, -1, -1)
    ax2 = _sh(v, 2, 0) + _sh(v, -2, 0) + _sh(v, 0, 2) + _sh(v, 0, -2)
    return ax1, dg, ax2


def _Lv(v, h, r):
    """L v on the periodic global grid, in v's precision."""
    c0, c1, c2, c3 = (v.dtype.type(c) for c in coef(h, r))
    ax1, dg, ax2 = _sums(v)
    return c0 * v + c1 * ax1 + c2 * dg + c3 * ax2


def _Lm(m, h, r):
    """The same with absolute values, of a field of magnitudes m >= 0."""
    c0, c1, c2, c3 = (abs(m.dtype.type(c)) for c in coef(h, r))
    m1, md, m2 = _sums(m)
    return c0 * m + c1 * m1 + c2 * md + c3 * m2


def _L(v, h, r):
    return _Lv(v, h, r), _Lm(np.abs(v), h, r)


def _G(w, wm, h, r, k, g):
    """G(w) = w/k - (L w + g w^2 - w^3)/2 and its magnitude at |w| <= wm."""
    Lw, Lm = _Lv(w, h, r), _Lm(wm, h, r)
    k, g = w.dtype.type(k), w.dtype.type(g)
    return (w / k - (Lw + g * w * w - w * w * w) / 2,
            wm / abs(k) + (Lm + abs(g) * wm * wm + wm * wm * wm) / 2)


def _comb(a, b, alpha, dtype=LD):
    a, b, alpha = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype), dtype(alpha)
    return a + alpha * b, np.abs(a) + abs(alpha) * np.abs(b)


def lap5(a, e):
    a, e = _ld(a), LD(e)
    s = _sh(a, 1, 0) + _sh(a, -1, 0) + _sh(a, 0, 1) + _sh(a, 0, -1)
    m = np.abs(a)
    sm = _sh(m, 1, 0) + _sh(m, -1, 0) + _sh(m, 0, 1) + _sh(m, 0, -1)
    return e * (s - 4 * a), abs(e) * (sm + 4 * m)


def sh13(a, h, r):
    return _L(_ld(a), h, r)


def resid(u, uo, h, r, k, g):
    """F(u; uo) = (u - uo)/k - (L u + g u^2 - u^3 + L uo + g uo^2 - uo^3)/2."""
    u, uo, k, g = _ld(u), _ld(uo), LD(k), LD(g)
    Lu, Lum = _L(u, h, r)
    Lo, Lom = _L(uo, h, r)
    mu, mo = np.abs(u), np.abs(uo)
    val = (u - uo) / k - (Lu + g * u * u - u * u * u + Lo + g * uo * uo - uo * uo * uo) / 2
    mag = (mu + mo) / abs(k) + (Lum + abs(g) * mu * mu + mu ** 3 + Lom + abs(g) * mo * mo
                                + mo ** 3) / 2
    return val, mag


def bold(uo, h, r, k, g):
    """B(uo) = -uo/k - (L uo + g uo^2 - uo^3)/2, so that F(u) = G(u) + B(uo)."""
    uo, k, g = _ld(uo), LD(k), LD(g)
    Lo, Lom = _L(uo, h, r)
    mo = np.abs(uo)
    return (-uo / k - (Lo + g * uo * uo - uo * uo * uo) / 2,
            mo / abs(k) + (Lom + abs(g) * mo * mo + mo ** 3) / 2)


def trial(a, b, alpha, p0, h, r, k, g, dtype=LD):
    """w = a + alpha b: ((F, G, w), (their magnitudes)) with G = G(w), F = G + p0.  dtype =
    np.float64 only scales the bound of a case too large for extended precision."""
    w, wm = _comb(a, b, alpha, dtype)
    G, Gm = _G(w, wm, h, r, k, g)
    p0 = np.asarray(p0, dtype=dtype)
    return (G + p0, G, w), (Gm + np.abs(p0), Gm, wm)


def fdjvp(a, b, alpha, p0, sc, h, r, k, g):
    """(G(a + alpha b) - p0) / sc."""
    w, wm = _comb(a, b, alpha)
    G, Gm = _G(w, wm, h, r, k, g)
    p0, sc = _ld(p0), LD(sc)
    return (G - p0) / sc, (Gm + np.abs(p0)) / abs(sc)


def ajvp(z, u, alpha, h, r, k, g):
    """alpha (z/k - (L z + (2 g u - 3 u^2) z)/2): the analytic J(u) z, scaled."""
    z, u, alpha, k, g = _ld(z), _ld(u), LD(alpha), LD(k), LD(g)
    Lz, Lzm = _L(z, h, r)
    mz, mu = np.abs(z), np.abs(u)
    return (alpha * (z / k - (Lz + (2 * g * u - 3 * u * u) * z) / 2),
            abs(alpha) * (mz / abs(k) + (Lzm + (2 * abs(g) * mu + 3 * mu * mu) * mz) / 2))


def linop(a, b, alpha, p0, theta, h, r):
    """w = a + alpha b: ((A w, w), (magnitudes)) with A w = (1 + p0) w - theta L w."""
    w, wm = _comb(a, b, alpha)
    Lw, Lm = _Lv(w, h, r), _Lm(wm, h, r)
    p0, theta = _ld(p0), LD(theta)
    return ((1 + p0) * w - theta * Lw, w), ((1 + np.abs(p0)) * wm + abs(theta) * Lm, wm)


def dev_scale(mode, znorm2, omega):
    """(alpha, sc) of a device-scaled JVP as ``jvp_scale`` documents: v = z_raw / |z_raw|,
    FDJVP: sc = omega / |v| = omega, alpha = sc / |z_raw|; AJVP: alpha = 1 / |z_raw|."""
    hn = np.sqrt(LD(znorm2))
    if mode == FDJVP:
        return LD(omega) / hn, LD(omega)
    return LD(1) / hn, LD(1)


def spec_scale(spec, thr, ftol, rdiff, zn, zs):
    """(go, alpha, sc) of the speculative FDJVP from spec = (sum F^2, max|F|, max|x|): it runs if
    the trial passed (finite sum F^2 <= thr) and the iteration goes on (not max|F| <= ftol), at
    the host's step omega = rdiff max(1, max|x|) / max(1, max|F|), sc = omega / zn, alpha = sc zs."""
    red0, fm, xm = (float(s) for s in spec)
    go = bool(np.isfinite(red0) and red0 <= thr and not fm <= ftol)
    omega = LD(rdiff) * max(LD(1), LD(xm)) / max(LD(1), LD(fm))
    sc = omega / LD(zn)
    return go, sc * LD(zs), sc


def rows(x, row0, ny):
    """Rows [row0, row0 + ny) of a global result (or of each member of a tuple of results)."""
    if isinstance(x, tuple):
        return tuple(rows(v, row0, ny) for v in x)
    return x[row0:row0 + ny]


def halo_of(glob, row0, ny):
    """The 4 halo rows (global rows row0-2, row0-1, row0+ny, row0+ny+1, periodic) of a slab."""
    n = glob.shape[0]
    idx = [(row0 - 2) % n, (row0 - 1) % n, (row0 + ny) % n, (row0 + ny + 1) % n]
    return np.ascontiguousarray(glob[idx])


def ratio(out, ref, mag, bound=BOUND):
    """max over points of |out - ref| / (bound mag), NaN-propagating (points with mag == 0 must
    match exactly)."""
    d = np.abs(_ld(out) - ref)
    b = LD(bound) * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, d / np.where(b > 0, b, 1), np.where(d > 0, np.inf, 0.0))
    if np.isnan(np.asarray(d, dtype=np.float64)).any():
        return float("nan")
    return float(q.max())


# ----------------------------------------------------------------------------------------------
# fp64 evaluation in the kernel's layout
# ----------------------------------------------------------------------------------------------
MUTANTS = ("wrap", "halo_alpha", "swap", "ik")


def emulate64(mode, a, b=None, p0=None, *, alpha=0.0, sc=1.0, e=0.0, theta=0.0,
              h=0.625, r=0.01, k=0.2, g=1.0, a_halo=None, b_halo=None, mutant=None):
    """One pass in fp64 on a slab a (ny, nx) with its halo rows (4, nx; None: periodic), as the
    kernels lay it out: a window of own and halo rows, w = a + alpha b formed row by row, side
    columns by wrapped index, the symmetric pairs of the neighbour sums, 1/k and the reciprocal
    step as factors.  Returns out0, or (out0, out1, out2) for TRIAL and (out0, out2) for LINOP.

    mutant (tests only): "wrap" -- the column wrap at c + 2 lands one column off; "halo_alpha" --
    the halo rows enter the window without alpha b; "swap" -- the diagonal and the axial-2
    coefficients change places; "ik" -- the factor that should be 1/k is not (k itself).
    """
    assert mutant is None or mutant in MUTANTS
    f8 = np.float64
    a = np.asarray(a, dtype=f8)
    ny, nx = a.shape

    def window(f, halo):
        f = np.asarray(f, dtype=f8)
        if halo is None:
            idx = np.arange(-2, ny + 2) % ny
            return f[idx]
        return np.concatenate([halo[:2], f, halo[2:]], axis=0)

    W = window(a, a_halo)
    if mode in (TRIAL, FDJVP, LINOP):
        Wb = window(b, b_halo)
        comb = W + f8(alpha) * Wb
        if mutant == "halo_alpha":
            comb[:2] = W[:2]
            comb[-2:] = W[-2:]
        W = comb
    cols = np.arange(nx)

    def at(win, di, dj):
        own = win[2 + di:2 + di + ny]
        if mutant == "wrap" and dj == 2:
            return own[:, np.where(cols + 2 >= nx, (cols + 3) % nx, (cols + 2) % nx)]
        return np.roll(own, -dj, axis=1) if dj else own

    def nb(win):
        c = at(win, 0, 0)
        a1 = (at(win, 0, -1) + at(win, 0, 1)) + (at(win, -1, 0) + at(win, 1, 0))
        dg = (at(win, -1, -1) + at(win, -1, 1)) + (at(win, 1, -1) + at(win, 1, 1))
        a2 = (at(win, 0, -2) + at(win, 0, 2)) + (at(win, -2, 0) + at(win, 2, 0))
        return c, a1, dg, a2

    ee = f8(1.0) / (f8(h) * f8(h))
    c0 = f8(-20.0) * ee * ee + f8(8.0) * ee + f8(r) - f8(1.0)
    c1 = f8(8.0) * ee * ee - f8(2.0) * ee
    c2 = f8(-2.0) * ee * ee
    c3 = -ee * ee
    if mutant == "swap":
        c2, c3 = c3, c2
    kk, gg = f8(k), f8(g)
    ik = kk if mutant == "ik" else f8(1.0) / kk

    def L(n):
        return c0 * n[0] + c1 * n[1] + c2 * n[2] + c3 * n[3]

    def G(n):
        w = n[0]
        ww = w * w
        return w * ik - (L(n) + gg * ww - w * ww) / 2

    na = nb(W)
    if p0 is not None:
        p0 = np.asarray(p0, dtype=f8)
    if mode == LAP5:
        return f8(e) * (na[1] - 4.0 * na[0])
    if mode == SH13:
        return L(na)
    if mode == RESID:
        n2 = nb(window(b, b_halo))
        u, uo = na[0], n2[0]
        uu, oo = u * u, uo * uo
        return (u - uo) / kk - (L(na) + gg * uu - u * uu + L(n2) + gg * oo - uo * oo) / 2
    if mode == BOLD:
        uo = na[0]
        oo = uo * uo
        return -uo * ik - (L(na) + gg * oo - uo * oo) / 2
    if mode == TRIAL:
        Gw = G(na)
        return Gw + p0, Gw, na[0]
    if mode == FDJVP:
        return (G(na) - p0) * (f8(1.0) / f8(sc))
    if mode == AJVP:
        z, u = na[0], p0
        return f8(alpha) * (z * ik - (L(na) + (2.0 * gg * u - 3.0 * u * u) * z) / 2)
    if mode == LINOP:
        return (1.0 + p0) * na[0] - f8(theta) * L(na), na[0]
    raise ValueError(mode)
