"""GPU: every form of the stencil pass the solver launches, against the extended-precision
reference of the same operation (oracle/stencil_ref.py), point by point.

The passes run through ``nkhip.ops.stencil_pass`` (nk_debug_stencil: the solver's own
``stencil_launch`` on caller tensors).  Every output is prefilled with a NaN sentinel, so a point
the pass did not write fails the bound, and a point it should not have written is seen bitwise.
The per-point bound is ``|out - ref| <= 64 eps mag`` (derived in the oracle's docstring); the
largest ratios observed are recorded in profiles/stencil_passes.md.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import stencil_ref as sr

pytestmark = pytest.mark.gpu

H, R, K, G = 0.625, 0.01, 0.2, 1.0
PHYS = dict(h=H, r=R, k=K, g=G)
ALPHA, THETA, SC = 0.37, 0.1, 1e-4
EPS = sr.EPS64

# (ny, nx, off): off = every tensor is an 8-byte-offset view, which the point kernel takes
MARCH = [(2, 2), (3, 4), (7, 254), (13, 256), (8, 258), (14, 512), (9, 600), (20, 1026)]
POINT = [(5, 7, False), (1, 6, False), (8, 258, True)]
SHAPES = [(ny, nx, False) for ny, nx in MARCH] + POINT
_ids = [f"{ny}x{nx}{'v' if off else ''}" for ny, nx, off in SHAPES]


def _dev(x, off=False):
    x = np.array(x, dtype=np.float64).reshape(-1)  # a writable copy for torch.from_numpy
    buf = torch.empty(x.size + 2, dtype=torch.float64, device="cuda")
    view = buf[1:1 + x.size] if off else buf[2:]
    view.copy_(torch.from_numpy(x))
    return view


def _sent(n, off=False):
    buf = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda")
    return buf[1:1 + n] if off else buf[2:]


def _np(t, shape=None):
    x = t.cpu().numpy()
    return x if shape is None else x.reshape(shape)


def _is_sent(x):
    """bitwise the sentinel torch.full wrote (not merely some NaN)"""
    s = np.array([float("nan")]).view(np.int64)[0]
    return np.asarray(x).view(np.int64) == s


def _same(x, y):
    return np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64))


@functools.lru_cache(maxsize=None)
def _inputs(ny, nx):
    rng = np.random.default_rng(7919 * ny + nx)
    a, b, p0 = (rng.standard_normal((ny, nx)) for _ in range(3))
    for x in (a, b, p0):
        x.setflags(write=False)
    return a, b, p0


# name -> (mode, outputs the pass writes)
VARIANTS = {
    "LAP5": ("LAP5", ("out0",)),
    "SH13": ("SH13", ("out0",)),
    "RESID": ("RESID", ("out0",)),
    "BOLD": ("BOLD", ("out0",)),
    "TRIAL": ("TRIAL", ("out0", "out1", "out2")),
    "TRIAL_no_out2": ("TRIAL", ("out0", "out1")),
    "TRIAL_alias": ("TRIAL", ("out0", "out1", "out2")),
    "FDJVP": ("FDJVP", ("out0",)),
    "AJVP": ("AJVP", ("out0",)),
    "LINOP": ("LINOP", ("out0", "out2")),
}


def _fd_alpha(b):
    zs = 1.0 / float(np.linalg.norm(b))
    return SC * zs  # the fp64 product nk_sh_fdjvp and SHProblem::jvp pass as alpha


def _reference(variant, a, b, p0):
    """{output: (ref, mag)} on the global grid, and the pass's keyword arguments."""
    mode = VARIANTS[variant][0]
    if variant == "LAP5":
        return {"out0": sr.lap5(a, 1 / H ** 2)}, dict(e=1 / H ** 2)
    if variant == "SH13":
        return {"out0": sr.sh13(a, H, R)}, {}
    if variant == "RESID":
        return {"out0": sr.resid(a, b, H, R, K, G)}, {}
    if variant == "BOLD":
        return {"out0": sr.bold(a, H, R, K, G)}, {}
    if mode == "TRIAL":
        v, m = sr.trial(a, a if variant == "TRIAL_alias" else b, ALPHA, p0, H, R, K, G)
        return dict(zip(("out0", "out1", "out2"), zip(v, m))), dict(alpha=ALPHA)
    if variant == "FDJVP":
        al = _fd_alpha(b)
        return {"out0": sr.fdjvp(a, b, al, p0, SC, H, R, K, G)}, dict(alpha=al, sc=SC)
    if variant == "AJVP":
        return {"out0": sr.ajvp(a, p0, ALPHA, H, R, K, G)}, dict(alpha=ALPHA)
    v, m = sr.linop(a, b, ALPHA, p0, THETA, H, R)
    return dict(zip(("out0", "out2"), zip(v, m))), dict(alpha=ALPHA, theta=THETA)


@functools.lru_cache(maxsize=None)
def _ref_periodic(variant, ny, nx):
    return _reference(variant, *_inputs(ny, nx))


class Pass:
    """One pass's device tensors: inputs uploaded once, outputs fresh sentinels per run."""

    def __init__(self, variant, ny, nx, a, b, p0, off=False, a_halo=None, b_halo=None, **kw):
        self.mode, self.outs = VARIANTS[variant]
        self.ny, self.nx, self.off = ny, nx, off
        m = self.mode
        self.t = {"a": _dev(a, off)}
        if m in ("RESID", "TRIAL", "FDJVP", "LINOP"):
            self.t["b"] = self.t["a"] if variant == "TRIAL_alias" else _dev(b, off)
        if m in ("TRIAL", "FDJVP", "AJVP", "LINOP"):
            self.t["p0"] = _dev(p0, off)
        if a_halo is not None:
            self.t["a_halo"] = _dev(a_halo, off)
            if "b" in self.t:
                self.t["b_halo"] = (self.t["a_halo"] if variant == "TRIAL_alias"
                                    else _dev(b_halo, off))
        self.kw = dict(PHYS, **kw)

    def fresh(self):
        return {k: _sent(self.ny * self.nx, self.off) for k in self.outs}

    def run(self, out=None, **kw):
        """-> ({output: numpy (ny, nx)}, red, nblk); out: tensors to write into (else fresh)"""
        from nkhip import ops
        out = self.fresh() if out is None else out
        args = dict(self.t, **{k: v for k, v in out.items() if k != "out0"})
        red, nblk = ops.stencil_pass(self.mode, self.ny, self.nx, args.pop("a"), out["out0"],
                                     **args, **dict(self.kw, **kw))
        return {k: _np(v, (self.ny, self.nx)) for k, v in out.items()}, red, nblk


def _check_bound(got, ref, row0=0, ny=None, scale=1.0, what=""):
    """every output within the bound of its reference rows; returns the largest ratio"""
    worst = 0.0
    for k, o in got.items():
        f, m = ref[k]
        if ny is not None:
            f, m = sr.rows(f, row0, ny), sr.rows(m, row0, ny)
        q = sr.ratio(o, f, m, sr.BOUND * scale)
        print(f"{what} {k}: |out - ref| / bound = {q:.4f}")
        assert q <= 1.0, (what, k, q)
        worst = max(worst, q)
    return worst


# ------------------------------------------------------------------------------------------
# a. every mode on the periodic grid, both walks
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx,off", SHAPES, ids=_ids)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mode_periodic_both_walks(variant, ny, nx, off):
    a, b, p0 = _inputs(ny, nx)
    ref, kw = _ref_periodic(variant, ny, nx)
    P = Pass(variant, ny, nx, a, b, p0, off, **kw)
    got0, red0, nblk0 = P.run(rev=0)
    got1, red1, nblk1 = P.run(rev=1)
    _check_bound(got0, ref, what=f"{variant} {ny}x{nx} rev=0")
    _check_bound(got1, ref, what=f"{variant} {ny}x{nx} rev=1")
    for k in got0:
        assert _same(got0[k], got1[k]), k
    assert nblk0 == nblk1 and nblk0 >= 1
    assert _same(np.array(red0), np.array(red1)), (red0, red1)  # partials are slotted by band


# ------------------------------------------------------------------------------------------
# b. reductions
# ------------------------------------------------------------------------------------------
def _sum_check(value, x, y, what):
    """value = sum x y over the kernel's own outputs, every stored point counted once"""
    t = np.asarray(x, dtype=np.longdouble) * np.asarray(y, dtype=np.longdouble)
    own = t.sum()
    tol = x.size * EPS * np.abs(t).sum()
    print(f"{what}: |red - sum own| = {float(abs(value - own)):.3e}, allowed {float(tol):.3e}")
    assert abs(value - own) <= tol, what


def _sum_ref_check(value, fx, mx, fy, my, what):
    """... and within the propagated per-point bounds of the reference sum"""
    n = fx.size
    bx, by = sr.BOUND * mx, sr.BOUND * my
    tol = (np.abs(fx) * by + np.abs(fy) * bx).sum() + n * EPS * np.abs(fx * fy).sum()
    d = abs(value - (fx * fy).sum())
    print(f"{what}: |red - sum ref| = {float(d):.3e}, allowed {float(tol):.3e}")
    assert d <= tol, what


@pytest.mark.parametrize("ny,nx,off", SHAPES, ids=_ids)
@pytest.mark.parametrize("variant", ["TRIAL", "TRIAL_no_out2", "LINOP"])
def test_reductions(variant, ny, nx, off):
    a, b, p0 = _inputs(ny, nx)
    ref, kw = _ref_periodic(variant, ny, nx)
    got, red, nblk = Pass(variant, ny, nx, a, b, p0, off, **kw).run(rev=0)
    what = f"{variant} {ny}x{nx}"
    if variant == "LINOP":
        _sum_check(red[0], got["out2"], got["out0"], what)
        (f2, m2), (f0, m0) = ref["out2"], ref["out0"]
        _sum_ref_check(red[0], f2, m2, f0, m0, what)
        return
    F = got["out0"]
    assert red[1] == np.abs(F).max()
    _sum_check(red[0], F, F, what)
    f0, m0 = ref["out0"]
    _sum_ref_check(red[0], f0, m0, f0, m0, what)  # 2 sum |F_ref| bound_p + n eps sum F_ref^2
    if "out2" in got:
        assert red[2] == np.abs(got["out2"]).max()
    else:  # no stored w to compare with: the reference's, within its bound
        w, wm = ref["out2"]
        assert abs(red[2] - np.abs(w).max()) <= sr.BOUND * wm.max()


@pytest.mark.parametrize("ny,nx,off", [(13, 256, False), (9, 600, False), (5, 7, False)],
                         ids=["13x256", "9x600", "5x7"])
def test_nan_in_p0_reaches_max_F(ny, nx, off):
    a, b, p0 = _inputs(ny, nx)
    p0 = p0.copy()
    p0[ny - 1, nx - 2] = float("nan")
    _, red, _ = Pass("TRIAL", ny, nx, a, b, p0, off, alpha=ALPHA).run(rev=0)
    assert math.isnan(red[1]) and math.isnan(red[0]) and not math.isnan(red[2])


# ------------------------------------------------------------------------------------------
# c. device scales
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx,off", [(13, 256, False), (9, 600, False), (20, 1026, False),
                                       (5, 7, False), (8, 258, True)],
                         ids=["13x256", "9x600", "20x1026", "5x7", "8x258v"])
@pytest.mark.parametrize("variant", ["FDJVP", "AJVP"])
def test_device_scales(variant, ny, nx, off):
    a, b, p0 = _inputs(ny, nx)
    z = b if variant == "FDJVP" else a
    zn2 = float(np.dot(z.reshape(-1), z.reshape(-1)))
    omega = 3e-4
    al, sc = sr.dev_scale(sr.MODE_NAMES.index(variant), zn2, omega)
    if variant == "FDJVP":
        ref = {"out0": sr.fdjvp(a, b, al, p0, sc, H, R, K, G)}
    else:
        ref = {"out0": sr.ajvp(a, p0, al, H, R, K, G)}
    P = Pass(variant, ny, nx, a, b, p0, off)
    zt = _dev(np.array([zn2]))
    got, _, _ = P.run(znorm2=zt, omega=omega, rev=0)
    _check_bound(got, ref, what=f"{variant} device scale {ny}x{nx}")
    # the host-scale call at the same step, formed in fp64 as jvp_scale forms it
    hn = math.sqrt(zn2)
    sig = 1.0 / hn
    if variant == "FDJVP":
        hsc = omega / (sig * hn)
        host, _, _ = P.run(alpha=hsc * sig, sc=hsc, rev=0)
    else:
        host, _, _ = P.run(alpha=sig, rev=0)
    q = sr.ratio(got["out0"], np.asarray(host["out0"], dtype=np.longdouble), ref["out0"][1],
                 8 * EPS)
    print(f"{variant} device vs host scale {ny}x{nx}: ratio to 8 eps mag = {q:.4f}")
    assert q <= 1.0


# ------------------------------------------------------------------------------------------
# d. speculative gate
# ------------------------------------------------------------------------------------------
SPEC = dict(spec_thr=2.0, spec_ftol=1e-9, spec_rdiff=1e-3, spec_zn=2.0)


@pytest.mark.parametrize("ny,nx", [(14, 512), (5, 7)], ids=["march", "point"])
def test_speculative_gate(ny, nx):
    from nkhip import ops
    a, b, p0 = _inputs(ny, nx)
    march = nx % 2 == 0
    zs = 0.5 / float(np.linalg.norm(b))
    P = Pass("FDJVP", ny, nx, a, b, p0, spec_zs=zs, **SPEC)
    ne = int(ops.edge_gather(P.t["a"], ny, nx).numel()) if march else 0

    def run(vals):
        out = P.fresh()
        E0 = _sent(ne) if march else None
        got, _, _ = P.run(out=out, spec=_dev(np.array(vals)), E0=E0, rev=0)
        return got["out0"], (_np(E0) if march else None), out["out0"]

    vals = (1.5, 12.5, 3.75)  # sum F^2 <= thr, max|F| > ftol: the pass goes
    go, al, sc = sr.spec_scale(vals, SPEC["spec_thr"], SPEC["spec_ftol"], SPEC["spec_rdiff"],
                               SPEC["spec_zn"], zs)
    assert go
    out0, E0, t0 = run(vals)
    _check_bound({"out0": out0}, {"out0": sr.fdjvp(a, b, al, p0, sc, H, R, K, G)},
                 what=f"spec go {ny}x{nx}")
    if march:
        assert _same(E0, _np(ops.edge_gather(t0, ny, nx)))
    for vals in [(float("nan"), 12.5, 3.75), (2.5, 12.5, 3.75), (1.5, 1e-9, 3.75)]:
        assert not sr.spec_scale(vals, SPEC["spec_thr"], SPEC["spec_ftol"], SPEC["spec_rdiff"],
                                 SPEC["spec_zn"], zs)[0]
        out0, E0, _ = run(vals)
        assert _is_sent(out0).all(), vals
        if march:
            assert _is_sent(E0).all(), vals


# ------------------------------------------------------------------------------------------
# e. slabs and row ranges   f. edge arrays   g. pushed rows
# ------------------------------------------------------------------------------------------
SLABS = [(24, 512, 3), (27, 130, 3), (16, 7, 2)]
SLAB_MODES = ["FDJVP", "AJVP", "TRIAL", "BOLD"]


@functools.lru_cache(maxsize=None)
def _ref_global(variant, gy, nx):
    return _reference(variant, *_inputs(gy, nx))


def _slab_pass(variant, gy, nx, nslab, p, **extra):
    a, b, p0 = _inputs(gy, nx)
    ny = gy // nslab
    row0 = p * ny
    sl = slice(row0, row0 + ny)
    _, kw = _ref_global(variant, gy, nx)
    return Pass(variant, ny, nx, a[sl], b[sl], p0[sl], a_halo=sr.halo_of(a, row0, ny),
                b_halo=sr.halo_of(b, row0, ny), **dict(kw, **extra)), row0, ny


def _three_launches(P, ny, after=None, **kw):
    """the pass as SHProblem::halo_stencil splits it; after(i, range, out): hook per launch"""
    out = P.fresh()
    reds = []
    done = np.zeros(ny, dtype=bool)
    for i, (r0, r1) in enumerate([(2, ny - 2), (0, 2), (ny - 2, ny)]):
        got, red, _ = P.run(out=out, rows=(r0, r1), **kw)
        done[r0:r1] = True
        for k, o in got.items():  # rows outside the ranges launched so far: still the sentinel
            assert _is_sent(o[~done]).all(), (k, r0, r1)
            assert not np.isnan(o[done]).any(), (k, r0, r1)
        reds.append(red)
        if after:
            after(i, (r0, r1), out)
    return got, reds


@pytest.mark.parametrize("gy,nx,nslab", SLABS, ids=["24x512", "27x130", "16x7"])
@pytest.mark.parametrize("variant", SLAB_MODES)
def test_slabs_and_row_ranges(variant, gy, nx, nslab):
    ref, _ = _ref_global(variant, gy, nx)
    for p in range(nslab):
        P, row0, ny = _slab_pass(variant, gy, nx, nslab, p)
        whole, red, _ = P.run(rev=p % 2)
        _check_bound(whole, ref, row0, ny, what=f"{variant} slab {p} of {gy}x{nx}")
        parts, reds = _three_launches(P, ny, rev=(p + 1) % 2)
        for k in whole:
            assert _same(whole[k], parts[k]), (k, p)
        if variant == "TRIAL":  # the three launches' reductions cover the slab once
            assert max(r[1] for r in reds) == red[1] and max(r[2] for r in reds) == red[2]
            F = whole["out0"].astype(np.longdouble)
            assert abs(sum(r[0] for r in reds) - red[0]) <= F.size * EPS * float((F * F).sum())


EDGE_SHAPES = [(14, 512), (9, 600), (13, 256)]
EDGE_MODES = ["TRIAL", "FDJVP", "AJVP", "BOLD"]


def _edge_kw(P, ny, nx, inputs=True):
    """edge arrays of the pass's fields (as SHProblem::side_edges) and sentinel output arrays"""
    from nkhip import ops
    kw = {}
    if inputs:
        kw["Ea"] = ops.edge_gather(P.t["a"], ny, nx)
        if "b" in P.t and P.mode != "RESID":
            kw["Eb"] = ops.edge_gather(P.t["b"], ny, nx)
    ne = int(ops.edge_gather(P.t["a"], ny, nx).numel())
    kw["E0"] = _sent(ne)
    if "out2" in P.outs and P.mode == "TRIAL":
        kw["E2"] = _sent(ne)
    return kw


def _check_edges_out(out, ekw, ny, nx):
    from nkhip import ops
    for e, o in (("E0", "out0"), ("E2", "out2")):
        if e in ekw:
            E = _np(ekw[e])
            assert not np.isnan(E).any(), e
            assert _same(E, _np(ops.edge_gather(out[o], ny, nx))), e


@pytest.mark.parametrize("ny,nx", EDGE_SHAPES, ids=["14x512", "9x600", "13x256"])
@pytest.mark.parametrize("variant", EDGE_MODES)
def test_edge_arrays_periodic(variant, ny, nx):
    a, b, p0 = _inputs(ny, nx)
    _, kw = _ref_periodic(variant, ny, nx)
    P = Pass(variant, ny, nx, a, b, p0, **kw)
    plain, red, _ = P.run(rev=0)
    for rev in (0, 1):
        ekw = _edge_kw(P, ny, nx)
        out = P.fresh()
        got, red_e, _ = P.run(out=out, rev=rev, **ekw)
        for k in plain:
            assert _same(plain[k], got[k]), (k, rev)
        assert _same(np.array(red), np.array(red_e))
        _check_edges_out(out, ekw, ny, nx)


@pytest.mark.parametrize("variant", EDGE_MODES)
def test_edge_arrays_slab(variant):
    gy, nx, nslab = SLABS[0]
    for p in range(nslab):
        P, row0, ny = _slab_pass(variant, gy, nx, nslab, p)
        plain, _, _ = P.run(rev=0)
        ekw = _edge_kw(P, ny, nx)
        out = P.fresh()
        got, _, _ = P.run(out=out, rev=1, **ekw)
        for k in plain:
            assert _same(plain[k], got[k]), (k, p)
        _check_edges_out(out, ekw, ny, nx)
        # the three-launch composition: the same outputs, and no sentinel left in E0 / E2
        ekw = _edge_kw(P, ny, nx)
        last = {}
        parts, _ = _three_launches(P, ny, after=lambda i, rg, o: last.update(o), **ekw)
        for k in plain:
            assert _same(plain[k], parts[k]), (k, p)
        _check_edges_out(last, ekw, ny, nx)


def test_point_kernel_refuses_edge_arrays():
    from nkhip import NKError
    ny, nx = 5, 7
    a, b, p0 = _inputs(ny, nx)
    P = Pass("TRIAL", ny, nx, a, b, p0, alpha=ALPHA)
    for name in ("Ea", "Eb", "E0", "E2"):
        out = P.fresh()
        with pytest.raises(NKError):
            P.run(out=out, **{name: _sent(4 * ny)})
        assert all(_is_sent(_np(o)).all() for o in out.values()), name
    # ... and an even grid through unaligned views, which only the point kernel takes
    ny, nx = 8, 258
    P = Pass("FDJVP", ny, nx, *_inputs(ny, nx), off=True, alpha=1e-4, sc=1e-4)
    with pytest.raises(NKError):
        P.run(E0=_sent(2 * 4 * ny))


@pytest.mark.parametrize("variant", ["TRIAL", "FDJVP", "AJVP"])
@pytest.mark.parametrize("split", [False, True], ids=["whole", "three_launches"])
def test_pushed_rows(variant, split):
    gy, nx, nslab = SLABS[0]
    ld = nx + 8
    for p in range(nslab):
        P, row0, ny = _slab_pass(variant, gy, nx, nslab, p)
        plain, _, _ = P.run(rev=0)
        slots = {k: (_sent(4 * ld), _sent(4 * ld))
                 for k in (("PS0", "PS2") if variant == "TRIAL" else ("PS0",))}
        kw = dict(_edge_kw(P, ny, nx, inputs=False), ps_ld=ld, **slots)
        if split:
            got, _ = _three_launches(P, ny, **kw)
        else:
            got, _, _ = P.run(rev=1, **kw)
        for k in plain:
            assert _same(plain[k], got[k]), (k, p)
        for s, o in (("PS0", "out0"), ("PS2", "out2")):
            if s not in slots:
                continue
            prev, nxt = (_np(t, (4, ld)) for t in slots[s])
            assert _same(prev[2:4, :nx], got[o][0:2]), (s, p)
            assert _same(nxt[0:2, :nx], got[o][ny - 2:ny]), (s, p)
            assert _is_sent(prev[0:2]).all() and _is_sent(prev[:, nx:]).all(), (s, p)
            assert _is_sent(nxt[2:4]).all() and _is_sent(nxt[:, nx:]).all(), (s, p)


# ------------------------------------------------------------------------------------------
# h. one long-band case
# ------------------------------------------------------------------------------------------
def test_trial_long_bands():
    """TRIAL at 2310 x 4096: the smallest grid whose bands are 12 rows (ny gx >= 36864), the last
    one ragged.  Reference: the fp64 NumPy evaluation (extended precision would take minutes), so
    both sides round and the bound is doubled."""
    ny, nx = 2310, 4096
    rng = np.random.default_rng(2310)
    a, b, p0 = (rng.standard_normal((ny, nx)) for _ in range(3))
    ref = sr.emulate64(sr.TRIAL, a, b, p0, alpha=ALPHA, **PHYS)
    _, mag = sr.trial(a, b, ALPHA, p0, H, R, K, G, dtype=np.float64)
    P = Pass("TRIAL", ny, nx, a, b, p0, alpha=ALPHA)
    got0, red0, nblk = P.run(rev=0)
    assert nblk == 16 * math.ceil(ny / 12)
    for k, f, m in zip(("out0", "out1", "out2"), ref, mag):
        d = np.abs(got0[k] - f)
        q = float((d / (2 * sr.BOUND * m)).max())
        print(f"TRIAL long bands {k}: |out - fp64| / (2 bound) = {q:.4f}")
        assert q <= 1.0, k
    assert red0[1] == np.abs(got0["out0"]).max() and red0[2] == np.abs(got0["out2"]).max()
    _sum_check(red0[0], got0["out0"], got0["out0"], "TRIAL long bands")
    got1, red1, _ = P.run(rev=1)
    for k in got0:
        assert _same(got0[k], got1[k]), k
    assert _same(np.array(red0), np.array(red1))
