"""Swift-Hohenberg Crank-Nicolson stepper: the reference's call surface over libnkhip.

The reference script ``python_work/sh_scipy_nk.py`` (and its duplicate ``sh_vscode_nk.py``, and
the C++ twin ``cpp_work/.../main.cpp``) is a module-level loop:

    L = -Lap*Lap - 2*Lap + (r-1)*I                       # :38-39
    for s in range(Nsteps):                              # :53
        Uo = U.copy(); UoUo = Uo*Uo; UoUoUo = Uo*UoUo    # :56-58
        U = newton_krylov(residual, Uo, verbose=1)       # :61

``SwiftHohenberg`` keeps those parameters (d, N, h = d/N, k, r, g; defaults = the reference
constants :15-29) and ``step(U)`` is the loop body: hand in a 2-D grid state, get the next
implicit time step.  The whole Newton-Krylov solve runs on the GPU (nk_sh_step): the residual,
the finite-difference JVP and the Arnoldi BLAS-1 work are HIP kernels, the host keeps scalars.

``run_batch`` / ``step_batch`` serve small grids (ny*N <= ``resident_max_points``) and ensembles of
them: one workgroup per state runs whole implicit steps on chip, Newton-CG with the analytic
Jacobian, in one launch for the batch (csrc/sh_resident.hip).  ``precond="spectral"`` preconditions
CG inside the workgroup on power-of-two sides, ``precond="spectral-mixed"`` on even sides
2^a 3^b 5^c in [6, 128] that are not both powers of two (csrc/sh_resident_pcm.hip).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import check, lib
from .solver import make_opts, raise_for_status, NoConvergence  # noqa: F401


class SwiftHohenberg:
    """u_t = r u - (1 + lap)^2 u + g u^2 - u^3 on a periodic N x N torus (sh_scipy_nk.py)."""

    def __init__(self, N: int = 64, d: float = 40.0, k: float = 0.2, r: float = 0.01,
                 g: float = 1.0, *, ny: int | None = None, jvp: str = "fd", f_tol=None,
                 f_rtol=None, x_tol=None, x_rtol=None, maxiter=None, rdiff=None, outer_k=10,
                 inner_m=30, line_search="armijo", verbose=False, profile=False,
                 comm=None, ny_local: int | None = None, stream=None, inner_M=None):
        self.N = int(N)          # points in x (and in y unless ny is given)
        self.nx = int(N)
        self.ny = int(ny) if ny is not None else int(N)
        self.d = float(d)
        self.h = self.d / self.N  # sh_scipy_nk.py:17
        self.k = float(k)
        self.r = float(r)
        self.g = float(g)
        self.e = 1.0 / self.h ** 2  # :32
        self.comm = comm
        self.ny_local = int(ny_local) if ny_local is not None else self.ny
        self.opts = make_opts(rdiff=rdiff, outer_k=outer_k, verbose=verbose, maxiter=maxiter,
                              f_tol=f_tol, f_rtol=f_rtol, x_tol=x_tol, x_rtol=x_rtol,
                              line_search=line_search, inner_m=inner_m, jvp=jvp,
                              profile=profile)
        self._stream = stream
        self._h = C.c_void_p()
        s = self._stream_ptr()
        check(lib.nk_sh_create(C.byref(self._h), self.ny_local, self.nx, self.ny, self.h, self.r,
                               self.k, self.g, C.byref(self.opts),
                               comm.handle if comm is not None else None, s), "nk_sh_create")
        self.last_stats = None
        self.last_batch = None  # per-member results of the last run_batch
        self.last_batch_state = None  # its U_new: the survivors' states when it raised
        self.inner_M = None
        if inner_M is not None:
            try:
                self.set_precond(inner_M)
            except Exception:
                self.close()
                raise

    def _stream_ptr(self):
        st = self._stream if self._stream is not None else torch.cuda.current_stream()
        return C.c_void_p(st.cuda_stream)

    def close(self):
        if self._h:
            lib.nk_sh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    # ----------------------------------------------------------------------------- options
    def set_options(self, **kw):
        o = make_opts(**kw)
        check(lib.nk_sh_set_opts(self._h, C.byref(o)), "nk_sh_set_opts")
        self.opts = o

    def set_precond(self, kind):
        """Preconditioner of the inner LGMRES solves, scipy's ``inner_M``: ``None`` / ``"none"`` /
        ``NK_PC_NONE`` (the unpreconditioned solver, exactly) or ``"spectral"`` /
        ``NK_PC_SPECTRAL``, the exact inverse of the Jacobian's linear part I/k - L/2 applied with
        hand-written FFT passes (``ops.sh_precond``).  Spectral needs a single slab (no ``comm``),
        nx and ny powers of two in [8, 16384] and k r < 2; anything else raises and leaves the
        stepper as it was.  ``"spectral-mixed"`` / ``NK_PC_SPECTRAL_MIXED`` is the same operator on
        more grids: sides that are both even, of the form 2^a 3^b 5^c and in [6, 4096] as well
        (``ops.sh_precond(..., mixed=True)``); it is a name of its own because ``"spectral"``
        refuses such sides by contract."""
        names = {None: _lib.NK_PC_NONE, "none": _lib.NK_PC_NONE, "spectral": _lib.NK_PC_SPECTRAL,
                 "spectral-mixed": _lib.NK_PC_SPECTRAL_MIXED}
        if isinstance(kind, str) or kind is None:
            if kind not in names:
                raise ValueError(f"inner_M={kind!r}: None, 'spectral' or 'spectral-mixed'")
            code = names[kind]
        else:
            code = int(kind)
        check(lib.nk_sh_set_precond(self._h, code), "nk_sh_set_precond")
        self.inner_M = {_lib.NK_PC_SPECTRAL: "spectral",
                        _lib.NK_PC_SPECTRAL_MIXED: "spectral-mixed"}.get(code)

    # ----------------------------------------------------------------------------- stepping
    def _as_grid(self, U):
        U = torch.as_tensor(U)
        if U.device.type != "cuda" or U.dtype != torch.float64:
            U = U.to(device="cuda", dtype=torch.float64)
        return U.contiguous()

    def step(self, U, out=None):
        """One implicit Crank-Nicolson step U[s] -> U[s+1] (sh_scipy_nk.py:56-61).

        ``out`` (optional) must be a contiguous float64 CUDA tensor with as many values as the
        slab; it may alias ``U``.  The library runs on the stepper's stream: when that is not
        torch's current stream, it first waits for the work torch has queued (U, out), and torch's
        stream waits for the step before anything reads ``out``."""
        U = self._as_grid(U)
        if U.numel() != self.ny_local * self.nx:
            raise ValueError(f"state has {U.numel()} values, slab is {self.ny_local}x{self.nx}")
        if out is None:
            out = torch.empty_like(U)
        elif (not isinstance(out, torch.Tensor) or out.device.type != "cuda"
              or out.device != U.device or out.dtype != torch.float64
              or out.numel() != U.numel() or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float64 CUDA tensor on the state's device "
                             f"with {U.numel()} values")
        cur = torch.cuda.current_stream(U.device)
        mine = self._stream if self._stream is not None else cur
        if mine != cur:
            mine.wait_stream(cur)
        st = _lib.nk_stats()
        rc = lib.nk_sh_step(self._h, C.c_void_p(U.data_ptr()), C.c_void_p(out.data_ptr()),
                            C.byref(st))
        if mine != cur:
            cur.wait_stream(mine)
        self.last_stats = st.as_dict()
        self.last_stats["n_precond"] = int(lib.nk_sh_precond_applies(self._h))
        if rc == _lib.NK_NO_CONVERGENCE:
            raise NoConvergence(out)
        raise_for_status(rc)
        return out

    def run(self, U, nsteps: int):
        """``nsteps`` implicit steps (the loop of sh_scipy_nk.py:53-61 without plotting)."""
        U = self._as_grid(U)
        a, b = U.clone(), torch.empty_like(U)
        for _ in range(int(nsteps)):
            self.step(a, out=b)
            a, b = b, a
        return a

    # ----------------------------------------------------------------------------- small grids
    #: the cap of ``run_batch`` in grid points (host only; 96 x 96)
    resident_max_points = int(lib.nk_shlin_resident_max_points())

    #: the cap of ``run_batch(..., precond="spectral")`` in grid points (host only; 128 x 64)
    resident_precond_max_points = int(lib.nk_shlin_resident_precond_max_points())

    #: the cap of ``run_batch(..., precond="spectral-mixed")`` in grid points (host only; 96 x 96)
    resident_precond_mixed_max_points = int(lib.nk_shlin_resident_precond_mixed_max_points())

    def run_batch(self, U, nsteps=1, r=None, g=None, precond=None, inner_maxiter=1000):
        """``nsteps`` implicit steps of B independent states in one launch, one workgroup per state
        with whole steps on chip (csrc/sh_resident.hip): for small grids, where ``step`` is bound
        by launch and read-back latency, and for ensembles and sweeps in ``r`` and ``g`` of them.

        The method is Newton-CG with the analytic Jacobian, not ``step``'s LGMRES on a difference
        quotient: k J = I + k (1.5 u^2 - g u) - L k/2 is symmetric positive definite whenever
        k (g^2/6 + r/2) < 1, so each Newton correction is a conjugate-gradient solve.  The outer
        loop is ``step``'s (the stop on max|F| <= ``f_tol``, the forcing terms, the Armijo search or
        ``line_search=None``, Newton's ``maxiter``: the stepper's options).  It reaches the same
        root to ``f_tol``'s scale; its iteration counts are not SciPy's.  An inner solve ends at
        its tolerance or after ``inner_maxiter`` iterations; reaching the cap is no failure.

        ``U``: (B, ny*N), or one state (B = 1).  ``r``, ``g``: B values each for a per-member
        sweep, or None for the stepper's own.  Returns ``U_new`` as (B, ny*N) and fills
        ``last_batch`` (CPU tensors ``steps``, ``nit``, ``iters``, ``fnorm``, ``status``, and
        ``precond`` / ``shift``: applications of M over the run and sigma of the last solve,
        zeros on the plain path) and ``last_batch_state`` (``U_new``).

        ``precond``: ``None`` / ``"none"`` is plain CG, for sides >= 5 and ny*N <=
        ``resident_max_points``.  ``"spectral"`` preconditions CG with
        M = ((1 + sigma) I - L k/2)^-1, sigma = max(mean k (1.5 u^2 - g u), 0), applied inside the
        workgroup: the iteration count no longer grows as the mesh is refined.  It needs N and ny
        powers of two in [8, 128], ny*N <= ``resident_precond_max_points`` and k r < 2.
        ``"spectral-mixed"`` is the same solve (M, sigma, forcing, line search, guards, counters)
        with wave-local mixed-radix transforms (csrc/sh_resident_pcm.hip), for N and ny even, of
        the form 2^a 3^b 5^c, in [6, 128] and not both powers of two, ny*N <=
        ``resident_precond_mixed_max_points`` and k r < 2 (96 x 96, 128 x 72 and 72 x 128 fit; a
        grid whose plane, spectrum and tables exceed a workgroup's LDS raises).  A grid whose sides
        are both powers of two raises under this name: ``"spectral"`` serves it.
        ``set_precond`` / ``inner_M`` and ``jvp`` have no effect here.  Anything else (another
        grid, a stepper with ``f_rtol``, ``x_tol`` or ``x_rtol`` set, with a communicator or a slab
        of a larger grid) raises ``ValueError`` and leaves the stepper usable.

        A member's bits depend on its own inputs alone.  A member with k (g^2/6 + r/2) >= 1 (or,
        under either preconditioner, k r >= 2) is refused as a non-finite one is; a member that fails a
        step stops with the last state it completed a step to.  ``NoConvergence`` (carrying
        ``U_new``) or the non-finite error is raised after ``last_batch`` and ``last_batch_state``
        are filled, the other members' results among them."""
        if precond not in (None, "none", "spectral", "spectral-mixed"):
            raise ValueError(f"precond={precond!r}: None, 'none', 'spectral' or 'spectral-mixed'")
        if self.comm is not None or self.ny_local != self.ny:
            raise ValueError("run_batch serves one GPU: no communicator, ny_local == ny")
        o = self.opts
        if not (math.isnan(o.f_rtol) and math.isnan(o.x_tol) and math.isnan(o.x_rtol)):
            raise ValueError("run_batch stops on f_tol alone: f_rtol, x_tol and x_rtol must be unset")
        ny, nx, n = self.ny, self.nx, self.ny * self.nx
        if precond == "spectral":
            side = lambda v: 8 <= v <= 128 and v & (v - 1) == 0  # noqa: E731
            if not (side(ny) and side(nx) and n <= self.resident_precond_max_points):
                raise ValueError(f"precond='spectral': N and ny powers of two in [8, 128] with ny*N "
                                 f"<= {self.resident_precond_max_points}, got {ny} x {nx}")
            if not self.k * self.r < 2:
                raise ValueError("precond='spectral' needs k r < 2")
        elif precond == "spectral-mixed":
            def side(v):
                if v < 6 or v > 128 or v % 2:
                    return False
                for f in (2, 3, 5):
                    while v % f == 0:
                        v //= f
                return v == 1
            pow2 = lambda v: v & (v - 1) == 0  # noqa: E731
            if not (side(ny) and side(nx) and n <= self.resident_precond_mixed_max_points):
                raise ValueError(f"precond='spectral-mixed': N and ny even, 2^a 3^b 5^c, in "
                                 f"[6, 128] with ny*N <= {self.resident_precond_mixed_max_points}, "
                                 f"got {ny} x {nx}")
            if pow2(ny) and pow2(nx):
                raise ValueError(f"precond='spectral-mixed': {ny} x {nx} has two power-of-two "
                                 f"sides; precond='spectral' serves it")
            if not self.k * self.r < 2:
                raise ValueError("precond='spectral-mixed' needs k r < 2")
        elif min(ny, nx) < 5 or n > self.resident_max_points:
            raise ValueError(f"run_batch: sides >= 5 and ny*N <= {self.resident_max_points}, "
                             f"got {ny} x {nx}")
        if not self.k > 0 or int(nsteps) < 1 or int(inner_maxiter) < 1:
            raise ValueError("run_batch needs k > 0, nsteps >= 1 and inner_maxiter >= 1")
        U = torch.as_tensor(U).to(device="cuda", dtype=torch.float64).contiguous()
        if U.numel() == 0 or U.numel() % n or (U.dim() > 1 and U.shape[0] * n != U.numel()):
            raise ValueError(f"expected (B, {n}) values with B >= 1, got {tuple(U.shape)}")
        U = U.reshape(-1, n)
        B = U.shape[0]

        def member(v, name):
            if v is None:
                return None
            v = torch.as_tensor(v).to(device="cuda", dtype=torch.float64).contiguous().reshape(-1)
            if v.numel() != B:
                raise ValueError(f"{name}: expected {B} values, got {v.numel()}")
            return v

        r, g = member(r, "r"), member(g, "g")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        new = torch.empty_like(U)
        i64 = lambda: torch.zeros(B, dtype=torch.int64)  # noqa: E731
        res = {"steps": i64(), "nit": i64(), "iters": i64(),
               "fnorm": torch.zeros(B, dtype=torch.float64),
               "status": torch.zeros(B, dtype=torch.int32), "precond": i64(),
               "shift": torch.zeros(B, dtype=torch.float64)}
        cur = torch.cuda.current_stream(U.device)
        mine = self._stream if self._stream is not None else cur
        if mine != cur:
            mine.wait_stream(cur)
        kind = {"spectral": _lib.NK_PC_SPECTRAL,
                "spectral-mixed": _lib.NK_PC_SPECTRAL_MIXED}.get(precond, _lib.NK_PC_NONE)
        rc = lib.nk_sh_run_batch(self._h, ptr(U), ptr(new), B, int(nsteps), ptr(r), ptr(g), kind,
                                 int(inner_maxiter), ptr(res["nit"]), ptr(res["iters"]),
                                 ptr(res["steps"]), ptr(res["fnorm"]), ptr(res["status"]),
                                 ptr(res["precond"]), ptr(res["shift"]))
        if rc == _lib.NK_EINVAL and precond == "spectral-mixed":  # the one refusal left to the host
            raise ValueError(f"precond='spectral-mixed': the plane, spectrum and tables of "
                             f"{ny} x {nx} exceed a workgroup's LDS")
        check(min(rc, 0), "nk_sh_run_batch")
        self.last_batch, self.last_batch_state = res, new
        raise_for_status(rc, new)
        return new

    def step_batch(self, U, r=None, g=None, precond=None, inner_maxiter=1000):
        """One step of every member: ``run_batch(U, 1, r, g, precond, inner_maxiter)``."""
        return self.run_batch(U, 1, r, g, precond, inner_maxiter)

    # ----------------------------------------------------------------------------- operators
    def L(self, v):
        from .ops import sh13_apply
        return sh13_apply(self._as_grid(v), self.h, self.r, self.ny, self.nx)

    def Lap(self, v):
        from .ops import lap5_apply
        return lap5_apply(self._as_grid(v), self.e, self.ny, self.nx)

    def residual(self, u, Uo):
        """``residual(u)`` with the module global ``Uo`` made explicit (sh_scipy_nk.py:47-49)."""
        from .ops import sh_residual
        return sh_residual(self._as_grid(u), self._as_grid(Uo), self.h, self.r, self.k, self.g,
                           self.ny, self.nx)

    # ----------------------------------------------------------------------------- profiling
    def kernel_profile(self):
        recs = (_lib.nk_kprof * 32)()
        n = check(lib.nk_sh_kernel_profile(self._h, recs, 32), "nk_sh_kernel_profile")
        return {recs[i].name.decode(): {"launches": recs[i].launches, "ms": recs[i].total_ms,
                                        "alg_bytes": recs[i].alg_bytes, "timed": recs[i].timed,
                                        "timed_bytes": recs[i].timed_bytes} for i in range(n)}

    def reset_profile(self):
        check(lib.nk_sh_reset_profile(self._h), "nk_sh_reset_profile")

    def workspace_bytes(self) -> int:
        return int(lib.nk_sh_workspace_bytes(self._h))

    def step_log(self):
        """The accepted Armijo step of every Newton iteration of the last step (the ``step %g``
        column of the reference's verbose output, sh_scipy_nk.py:61)."""
        n = check(lib.nk_sh_step_log(self._h, None, 0), "nk_sh_step_log")
        buf = (C.c_double * max(n, 1))()
        check(lib.nk_sh_step_log(self._h, buf, n), "nk_sh_step_log")
        return [buf[i] for i in range(n)]


def sh_step(U, h, k=0.2, r=0.01, g=1.0, **kw):
    """Functional form: the next implicit step of a 2-D periodic grid with mesh spacing h."""
    U = torch.as_tensor(U)
    ny, nx = U.shape
    model = SwiftHohenberg(N=nx, d=h * nx, k=k, r=r, g=g, ny=ny, **kw)
    try:
        return model.step(U)
    finally:
        model.close()
