"""Semi-implicit Swift-Hohenberg stepper: python_work/sh_linearised.py over libnkhip.

The reference's ``main()`` (:14-65) advances U with one sparse direct solve per step,

    D = diags((5U - Uo)^2 k/16 - g k U);  Uo = U
    U = spsolve(I + D - L k/2, (I + L k/2) Uo)                                      (:48-56)

starting from ``Uo = U`` (:25-26).  ``SHLinearised.step`` performs the same step on the GPU with a
matrix-free conjugate-gradient solve over the 13-point stencil kernel (the system is symmetric
positive definite for g = 0, the reference's value), warm-started from U and run to a relative
residual of ``rtol``.

``precond="spectral"`` turns the solve into preconditioned CG with the constant-coefficient part of
the matrix, M = ((1 + sigma) I - L k/2)^-1 with sigma = max(mean(D), 0), applied in Fourier space
by hand-written FFT passes (``ops.shlin_precond``).  Off by default; off, the stepper is exactly
the unpreconditioned one.

``run_batch`` / ``step_batch`` serve small grids (ny*N <= ``resident_max_points``) and ensembles of
them: one workgroup per state runs whole steps on chip, in one launch for the batch.  Their own
``precond="spectral"`` applies the same preconditioner inside the resident workgroup (N and ny
powers of two in [8, 128], ny*N <= ``resident_precond_max_points``), ``precond="spectral-mixed"``
on even sides 2^a 3^b 5^c in [6, 128] that are not both powers of two (ny*N <=
``resident_precond_mixed_max_points``).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import NK_NO_CONVERGENCE, check, lib
from .solver import NoConvergence, raise_for_status


class SHLinearised:
    def __init__(self, N=64, d=40.0, k=0.2, r=0.2, g=0.0, *, ny=None, rtol=1e-14, maxiter=1000,
                 stream=None, precond=None):
        self.N = int(N)
        self.ny = int(ny) if ny is not None else self.N
        self.h = float(d) / self.N  # h = d/N (:18)
        self.k, self.r, self.g = float(k), float(r), float(g)
        self._stream = stream
        self._h = C.c_void_p()
        st = stream if stream is not None else torch.cuda.current_stream()
        check(lib.nk_shlin_create(C.byref(self._h), self.ny, self.N, self.h, self.r, self.g,
                                  self.k, float(rtol), int(maxiter), C.c_void_p(st.cuda_stream)),
              "nk_shlin_create")
        self.last_iters = 0
        self.last_relres = 0.0
        self.last_precond = 0   # applications of M launched in the last step
        self.last_shift = 0.0   # sigma of the last step
        self.last_batch = None  # per-member results of the last run_batch
        self.last_batch_state = None  # its (U_new, U_prev): the survivors' states when it raised
        self.precond = None
        if precond is not None:
            try:
                self.set_precond(precond)
            except Exception:
                self.close()
                raise

    def set_precond(self, kind):
        """Preconditioner of the CG solve: ``None`` / ``"none"`` / ``NK_PC_NONE`` (the
        unpreconditioned stepper, exactly) or ``"spectral"`` / ``NK_PC_SPECTRAL``,
        M = ((1 + sigma) I - L k/2)^-1 with sigma = max(mean(D), 0) recomputed every step.
        Spectral needs N and ny powers of two in [8, 16384] and k r < 2; anything else raises and
        leaves the stepper as it was.  ``"spectral-mixed"`` / ``NK_PC_SPECTRAL_MIXED``: the same on
        sides that are both even, of the form 2^a 3^b 5^c and in [6, 4096] as well."""
        names = {None: _lib.NK_PC_NONE, "none": _lib.NK_PC_NONE, "spectral": _lib.NK_PC_SPECTRAL,
                 "spectral-mixed": _lib.NK_PC_SPECTRAL_MIXED}
        if isinstance(kind, str) or kind is None:
            if kind not in names:
                raise ValueError(f"precond={kind!r}: None, 'spectral' or 'spectral-mixed'")
            code = names[kind]
        else:
            code = int(kind)
        check(lib.nk_shlin_set_precond(self._h, code), "nk_shlin_set_precond")
        self.precond = {_lib.NK_PC_SPECTRAL: "spectral",
                        _lib.NK_PC_SPECTRAL_MIXED: "spectral-mixed"}.get(code)

    def close(self):
        if self._h:
            lib.nk_shlin_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, a):
        t = torch.as_tensor(a).to(device="cuda", dtype=torch.float64).contiguous().reshape(-1)
        if t.numel() != self.ny * self.N:
            raise ValueError(f"expected {self.ny * self.N} values, got {t.numel()}")
        return t

    def step(self, U, Uo):
        """U[s+1] from U = U[s], Uo = U[s-1] (:48-56)."""
        U, Uo = self._dev(U), self._dev(Uo)
        out = torch.empty_like(U)
        its, rel = C.c_int64(), C.c_double()
        rc = lib.nk_shlin_step(self._h, C.c_void_p(U.data_ptr()), C.c_void_p(Uo.data_ptr()),
                               C.c_void_p(out.data_ptr()), C.byref(its), C.byref(rel))
        self.last_iters, self.last_relres = its.value, rel.value
        self.last_precond = int(lib.nk_shlin_precond_applies(self._h))
        self.last_shift = float(lib.nk_shlin_precond_shift(self._h))
        if rc == NK_NO_CONVERGENCE:
            raise NoConvergence(out)
        raise_for_status(rc)
        return out

    #: the cap of ``run_batch`` in grid points (host only; at least 96 x 96)
    resident_max_points = int(lib.nk_shlin_resident_max_points())

    #: the cap of ``run_batch(..., precond="spectral")`` in grid points (host only; 128 x 64)
    resident_precond_max_points = int(lib.nk_shlin_resident_precond_max_points())

    #: the cap of ``run_batch(..., precond="spectral-mixed")`` in grid points (host only; 96 x 96)
    resident_precond_mixed_max_points = int(lib.nk_shlin_resident_precond_mixed_max_points())

    def run_batch(self, U, Uo=None, nsteps=1, r=None, g=None, precond=None):
        """``nsteps`` steps of B independent states in one launch, one workgroup per state with
        the whole CG solve on chip (csrc/shlin_resident.hip).  ``U``: (B, ny*N), or one state
        (B = 1); ``Uo=None`` is the reference's start Uo = U (:25-26).  ``r``, ``g``: B values each
        for a per-member sweep, or None for the stepper's own.  Returns ``(U_new, U_prev)`` as
        (B, ny*N) tensors and fills ``last_batch`` (CPU tensors ``iters``, ``steps``, ``relres``,
        ``status``, and ``precond`` / ``shift``: applications of M over the run and sigma of the
        last solve, zeros on the plain path).  Needs ny*N <= ``resident_max_points``; one GPU.

        ``precond``: ``None`` / ``"none"`` is plain CG, and ``set_precond`` has no effect here:
        only this argument selects the solve.  ``"spectral"`` runs the preconditioned CG of
        ``step`` under ``precond="spectral"`` with the FFT preconditioner applied inside the
        resident workgroup (csrc/shlin_resident_pc.hip): the iteration count no longer grows as the
        mesh is refined.  It needs N and ny powers of two in [8, 128], ny*N <=
        ``resident_precond_max_points`` and k r < 2 (anything else raises and leaves the stepper
        usable); a member whose own k r >= 2 stops as a non-finite one does.
        ``"spectral-mixed"`` is the same solve (M, sigma, stopping rule, guards, counters) with
        wave-local mixed-radix transforms (csrc/shlin_resident_pcm.hip), for N and ny even, of the
        form 2^a 3^b 5^c, in [6, 128] and not both powers of two, ny*N <=
        ``resident_precond_mixed_max_points`` (96 x 96, 128 x 72 and 72 x 128 fit; a grid whose
        plane, spectrum and tables exceed a workgroup's LDS raises).  A grid whose sides are both
        powers of two raises under this name: ``"spectral"`` serves it.

        A member's bits depend on its own inputs alone.  A member that fails a step stops with its
        last accepted pair; ``NoConvergence`` (carrying ``U_new``) or the non-finite error is
        raised after ``last_batch`` is filled; ``last_batch_state`` then holds ``(U_new, U_prev)``,
        the other members' results among them."""
        if precond not in (None, "none", "spectral", "spectral-mixed"):
            raise ValueError(f"precond={precond!r}: None, 'none', 'spectral' or 'spectral-mixed'")
        n = self.ny * self.N
        U = torch.as_tensor(U).to(device="cuda", dtype=torch.float64).contiguous()
        if U.numel() == 0 or U.numel() % n or (U.dim() > 1 and U.shape[0] * n != U.numel()):
            raise ValueError(f"expected (B, {n}) values with B >= 1, got {tuple(U.shape)}")
        U = U.reshape(-1, n)
        B = U.shape[0]
        if Uo is None:
            Uo = U
        else:
            Uo = torch.as_tensor(Uo).to(device="cuda", dtype=torch.float64).contiguous()
            if Uo.numel() != U.numel():
                raise ValueError(f"Uo: expected {U.numel()} values, got {Uo.numel()}")

        def member(v, name):
            if v is None:
                return None
            v = torch.as_tensor(v).to(device="cuda", dtype=torch.float64).contiguous().reshape(-1)
            if v.numel() != B:
                raise ValueError(f"{name}: expected {B} values, got {v.numel()}")
            return v

        r, g = member(r, "r"), member(g, "g")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        new, prev = torch.empty_like(U), torch.empty_like(U)
        res = {"iters": torch.zeros(B, dtype=torch.int64), "steps": torch.zeros(B, dtype=torch.int64),
               "relres": torch.zeros(B, dtype=torch.float64),
               "status": torch.zeros(B, dtype=torch.int32),
               "precond": torch.zeros(B, dtype=torch.int64),
               "shift": torch.zeros(B, dtype=torch.float64)}
        if precond in ("spectral", "spectral-mixed"):
            kind = _lib.NK_PC_SPECTRAL if precond == "spectral" else _lib.NK_PC_SPECTRAL_MIXED
            rc = lib.nk_shlin_run_batch_pc(self._h, ptr(U), ptr(Uo), ptr(new), ptr(prev), B,
                                           int(nsteps), ptr(r), ptr(g), kind,
                                           ptr(res["iters"]), ptr(res["steps"]),
                                           ptr(res["relres"]), ptr(res["status"]),
                                           ptr(res["precond"]), ptr(res["shift"]))
            check(min(rc, 0), "nk_shlin_run_batch_pc")
        else:
            rc = lib.nk_shlin_run_batch(self._h, ptr(U), ptr(Uo), ptr(new), ptr(prev), B,
                                        int(nsteps), ptr(r), ptr(g), ptr(res["iters"]),
                                        ptr(res["steps"]), ptr(res["relres"]), ptr(res["status"]))
            check(min(rc, 0), "nk_shlin_run_batch")
        self.last_batch, self.last_batch_state = res, (new, prev)
        raise_for_status(rc, new)
        return new, prev

    def step_batch(self, U, Uo, r=None, g=None, precond=None):
        """One step of every member: ``run_batch(U, Uo, 1, r, g, precond)[0]``."""
        return self.run_batch(U, Uo, 1, r, g, precond)[0]

    def run(self, U0, nsteps):
        """main()'s loop from Uo = U = U0 (:25-26, :46-56); returns [U[1], ..., U[nsteps]]."""
        U = self._dev(U0)
        Uo, out = U, []
        for _ in range(int(nsteps)):
            U, Uo = self.step(U, Uo), U
            out.append(U)
        return out
