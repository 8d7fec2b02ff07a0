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
        leaves the stepper as it was."""
        names = {None: _lib.NK_PC_NONE, "none": _lib.NK_PC_NONE, "spectral": _lib.NK_PC_SPECTRAL}
        if isinstance(kind, str) or kind is None:
            if kind not in names:
                raise ValueError(f"precond={kind!r}: None or 'spectral'")
            code = names[kind]
        else:
            code = int(kind)
        check(lib.nk_shlin_set_precond(self._h, code), "nk_shlin_set_precond")
        self.precond = "spectral" if code == _lib.NK_PC_SPECTRAL else None

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

    def run(self, U0, nsteps):
        """main()'s loop from Uo = U = U0 (:25-26, :46-56); returns [U[1], ..., U[nsteps]]."""
        U = self._dev(U0)
        Uo, out = U, []
        for _ in range(int(nsteps)):
            U, Uo = self.step(U, Uo), U
            out.append(U)
        return out
