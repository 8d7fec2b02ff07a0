"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the preconditioned CG solve of the
semi-implicit Swift-Hohenberg stepper (csrc/shlin.cpp with set_precond(NK_PC_SPECTRAL)).

The step solves A x = b, A = I + D - (k/2) L, b = (I + (k/2) L) U, D = (5U - Uo)^2 k/16 - g k U
(oracle/shlin_oracle.py).  The preconditioner is the constant-coefficient part of A with D replaced
by its clamped mean,

    sigma = max(mean(D), 0),   M_sigma = ((1 + sigma) I - (k/2) L)^-1,

diagonal in Fourier space with symbol (1 + sigma) - (k/2) L^ = k [ (1 + sigma)/k - L^/2 ]: the
Newton-Krylov preconditioner of precond_ref.py at k' = k/(1 + sigma), divided by k.

* ``shift_ld``  the longdouble reference for M_sigma (dense DFTs, lengths up to 256);
* ``shift_np``  NumPy's double-precision FFT realisation, the yardstick of the GPU kernel;
* ``pcg``       the solve as the stepper runs it: warm start x = U, stop on the recursive
                unpreconditioned residual sqrt(r.r) <= rtol |b|;
* ``CASES`` / ``RECORDS``  the test states and the iteration counts of ``pcg`` on them
                (tests/test_shlin_pcg_ref.py checks the records on the CPU,
                tests/test_gpu_shlin_precond.py compares the GPU stepper's counts with them).
"""
import numpy as np

import precond_ref as pr
from oracle.sh_oracle import sh13

LD = pr.LD
K, R = 0.2, 0.2
RTOL = 1e-14

# name: (ny, nx, h, g, seed)
CASES = {
    "stiff64": (64, 64, 0.0625, 0.0, 11),
    "stiff128x64": (128, 64, 0.0625, 0.0, 12),
    "negD64": (64, 64, 0.625, 1.0, 13),
    "small8": (8, 8, 0.625, 0.0, 14),
    "small16x8": (16, 8, 0.0625, 0.0, 15),
}
# PCG iterations of pcg() to RTOL; "golden": the six steps of tests/golden/shlin_steps.npz
RECORDS = {
    "golden": [16, 17, 15, 13, 12, 12],
    "stiff64": 5,
    "stiff128x64": 5,
    "negD64": 8,
    "small8": 10,
    "small16x8": 4,
}
# unpreconditioned CG on the same systems, for orientation (not asserted on the GPU beyond
# "under a quarter" on the golden steps and NoConvergence at maxiter = 1000 on stiff64)
CG_RECORDS = {"golden": [92, 90, 90, 90, 90, 90], "stiff64": 2321, "stiff128x64": 4243,
              "negD64": 97, "small8": 56, "small16x8": 106}


def state(name):
    """(U, Uo, ny, nx, h, g) of a case, flat float64 vectors."""
    ny, nx, h, g, seed = CASES[name]
    rng = np.random.default_rng(seed)
    n = ny * nx
    if name == "negD64":
        U = 0.5 + 0.05 * rng.standard_normal(n)
        Uo = U + 0.01 * rng.standard_normal(n)
    else:
        U = 0.5 * rng.standard_normal(n)
        Uo = 0.5 * rng.standard_normal(n)
    return U, Uo, ny, nx, h, g


def diag(U, Uo, k, g, dtype=np.float64):
    U, Uo = np.asarray(U, dtype=dtype), np.asarray(Uo, dtype=dtype)
    a = 5 * U - Uo
    return a * a * dtype(k) / 16 - dtype(g) * dtype(k) * U


def shift(U, Uo, k, g, dtype=np.float64):
    """sigma = max(mean(D), 0)."""
    m = diag(U, Uo, k, g, dtype).sum() / dtype(np.asarray(U).size)
    return max(m, dtype(0))


def shift_ld(v, h, r, k, sigma, keep=False):
    """M_sigma v by dense longdouble DFTs (v of shape (ny, nx))."""
    z = pr.precond_ld(v, h, r, LD(k) / (1 + LD(sigma)), keep=True) / LD(k)
    return z if keep else z.astype(np.float64)


def shift_np(v, h, r, k, sigma):
    """M_sigma v by numpy.fft in double precision."""
    v = np.asarray(v, dtype=np.float64)
    ny, nx = v.shape
    A = ((1 + LD(sigma)) - LD(k) / 2 * lhat(ny, nx, h, r)).astype(np.float64)
    return np.fft.irfft2(np.fft.rfft2(v) / A[:, :nx // 2 + 1], s=(ny, nx))


def lhat(ny, nx, h, r):
    """L^(p, q) in longdouble, shape (ny, nx)."""
    cy = pr._cos_ld(ny)[:, None]
    cx = pr._cos_ld(nx)[None, :]
    s = (2 * cy + 2 * cx - 4) / (LD(h) * LD(h))
    return -s * s - 2 * s + (LD(r) - 1)


def system(U, Uo, ny, nx, h, r, k, g):
    """(A as a function, b, D) of one step."""
    D = diag(U, Uo, k, g)
    b = U + k / 2 * sh13(U, ny, nx, h, r)

    def A(x):
        return x + D * x - k / 2 * sh13(x, ny, nx, h, r)

    return A, b, D


def pcg(U, Uo, ny, nx, h, r=R, k=K, g=0.0, rtol=RTOL, maxiter=1000, precond=True):
    """One step's solve.  Returns (x, iterations, sigma, relres, applications of M);
    precond=False: plain CG (the stepper as it is without the option)."""
    A, b, D = system(U, Uo, ny, nx, h, r, k, g)
    sigma = max(float(D.mean()), 0.0) if precond else 0.0

    def M(v):
        if not precond:
            return v
        return shift_np(v.reshape(ny, nx), h, r, k, sigma).reshape(-1)

    bnorm = np.sqrt(b @ b)
    stop = rtol * bnorm
    x = U.copy()
    res = b - A(x)
    napp = 0
    z = M(res)
    napp += 1
    rho = res @ z
    p = z.copy()
    rr = res @ res
    it = 0
    while np.sqrt(rr) > stop and it < maxiter:
        q = A(p)
        pq = p @ q
        if not (pq > 0.0 and rho > 0.0):
            raise FloatingPointError("indefinite system or preconditioner")
        alpha = rho / pq
        x += alpha * p
        res -= alpha * q
        rr = res @ res
        it += 1
        if np.sqrt(rr) <= stop:
            break
        z = M(res)
        napp += 1
        rho_new = res @ z
        p = z + (rho_new / rho) * p
        rho = rho_new
    return x, it, sigma, float(np.sqrt(rr) / bnorm) if bnorm > 0 else 0.0, napp if precond else 0
