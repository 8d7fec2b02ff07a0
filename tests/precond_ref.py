"""TEST INFRASTRUCTURE ONLY -- NumPy restatements of the spectral preconditioner of the SH step.

M = A0^-1 with A0 = I/k - L/2 on a periodic ny x nx grid (L the 13-point operator), which is
diagonal in Fourier space: A0^(p,q) = 1/k - L^/2, L^ = -s^2 - 2 s + (r-1),
s = (2 cos(2 pi p/ny) + 2 cos(2 pi q/nx) - 4)/h^2.

* ``precond_ld``  the reference: dense DFT matrices and the symbol in ``np.longdouble`` (lengths up
                  to 256; the x87 80-bit format, eps 1.1e-19), rounded to float64 once at the end;
* ``precond_np``  NumPy's double-precision FFT realisation, the yardstick a double-precision
                  kernel is held against (tests/test_gpu_precond.py).

Also the records of SciPy's own newton_krylov with this M (tests/test_precond_ref.py checks them
on the CPU, tests/test_gpu_precond.py compares the GPU solver's counts with them).
"""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI_LD = LD(4) * np.arctan(LD(1))

# scipy.optimize.newton_krylov(residual, U0, inner_M=M) from the start states of start_state():
# Newton iterations and calls of F (test_precond_ref.py::test_scipy_converges_with_M)
SCIPY_WITH_M = {
    (64, 64): {"nit": 5, "nfev": 41},
    (128, 64): {"nit": 5, "nfev": 42},
}


def _cos_ld(n):
    """cos(2 pi j / n), j < n, in longdouble (exact argument reduction: j stays an integer)."""
    j = np.arange(n)
    return np.cos(2 * PI_LD * j.astype(LD) / LD(n))


@functools.lru_cache(maxsize=None)
def dft_ld(n):
    """W[j, k] = exp(-2 pi i j k / n) in longdouble, the angle reduced mod n in integers."""
    m = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    a = 2 * PI_LD * m.astype(LD) / LD(n)
    return (np.cos(a) - 1j * np.sin(a)).astype(CLD)


def symbol(ny, nx, h, r, k, dtype=LD):
    """A0^(p, q), shape (ny, nx)."""
    cy = _cos_ld(ny).astype(dtype)[:, None]
    cx = _cos_ld(nx).astype(dtype)[None, :]
    s = (2 * cy + 2 * cx - 4) / (dtype(h) * dtype(h))
    lh = -s * s - 2 * s + (dtype(r) - 1)
    return 1 / dtype(k) - lh / 2


def lam_min(ny, nx, h, r, k):
    """Smallest eigenvalue of A0 on the grid (>= 1/k - r/2)."""
    return float(symbol(ny, nx, h, r, k).min())


def precond_ld(v, h, r, k, keep=False):
    """M v by dense longdouble DFTs; float64 result (keep=True: the longdouble one)."""
    v = np.asarray(v)
    ny, nx = v.shape
    assert max(ny, nx) <= 256, "dense DFT reference: lengths up to 256"
    Wy, Wx = dft_ld(ny), dft_ld(nx)
    V = Wy @ v.astype(CLD) @ Wx
    V = V / symbol(ny, nx, h, r, k)
    z = (np.conj(Wy) @ V @ np.conj(Wx)).real / LD(nx * ny)
    return z if keep else z.astype(np.float64)


def precond_np(v, h, r, k):
    """M v by numpy.fft in double precision."""
    v = np.asarray(v, dtype=np.float64)
    ny, nx = v.shape
    A = symbol(ny, nx, h, r, k).astype(np.float64)
    return np.fft.irfft2(np.fft.rfft2(v) / A[:, :nx // 2 + 1], s=(ny, nx))


def start_state(golden_traj0, ny, nx):
    """The 64 x 64 fixture state (tests/golden/nk_n64_default.npz), tiled in y for 128 x 64."""
    U = np.asarray(golden_traj0, dtype=np.float64).reshape(64, 64)
    assert nx == 64 and ny % 64 == 0
    return np.tile(U, (ny // 64, 1))


def rel_err(a, ref):
    """max-norm of the error over max-norm of the reference."""
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(a, dtype=ref.dtype) - ref).max() / np.abs(ref).max())


def inputs(ny, nx, seed=0):
    """The operator tests' fields: random, one-hot in each corner and at the centre, a pure
    Nyquist mode along each axis, a constant."""
    rng = np.random.default_rng(seed + 1000 * ny + nx)
    out = {"random": rng.standard_normal((ny, nx))}
    for name, (i, j) in {"hot00": (0, 0), "hot0x": (0, nx - 1), "hoty0": (ny - 1, 0),
                         "hotyx": (ny - 1, nx - 1), "hotc": (ny // 2, nx // 2)}.items():
        e = np.zeros((ny, nx))
        e[i, j] = 1.0
        out[name] = e
    out["nyq_x"] = np.tile((-1.0) ** np.arange(nx), (ny, 1))
    out["nyq_y"] = np.tile(((-1.0) ** np.arange(ny))[:, None], (1, nx))
    out["const"] = np.full((ny, nx), 0.75)
    return out
