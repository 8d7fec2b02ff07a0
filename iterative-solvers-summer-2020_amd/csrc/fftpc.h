// Spectral preconditioner of the two Swift-Hohenberg solvers (fftpc.hip):
//   z = scale * IFFT2( FFT2(v) / (ik - L^/2) )  on a periodic ny x nx grid,
// the inverse of a constant-coefficient operator ik I - L/2 (L the 13-point operator of
// stencil.hip), diagonal in Fourier space:
//   s(p,q) = (2 cos(2 pi p/ny) + 2 cos(2 pi q/nx) - 4)/h^2,  L^ = -s^2 - 2 s + (r - 1).
// The Newton-Krylov step (sh_problem.cpp) uses M = A0^-1, A0 = I/k - L/2 the linear part of the
// Crank-Nicolson Jacobian: ik = 1/k, scale = 1.  The semi-implicit stepper's CG solve (shlin.cpp)
// uses ((1 + sigma) I - L k/2)^-1 with a shift sigma chosen every step: ik = (1 + sigma)/k,
// scale = 1/k, and the dot r . z from the last pass.
// No FFT library: three hand-written passes (rows real-to-complex, columns forward + symbol +
// inverse on chip, rows complex-to-real), 48 B per grid point.  Columns longer than 4096 (or than
// NKHIP_FFTPC_SPLIT, a test knob) do not fit on chip and are transformed in two factors, three
// trips over the half spectrum instead of one: 80 B per grid point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nk {

struct FftPcPlan {
  int64_t ny = 0, nx = 0;
  int ly = 0, lx2 = 0;       // log2(ny), log2(nx/2)
  double ih2 = 0.0, r = 0.0, ik = 0.0;
  double* tables = nullptr;  // twx (nx/2 complex: exp(-2 pi i j/nx)), then twy (ny/2 complex)
  double* work = nullptr;    // the packed half spectrum: ny rows of nx/2 complex = ny*nx doubles
  bool own_work = false;
  int rows = 0;              // rows per group of the row passes
  int cols = 0;              // columns per block of the column pass
  // row groups a block of the row passes takes in turn.  0: one group per block, the 256-thread
  // kernels (every grid with both sides <= 4096); otherwise the 1024-thread kernels
  int row_iters = 0;
  // split columns, ny = 2^l1 * 2^l2 (l1 = 0: whole columns on chip); 2^lw1 / 2^lw2 columns per
  // tile of the outer (length 2^l1) and inner (length 2^l2) sub-passes
  int l1 = 0, l2 = 0, lw1 = 0, lw2 = 0;
};

// NK_OK when the spectral preconditioner exists for this grid and these constants: nx, ny powers
// of two in [8, 16384], h > 0, k > 0 and k r < 2 (the symbol 1/k - L^/2 >= 1/k - r/2 + 1/2 is then
// positive); NK_EINVAL otherwise.  Host only.
int fftpc_check(int64_t ny, int64_t nx, double h, double r, double k);
// Builds the twiddle tables on the host in long double and uploads them (synchronises).  `work`:
// ny*nx doubles of device memory the plan uses as the half spectrum (nullptr: the plan allocates
// and owns it).  The environment variable NKHIP_FFTPC_SPLIT (a power of two in [16, 4096], anything
// else ignored; default 4096) is read here: the longest column kept on chip.  A longer one is
// split as min(split, 128) times the rest.
int fftpc_create(FftPcPlan* p, int64_t ny, int64_t nx, double h, double r, double k, double* work);
void fftpc_destroy(FftPcPlan* p);
// out = scale * (ik I - L/2)^-1 in, the symbol's constants given per application (three launches
// on s, five with split columns; in == out allowed).  A shifted operator
// ((1 + sigma) I - (k/2) L)^-1 is ik = (1 + sigma)/k, scale = 1/k.  The tables do not depend on ik: no plan rebuild, no
// allocation, no synchronisation.
// With w (may be `in` or `out`), the last pass also multiplies every value it stores by the
// matching entry of w and leaves one partial sum per block in partial[0, *nblk)
// (fftpc_dot_blocks(p) <= 4096 values); summed in order (reduce_final_launch) they give w . out,
// bit-reproducibly.
// hipErrorInvalidValue, and nothing launched, unless: the plan is built; in, out and w are 16-B
// aligned and none of them is the plan's work buffer; w and partial are given together or not at
// all; ik and scale are finite and ik > (r - 1)/2 (the symbol stays positive).
hipError_t fftpc_apply(const FftPcPlan& p, const double* in, double* out, double ik, double scale,
                       const double* w, double* partial, int64_t* nblk, hipStream_t s);
// out = M in: the plan's own ik = 1/k, scale = 1, no dot.
inline hipError_t fftpc_apply(const FftPcPlan& p, const double* in, double* out, hipStream_t s) {
  return fftpc_apply(p, in, out, p.ik, 1.0, nullptr, nullptr, nullptr, s);
}
// blocks of a row pass = partial sums of an application with the dot: at most 4096 (a block
// takes row_iters groups in turn where there are more groups than that)
inline int64_t fftpc_dot_blocks(const FftPcPlan& p) {
  return p.rows > 0 ? p.ny / (int64_t(p.rows) * (p.row_iters > 0 ? p.row_iters : 1)) : 0;
}
// algorithmic HBM bytes of one application of this plan (fftpc_dot_bytes: the last pass also
// reads w): each pass reads and writes one vector's worth, three passes or, with split columns, five
inline double fftpc_bytes(const FftPcPlan& p) {
  return (p.l1 ? 80.0 : 48.0) * double(p.ny) * double(p.nx);
}
inline double fftpc_dot_bytes(const FftPcPlan& p) {
  return fftpc_bytes(p) + 8.0 * double(p.ny) * double(p.nx);
}

}  // namespace nk
