// Semi-implicit Swift-Hohenberg stepper of python_work/sh_linearised.py (see shlin.cpp).
#pragma once

#include <vector>

#include "fftpc.h"
#include "nk_solver.h"

namespace nk {

struct ShLinStats {
  int64_t iters = 0;     // CG iterations of the last step
  double relres = 0.0;   // |b - A x| / |b| at exit
  int64_t precond_applies = 0;  // applications of M launched in the last step (0 without M)
  double shift = 0.0;           // sigma of the last step (0 without M)
};

// U[s+1] = solve(I + D - L k/2, (I + L k/2) U[s]), D = diag((5U[s] - U[s-1])^2 k/16 - g k U[s])
// (sh_linearised.py:48-56).  The reference factorises the sparse matrix (spsolve); here the
// matrix is never formed: it is symmetric positive definite whenever 1 + min(D) > k r/2
// (always for g = 0), so a matrix-free conjugate-gradient solve on the 13-point stencil replaces
// the direct solve, warm-started from U[s] and run to a relative residual of rtol.
//
// set_precond(NK_PC_SPECTRAL): preconditioned CG with the constant-coefficient part of the matrix,
//   M = ((1 + sigma) I - L k/2)^-1,  sigma = max(mean(D), 0)
// (the clamp keeps the symbol positive where g != 0 makes the mean negative), applied in Fourier
// space by fftpc.hip: M v = (1/k) (I (1 + sigma)/k - L/2)^-1 v, the Newton-Krylov preconditioner's
// passes with ik = (1 + sigma)/k per application.  The stopping rule stays the recursive
// unpreconditioned residual.  Per iteration: q = A p, p.q (LINOP, which also forms p = z + beta p);
// the x/r update with r.r; z = M r with r.z from the last FFT pass -- two scalar read-backs, the
// second one of r.r and r.z together (the application is queued behind the update before r.r is
// known, so the last iteration launches one application that is not used).
class ShLinStepper {
 public:
  ShLinStepper(int64_t ny, int64_t nx, double h, double r, double g, double k, double rtol,
               int64_t maxiter, hipStream_t s, bool profile);
  int status() const { return status_; }
  int step(const double* U, const double* Uo, double* Unew, ShLinStats* st);
  // NK_PC_NONE: the unpreconditioned stepper, exactly.  NK_PC_SPECTRAL needs nx, ny powers of two
  // in [8, 16384] and k r < 2 (fftpc_check); NK_EINVAL otherwise, and the stepper stays as it was.
  // The first NK_PC_SPECTRAL builds the plan and allocates two vectors (z and the half spectrum);
  // no step allocates.
  int set_precond(int kind);
  const ShLinStats& last() const { return last_; }
  ~ShLinStepper();
  Engine E;

 private:
  int linop(const double* a, const double* b, double beta, const double* d, double theta,
            double* w, double* out, int64_t* nblk);
  // z = M r and the block partials of r . z (*nblk of them)
  int precond(const double* r, double* z, double sigma, int64_t* nblk);
  int64_t ny_, nx_;
  double h_, r_;
  double g_, k_, rtol_;
  int64_t maxiter_;
  SHCoef c_{};
  std::vector<double*> v_;
  FftPcPlan pc_{};       // spectral preconditioner (tables != nullptr once built)
  double* z_ = nullptr;  // M r
  bool pc_on_ = false;
  ShLinStats last_{};
  int status_ = NK_OK;
};

}  // namespace nk
