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
  // NK_PC_SPECTRAL_MIXED takes even sides 2^a 3^b 5^c in [6, 4096] as well (fftpc_check_mixed).
  // The first of either builds the plan and allocates two vectors (z and the half spectrum);
  // no step allocates.
  int set_precond(int kind);
  // `nsteps` steps of `batch` independent states (contiguous rows of ny nx doubles) in one launch
  // of shlin_resident.hip: one workgroup per state runs what step() runs, on chip.  Plain CG,
  // whatever set_precond says (run_batch_pc below takes the preconditioner as an argument).
  // r, g: per-member device arrays, or null for the stepper's values.
  // A member that ends a step with a status other than NK_OK stops there with its last accepted
  // (U, Uo) in (Unew, Uprev); the others go on.  Host results per member (any may be null): CG
  // iterations over the run, steps completed, the last solve's relative residual, status.
  // Returns the worst member status; NK_EINVAL, with nothing launched, for a grid outside
  // shlin_resident_fits, batch < 1 or nsteps < 1.  Synchronises.
  int run_batch(const double* U, const double* Uo, double* Unew, double* Uprev, int64_t batch,
                int64_t nsteps, const double* r, const double* g, int64_t* iters,
                int64_t* steps_done, double* relres, int32_t* status);
  // run_batch with the preconditioner named by the call.  NK_PC_NONE: run_batch, exactly (applies
  // and shift are zeros).  NK_PC_SPECTRAL: preconditioned CG with M applied on chip
  // (shlin_resident_pc.hip), for ny, nx powers of two in [8, 128] with ny nx <=
  // kShLinResidentPcMaxPoints and k r < 2.  A member whose own k r_m >= 2 ends with NK_NONFINITE
  // before its first step.  applies, shift (host, may be null): applications of M over the run and
  // sigma of the last solve, per member.  NK_PC_SPECTRAL_MIXED: the same solve with wave-local
  // mixed-radix transforms (shlin_resident_pcm.hip), for even sides 2^a 3^b 5^c in [6, 128], at
  // least one of them no power of two (a grid of two powers of two belongs to NK_PC_SPECTRAL and is
  // refused under this kind), ny nx <= kShLinResidentPcMixedMaxPoints and an LDS footprint that
  // fits (shlin_resident_pcm_fits).  Any other kind or grid: NK_EINVAL, nothing launched or
  // allocated.  The first call of a kind allocates its table (nx + ny doubles; mixed:
  // shlin_resident_pcm_table_doubles).
  int run_batch_pc(const double* U, const double* Uo, double* Unew, double* Uprev, int64_t batch,
                   int64_t nsteps, const double* r, const double* g, int kind, int64_t* iters,
                   int64_t* steps_done, double* relres, int32_t* status, int64_t* applies,
                   double* shift);
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
  // run_batch's per-member results: device entries and their pinned host copy, grown on demand
  ShLinResidentOut* bout_ = nullptr;
  ShLinResidentOut* bout_h_ = nullptr;
  int64_t bout_cap_ = 0;
  // run_batch_pc's: the second per-member record, and the twiddle table of the resident kernel
  ShLinResidentPcOut* bpc_ = nullptr;
  ShLinResidentPcOut* bpc_h_ = nullptr;
  int64_t bpc_cap_ = 0;
  double* rtab_ = nullptr;
  double* rtab_mixed_ = nullptr;  // the mixed kernel's: all roots and the permutations
  int grow_batch_out(int64_t batch);
  void resident_args(ShLinResidentArgs* A, const double* U, const double* Uo, double* Unew,
                     double* Uprev, int64_t nsteps, const double* r, const double* g) const;
  int collect_batch(int64_t batch, int64_t* iters, int64_t* steps_done, double* relres,
                    int32_t* status) const;
  int status_ = NK_OK;
};

}  // namespace nk
