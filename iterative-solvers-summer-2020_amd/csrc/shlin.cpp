// sh_linearised.py (:48-56) on the GPU: the semi-implicit step's SPD system solved by conjugate
// gradients with the operator applied matrix-free by the 13-point stencil (SMode::LINOP, which
// also forms the new search direction p = r + beta p_old on the fly and the fused p.Ap), plus a
// fused x/r update with r.r: two passes (88 B/point) and two scalar read-backs per iteration.
// With set_precond(NK_PC_SPECTRAL) (shlin.h) an application of the spectral preconditioner follows
// each update (56 B/point more), its last pass returning r.z.
#include "shlin.h"

#include <cmath>

namespace nk {

ShLinStepper::ShLinStepper(int64_t ny, int64_t nx, double h, double r, double g, double k,
                           double rtol, int64_t maxiter, hipStream_t s, bool profile)
    : E(ny * nx, nullptr, s, profile, stencil_partial_slots(ny, nx)), ny_(ny), nx_(nx), h_(h),
      r_(r), g_(g), k_(k), rtol_(rtol), maxiter_(maxiter) {
  c_ = sh_coef(h, r, k, g);
  status_ = E.alloc(8, &v_);
}

int ShLinStepper::linop(const double* a, const double* b, double beta, const double* d,
                        double theta, double* w, double* out, int64_t* nblk) {
  StencilArgs A;
  A.ny = ny_;
  A.nx = nx_;
  A.a = Field{a, nullptr, nullptr};
  A.b = Field{b, nullptr, nullptr};
  A.alpha = beta;
  A.p0 = d;
  A.out0 = out;
  A.out2 = w;
  A.c = c_;
  A.theta = theta;
  A.partial = E.partial();
  return E.launch(K_TRIAL, stencil_bytes_per_point(SMode::LINOP, false) * E.n,
                  [&] { return stencil_launch(SMode::LINOP, A, E.s, nblk); });
}

ShLinStepper::~ShLinStepper() { fftpc_destroy(&pc_); }

int ShLinStepper::set_precond(int kind) {
  if (status_) return status_;
  if (kind == NK_PC_NONE) {
    pc_on_ = false;
    return NK_OK;
  }
  if (kind != NK_PC_SPECTRAL) return NK_EINVAL;
  // a refusal allocates nothing and leaves the stepper as it was
  if (fftpc_check(ny_, nx_, h_, r_, k_)) return NK_EINVAL;
  if (!pc_.tables) {
    // the last FFT pass leaves one partial per block: at most 4096 (fftpc_dot_blocks; e.g.
    // nx = 4096, one row each -- past 4096 row groups a block takes several in turn)
    if (E.partial_cap() < 4096) return NK_EINVAL;
    if (!z_) {  // z and, behind it, the half spectrum
      std::vector<double*> w;
      const int rc = E.alloc_aux(2, &w);
      if (rc) return rc;
      z_ = w[0];
    }
    const int rc = fftpc_create(&pc_, ny_, nx_, h_, r_, k_, z_ + E.npad);
    if (rc) return rc;
  }
  pc_on_ = true;
  return NK_OK;
}

int ShLinStepper::precond(const double* r, double* z, double sigma, int64_t* nblk) {
  // ((1 + sigma) I - L k/2)^-1 = (1/k) (I (1 + sigma)/k - L/2)^-1
  return E.launch(K_PRECOND, fftpc_dot_bytes(pc_), [&] {
    return fftpc_apply(pc_, r, z, (1.0 + sigma) / k_, 1.0 / k_, r, E.partial(), nblk, E.s);
  });
}

// One CG body for both solves.  With M, z = M r stands in the place of r in the search direction
// and rho = r.z in the place of r.r in alpha and beta; the stop still tests r.r.  Without M, z is r
// and rho is r.r: the launches and read-backs are those of plain CG, and z_ is not touched.
int ShLinStepper::step(const double* U, const double* Uo, double* Unew, ShLinStats* st) {
  if (status_) return status_;
  last_ = ShLinStats{};
  const int64_t n = E.n;
  double *x = v_[0], *r = v_[1], *p = v_[2], *pn = v_[3], *q = v_[4], *d = v_[5], *zero = v_[6],
         *b = v_[7], *z = pc_on_ ? z_ : r;
  constexpr int kSlotAux = Engine::kSlotCombo;  // a result read together with the next reduce()
  int64_t nblk = 0, napp = 0;
  double red[3], sigma = 0.0, rr = 0.0, rho = 0.0;
  // rr = r.r and rho = r.z after a pass that wrote r and left nv values per block, r.r first.
  auto residual_dots = [&](int nv) {
    if (!pc_on_) {
      const int rc = E.reduce(nblk, 1, nv, red);
      if (!rc) rr = rho = red[0];
      return rc;
    }
    // M queued behind the pass before r.r is known: r.r and r.z come back together
    int rc = E.reduce_async(nblk, 1, 1, kSlotAux);
    if (!rc) rc = precond(r, z, sigma, &nblk);
    ++napp;
    if (!rc) rc = E.reduce(nblk, 1, 1, red);
    if (rc) return rc;
    rr = *E.hres(kSlotAux);
    rho = red[0];
    return rc;
  };
  int rc;
  if (pc_on_) {
    rc = E.launch(K_AXPBY, 24.0 * n, [&] {
      return shlin_diag_sum_launch(U, Uo, k_, g_, d, n, E.partial(), E.s, &nblk);
    });
    if (!rc) rc = E.reduce_async(nblk, 1, 1, kSlotAux);  // sum D, read after the next reduce()
  } else {
    rc = E.launch(K_AXPBY, 24.0 * n, [&] { return shlin_diag_launch(U, Uo, k_, g_, d, n, E.s); });
  }
  // b = (I + L k/2) U  (the zero vector stands in for D)
  if (!rc) rc = linop(U, U, 0.0, zero, -k_ / 2, pn, b, &nblk);
  // |b|^2 (combo rewrites b unchanged and sums its squares)
  VecList none{};
  if (!rc) rc = E.launch(K_COMBO, 16.0 * n, [&] {
    return combo_launch(b, b, 1.0, none, 0, n, E.partial(), E.s, &nblk);
  });
  if (!rc) rc = E.reduce(nblk, 1, 2, red);
  if (rc) return rc;
  const double bnorm = std::sqrt(red[0]);
  if (pc_on_) {
    const double dmean = *E.hres(kSlotAux) / double(n);
    if (!std::isfinite(dmean)) return NK_NONFINITE;
    sigma = dmean > 0.0 ? dmean : 0.0;
    last_.shift = sigma;
    if (st) *st = last_;
  }
  // warm start x = U: r = b - A U (and z = M r)
  rc = E.copy(x, U, n);
  if (!rc) rc = linop(U, U, 0.0, d, k_ / 2, pn, q, &nblk);
  VecList mq{};
  mq.p[0] = q;
  mq.c[0] = -1.0;
  if (!rc) rc = E.launch(K_COMBO, 24.0 * n, [&] {
    return combo_launch(r, b, 1.0, mq, 1, n, E.partial(), E.s, &nblk);
  });
  if (!rc) rc = residual_dots(2);
  if (rc) return rc;
  const double stop = rtol_ * bnorm;
  double beta = 0.0;
  int64_t it = 0;
  while (std::sqrt(rr) > stop && it < maxiter_) {
    // M is positive definite: non-finite data (without M, rho = r.r > stop^2 here)
    if (!(rho > 0.0)) return NK_NONFINITE;
    // p' = z + beta p; q = A p'; p'.q
    rc = linop(z, it == 0 ? z : p, beta, d, k_ / 2, pn, q, &nblk);
    if (!rc) rc = E.reduce(nblk, 1, 3, red);
    if (rc) return rc;
    const double pq = red[0];
    if (!(pq > 0.0)) return NK_NONFINITE;  // not SPD (g k U dominated) or non-finite data
    const double alpha = rho / pq, rho_old = rho;
    rc = E.launch(K_AXPBY, 48.0 * n, [&] {
      return cg_update_launch(x, r, pn, q, alpha, n, E.partial(), E.s, &nblk);
    });
    if (!rc) rc = residual_dots(1);
    if (rc) return rc;
    beta = rho / rho_old;
    std::swap(p, pn);
    ++it;
  }
  rc = E.copy(Unew, x, n);
  if (!rc) rc = E.sync();
  last_.iters = it;
  last_.relres = bnorm > 0 ? std::sqrt(rr) / bnorm : std::sqrt(rr);
  last_.precond_applies = napp;
  if (st) *st = last_;
  if (rc) return rc;
  return std::isfinite(rr) ? (std::sqrt(rr) <= stop ? NK_OK : NK_NO_CONVERGENCE) : NK_NONFINITE;
}

}  // namespace nk
