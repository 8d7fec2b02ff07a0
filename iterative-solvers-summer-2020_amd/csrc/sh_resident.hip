// The implicit Crank-Nicolson Swift-Hohenberg step (SwiftHohenberg.step, sh_scipy_nk.py:47-61) for
// small grids, resident on one CU (gfx950): Newton-CG with the analytic Jacobian.
//
// NewtonKrylov::solve spends a 64 x 64 step on launches and read-backs: five Newton iterations and
// well over a hundred Arnoldi steps around a few hundred nanoseconds of arithmetic each.  Here one
// workgroup owns one state and runs whole steps in a single launch; a batch of independent states
// is one block each.  No block waits for, signals or reads another, and every loop is bounded by
// nsteps, Newton's maxiter, the inner cap, the line search's amin or the transforms' stage counts.
//
// The method.  With c = Uo/k + (L Uo + g Uo^2 - Uo^3)/2 the residual is
//   F(u) = u/k - (L u + g u^2 - u^3)/2 - c,   J(u) = (1/k + d) I - L/2,   d = 1.5 u^2 - g u,
// and k J = I + k d - L k/2 is the resident semi-implicit kernels' matrix with another diagonal:
// symmetric, and positive definite whenever k (g^2/6 + r/2) < 1 (L <= r, d >= -g^2/6).  So the
// Newton correction J dx = -F is solved by CG -- plain, or (PC) with the spectral preconditioner
// M = ((1 + sigma)/k I - L/2)^-1, sigma = max(mean k d, 0) at the current iterate, applied on chip
// by shlin_resident_pc_dev.h -- where NewtonKrylov::solve runs LGMRES on a difference quotient.
// Around it the loop is that solver's (nk_solver.cpp), in scalars every lane holds alike: stop on
// max|F| <= f_tol; Eisenstat-Walker forcing (eta0 = 1e-3, gamma = 0.9, eta_max = 0.9999,
// threshold 0.1), the inner solve run to |res| <= min(eta, eta |F|) |F| or to inner_maxiter
// iterations, whichever comes first (reaching the cap is no failure: Newton goes on with the dx it
// has, as after one LGMRES cycle); the Armijo search of scalar_search_armijo (c1 = 1e-4,
// amin = 1e-2, a quadratic then cubic steps) on phi(s) = |F(u + s dx)|^2.
//
// Where the data live (the resident kernels' scheme: a thread owns the points t, t + BS, ...)
//   u      the Newton iterate                                  registers
//   c      the step's constant, formed once from the plane that holds Uo
//   dx     the Newton correction (CG's x, started from 0)
//   res    -F(u), then CG's residual
//   q      J p in CG; F at the trial point in the line search (an accepted trial is the next res)
//   plane  one framed LDS plane (shlin_resident_dev.h), in turn: Uo, CG's search direction, the
//          trial point u + s dx (the owner takes the accepted trial back from it)
//   PC     the spectrum region and tables of shlin_resident_pc.hip behind the plane; z = M res never
//          takes a register plane
// d is formed from u where it is used.  The last accepted state of a member is its row of Unew in
// HBM: the input at first, then each completed step, so a member that fails inside a step leaves
// the state it entered that step with.  HBM sees U once, n doubles per step, 56 bytes per member.
//
// Reductions are fixed-order block sums (and a block max of |F| built the same way), returned to
// every thread with the same bits: branches are uniform, and a member's bits depend on its own
// inputs alone.  Barriers per CG iteration: three plain, seven preconditioned, as in the
// semi-implicit kernels; the reduction buffers alternate so that a buffer is rewritten only after
// a barrier that every reader of its last use has passed, and the F evaluations (each behind the
// barrier that publishes its trial point) have a buffer of their own.
#include <cmath>

#include "shlin_resident_pc_dev.h"

namespace nk {

namespace {

// v[1] max-reduced, the others summed, over the block; every thread gets the same bits.
template <int NV, int BS>
__device__ __forceinline__ void block_sum_max_all(double (&v)[NV], double (*sm)[BS / 64]) {
  constexpr int NW = BS / 64;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double t = __shfl_xor(v[k], o, 64);
      v[k] = k == 1 ? fmax(v[k], t) : v[k] + t;
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sm[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double acc = sm[k][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc = k == 1 ? fmax(acc, sm[k][w]) : acc + sm[k][w];
    v[k] = uniform(acc);
  }
}

extern __shared__ __align__(16) double sh_resident_lds[];

template <int BS, int PPT, bool PC>
__global__ void __launch_bounds__(BS) sh_resident_kernel(ShResidentArgs A) {
  constexpr int NW = BS / 64, NF = PC ? 3 : 2;
  __shared__ double red[2][1][NW];  // CG's sums
  __shared__ double redf[NF][NW];   // an F evaluation's: |F|^2, max|F|, (PC) sum k d
  const int ny = A.ny, nx = A.nx, n = ny * nx, ld = nx + 4, rowspan = ny * ld;
  const int lx = 31 - __clz(nx), ly = 31 - __clz(ny), n2 = nx >> 1;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* fr = sh_resident_lds;
  double* Sd = fr + (ny + 4) * ld;  // PC: nx even, an even count of doubles, 16-B aligned
  cd* S = reinterpret_cast<cd*>(Sd);
  cd* twx = S + ny * (n2 + 1);
  cd* twy = twx + n2;
  PcShare G{};
  if constexpr (PC) {
    const cd* tab = reinterpret_cast<const cd*>(A.tables);
    for (int i = t; i < (nx + ny) >> 1; i += BS) twx[i] = tab[i];  // behind the first barrier
    G = pc_share<NW>(w, lx, ly);
  }

  const int64_t m = blockIdx.x;
  const double* Ug = A.U + m * n;
  double* Un = A.Unew + m * n;
  // the centre coefficient of L, d, the symbol and sigma depend on the member's r and g
  const double rm = A.r ? A.r[m] : A.r0, gm = A.g ? A.g[m] : A.g0;
  const double c0 = A.cbase + rm - 1.0, c1 = A.c1, c2 = A.c2, c3 = A.c3;
  const double k = A.k, ik = 1.0 / A.k;

  int code[PPT];
  double u[PPT], cc[PPT], dx[PPT], res[PPT], q[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = t + j * BS;
    code[j] = point_code(i, ny, nx);
    u[j] = i < n ? Ug[i] : 0.0;
    if (i < n) Un[i] = u[j];  // the member's answer until a step completes
    cc[j] = dx[j] = res[j] = q[j] = 0.0;
  }
  // a live point's place in the spectrum region: row stride nx + 2 doubles
  // (formed where it is used, like what derives from a point's code)
  auto spec = [&](int j) {
    const int i = fresh(t) + j * BS;
    return i + 2 * (i >> lx);
  };

  int64_t nit = 0, iters = 0, steps = 0, applies = 0, status = kOk;
  double fmx = 0.0, sigma = 0.0;
  // J need not be positive definite (or r, g are not finite); PC: nor the symbol positive.  The
  // member never starts.
  if (!(k * (gm * gm / 6 + rm / 2) < 1.0) || (PC && !(k * rm < 2.0))) status = kNonFinite;
  for (int64_t s = 0; s < A.nsteps && status == kOk; ++s) {
    // the plane holds Uo = u: W = L Uo + g Uo^2 - Uo^3 gives c, and F(Uo) = -W
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int c = fresh(code[j]);
      if (c & kLive) put_p(fr, c, u[j], rowspan, nx);
    }
    __syncthreads();
    double vf[NF] = {};
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int c = fresh(code[j]);
      const bool act = c & kLive;
      const double uj = u[j];
      const double W = apply_L(fr, c & 0xffff, ld, c0, c1, c2, c3) + (gm - uj) * uj * uj;
      cc[j] = act ? uj * ik + 0.5 * W : 0.0;
      res[j] = act ? W : 0.0;
      vf[0] += res[j] * res[j];
      vf[1] = fmax(vf[1], fabs(res[j]));
      if constexpr (PC) {
        vf[2] += act ? k * (1.5 * uj - gm) * uj : 0.0;
        if (act) Sd[spec(j)] = res[j];
      }
      __builtin_amdgcn_sched_barrier(0);  // one point's 13 reads in flight, not all PPT points'
    }
    block_sum_max_all<NF, BS>(vf, redf);  // PC: its barrier publishes the residual's rows as well
    double fn2 = vf[0], dsum = PC ? vf[NF - 1] : 0.0;
    fmx = vf[1];

    double eta = 1e-3;
    int64_t it = 0;
    for (;;) {
      if (!isfinite(fn2)) {
        status = kNonFinite;
        break;
      }
      if (fmx <= A.f_tol) break;  // converged
      if (it >= A.maxiter) {
        status = kNoConv;
        break;
      }
      // ---- J dx = -F by CG from dx = 0 (res = -F is in place; PC: its rows are in S)
      const double fn = sqrt(fn2), stop = fmin(eta, eta * fn) * fn;
      Symbol sym{};
      if constexpr (PC) {
        const double dmean = dsum / double(n);
        sigma = dmean > 0.0 ? dmean : 0.0;
        sym = Symbol{A.ih2, rm, (1.0 + sigma) * ik, 1.0 / double(n)};
      }
#pragma unroll
      for (int j = 0; j < PPT; ++j) dx[j] = 0.0;
      double rr = fn2, rho = 0.0, beta = 0.0;
      int64_t cit = 0;
      bool bad = false;
      while (sqrt(rr) > stop && cit < A.inner_maxiter) {
        if (!(rr > 0.0)) {  // above the stop and not positive: non-finite data
          bad = true;
          break;
        }
        // the new search direction.  The last readers of the plane and its frame (the stencil, the
        // owner's own read in the update) are behind the r.r barrier.
        if constexpr (PC) {
          apply_M(S, twx, twy, G, sym, lane);
          ++applies;
          double v1[1] = {0.0};
#pragma unroll
          for (int j = 0; j < PPT; ++j) {
            const int c = fresh(code[j]);
            if (c & kLive) v1[0] += res[j] * Sd[spec(j)];
          }
          block_sum_all<1, BS>(v1, red[0]);
          const double rho_old = rho;
          rho = v1[0];
          if (!(rho > 0.0)) {  // M is positive definite: non-finite data
            bad = true;
            break;
          }
          beta = cit == 0 ? 0.0 : rho / rho_old;
#pragma unroll
          for (int j = 0; j < PPT; ++j) {
            const int c = fresh(code[j]);
            if (c & kLive) {
              const double z = Sd[spec(j)];
              put_p(fr, c, cit == 0 ? z : z + beta * fr[c & 0xffff], rowspan, nx);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < PPT; ++j) {
            const int c = fresh(code[j]);
            if (c & kLive)
              put_p(fr, c, cit == 0 ? res[j] : res[j] + beta * fr[c & 0xffff], rowspan, nx);
          }
        }
        __syncthreads();
        double v1[1] = {0.0};
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]), f = c & 0xffff;
          const double uj = fresh(u[j]);
          const double d = (1.5 * uj - gm) * uj;
          const double p = fr[f];
          q[j] = (ik + d) * p - 0.5 * apply_L(fr, f, ld, c0, c1, c2, c3);
          v1[0] += c & kLive ? p * q[j] : 0.0;
          __builtin_amdgcn_sched_barrier(0);
        }
        block_sum_all<1, BS>(v1, red[PC ? 1 : 0]);
        const double pq = v1[0];
        if (!(pq > 0.0)) {  // J not positive definite at this u, or non-finite data
          bad = true;
          break;
        }
        const double alpha = (PC ? rho : rr) / pq, rr_old = rr;
        v1[0] = 0.0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]);
          if (c & kLive) {
            dx[j] += alpha * fr[c & 0xffff];
            res[j] -= alpha * q[j];
            if constexpr (PC) Sd[spec(j)] = res[j];
            v1[0] += res[j] * res[j];
          }
        }
        block_sum_all<1, BS>(v1, red[PC ? 0 : 1]);
        rr = v1[0];
        beta = rr / rr_old;  // (plain CG's)
        ++cit;
      }
      iters += cit;
      if (bad || !isfinite(rr)) {
        status = kNonFinite;
        break;
      }

      // ---- the step length: scalar_search_armijo on phi(s) = |F(u + s dx)|^2, phi'(0) = -phi(0).
      // stage 0: s = 1; 1: the quadratic's minimiser; 2: a cubic's; 3: the evaluation that is
      // accepted as it is (no line search, or amin passed: "the full Newton step").
      const double phi0 = fn2, derphi0 = -fn2, c1a = 1e-4, amin = 1e-2;
      double sT = 1.0, a0 = 1.0, a1 = 0.0, pa0 = 0.0, pa1 = 0.0, phi_raw = 0.0;
      int stage = A.line_search ? 0 : 3;
      for (;;) {
        // the trial point into the plane (its last readers are behind a sum's barrier), F there
        // into q
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]);
          if (c & kLive) put_p(fr, c, u[j] + sT * dx[j], rowspan, nx);
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < NF; ++k2) vf[k2] = 0.0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]), f = c & 0xffff;
          const bool act = c & kLive;
          const double x = fr[f];
          const double W = apply_L(fr, f, ld, c0, c1, c2, c3) + (gm - x) * x * x;
          q[j] = act ? x * ik - 0.5 * W - fresh(cc[j]) : 0.0;
          vf[0] += q[j] * q[j];
          vf[1] = fmax(vf[1], fabs(q[j]));
          if constexpr (PC) {
            vf[2] += act ? k * (1.5 * x - gm) * x : 0.0;
            if (act) Sd[spec(j)] = -q[j];  // the next solve's residual, if this trial is accepted
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        block_sum_max_all<NF, BS>(vf, redf);
        phi_raw = vf[0];
        const double phi = isfinite(phi_raw) ? phi_raw : INFINITY;
        if (stage == 3 || phi <= phi0 + c1a * sT * derphi0) break;
        if (stage == 0) {
          pa0 = phi;
          a1 = -(derphi0)*a0 * a0 / 2.0 / (pa0 - phi0 - derphi0 * a0);
          stage = 1;
          sT = a1;
          continue;
        }
        if (stage == 1) {
          pa1 = phi;
          stage = 2;
        } else {
          double a2 = sT;
          if ((a1 - a2) > a1 / 2.0 || (1 - a2 / a1) < 0.96) a2 = a1 / 2.0;
          a0 = a1;
          a1 = a2;
          pa0 = pa1;
          pa1 = phi;
        }
        if (!(a1 > amin)) {
          sT = 1.0;
          stage = 3;
          continue;
        }
        const double factor = a0 * a0 * a1 * a1 * (a1 - a0);
        double a = a0 * a0 * (pa1 - phi0 - derphi0 * a1) - a1 * a1 * (pa0 - phi0 - derphi0 * a0);
        a = a / factor;
        double b = -a0 * a0 * a0 * (pa1 - phi0 - derphi0 * a1) +
                   a1 * a1 * a1 * (pa0 - phi0 - derphi0 * a0);
        b = b / factor;
        sT = (-b + sqrt(fabs(b * b - 3 * a * derphi0))) / (3.0 * a);
      }
      if (!isfinite(phi_raw)) {
        status = kNonFinite;
        break;
      }
      // accepted: the plane holds the new iterate, q its F
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive) {
          u[j] = fr[c & 0xffff];
          res[j] = -q[j];
        }
      }
      const double gamma = 0.9, eta_max = 0.9999, eta_threshold = 0.1;
      const double eta_A = gamma * phi_raw / fn2;
      if (gamma * eta * eta < eta_threshold)
        eta = fmin(eta_max, eta_A);
      else
        eta = fmin(eta_max, fmax(eta_A, gamma * eta * eta));
      fn2 = phi_raw;
      fmx = vf[1];
      if constexpr (PC) dsum = vf[NF - 1];
      ++it;
    }
    nit += it;
    if (status != kOk) break;  // the member's row of Unew stays its last accepted state
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int i = t + j * BS;
      if (i < n) Un[i] = u[j];
    }
    ++steps;
  }
  if (t == 0) A.out[m] = ShResidentOut{nit, iters, steps, applies, fmx, sigma, status};
}

template <int BS, int PPT, bool PC>
hipError_t launch_variant(const ShResidentArgs& A, int64_t batch, hipStream_t s) {
  const size_t lds = PC ? resident_pc_lds_bytes(A.ny, A.nx)
                        : sizeof(double) * size_t(A.ny + 4) * size_t(A.nx + 4);
  if (lds > 65536) {  // once per variant: the largest footprint under the cap
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&sh_resident_kernel<BS, PPT, PC>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        PC ? int(resident_pc_lds_bytes(128, 64)) : int(kShLinResidentMaxLds));
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL((sh_resident_kernel<BS, PPT, PC>), dim3(unsigned(batch)), dim3(BS), lds, s, A);
  return hipGetLastError();
}

}  // namespace

hipError_t sh_resident_launch(const ShResidentArgs& A, int64_t batch, hipStream_t s) {
  const bool pc = A.tables != nullptr;
  if (!(pc ? shlin_resident_pc_fits(A.ny, A.nx) : shlin_resident_fits(A.ny, A.nx)) || batch < 1 ||
      batch > 0x7fffffff || !A.U || !A.Unew || !A.out || A.nsteps < 1 || A.maxiter < 1 ||
      A.inner_maxiter < 1 || !(A.k > 0.0))
    return hipErrorInvalidValue;
  const int n = A.ny * A.nx;
  // the semi-implicit kernels' shapes: four waves for few points (cheaper barriers, several
  // members per CU), four points per thread up to 64 x 64, eight waves of eighteen (plain) or
  // sixteen (preconditioned) points to the caps
  if (n <= 1024)
    return pc ? launch_variant<256, 4, true>(A, batch, s) : launch_variant<256, 4, false>(A, batch, s);
  if (n <= 4096)
    return pc ? launch_variant<1024, 4, true>(A, batch, s)
              : launch_variant<1024, 4, false>(A, batch, s);
  static_assert(512 * 18 >= kShLinResidentMaxPoints && 512 * 16 >= kShLinResidentPcMaxPoints,
                "every point under the caps needs an owner");
  return pc ? launch_variant<512, 16, true>(A, batch, s)
            : launch_variant<512, 18, false>(A, batch, s);
}

}  // namespace nk
