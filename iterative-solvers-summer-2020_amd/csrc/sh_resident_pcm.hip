// The implicit Crank-Nicolson Swift-Hohenberg step of sh_resident.hip (Newton-CG with the analytic
// Jacobian, one workgroup per state, whole steps in one launch) with the spectral preconditioner
// on grids whose sides are 2^a 3^b 5^c (gfx950): sh_resident_kernel<BS, PPT, true> around the
// wave-local mixed-radix z = M res of shlin_resident_pcm.hip,
//   M = ((1 + sigma)/k I - L/2)^-1,  sigma = max(mean k (1.5 u^2 - g u), 0) at the current iterate.
//
// sh_resident.hip is the method of record; its header says what holds and it holds here: the
// residual F, J = (1/k + d) I - L/2, the stop on max|F| <= f_tol, Eisenstat-Walker forcing, the
// inner solve to its tolerance or inner_maxiter, the Armijo stages, the refusals
// k (g^2/6 + r/2) >= 1 and k r >= 2, a member's row of Unew holding its last accepted state, and
// fixed-order block sums, so a member's bits depend on its own inputs alone.  That file is not
// touched; the Newton-CG body is written here a second time.
//
// Where the data live.  Thread t owns the points t, t + BS, ...: u, c, dx, res and q in registers,
// one framed LDS plane in turn Uo, CG's search direction and the trial point.  Behind the plane the
// LDS map of shlin_resident_pcm.hip: the spectrum region (ny rows of ldc complex values, ldc odd in
// 16-B units; the residual, then its packed half spectrum, then z, in place), the full root tables
// and the permutations, staged once per launch.  The dynamic footprint is
// shlin_resident_pcm_lds_bytes(ny, nx), so the served grids are exactly those
// shlin_resident_pcm_fits admits (96 x 96: 158 912 B; 128 x 72: 159 888 B); the static sums
// (red[2][1][NW], redf[3][NW]: 640 B at sixteen waves) stay within the 768 B that check reserves.
//
// Design points settled here
//   transform code   shlin_resident_pcm_dev.h, moved there verbatim from shlin_resident_pcm.hip
//                    (PcmStages, PcmShare, qdiv, wave_stage, wave_mfft, apply_M), as the
//                    power-of-two kernels share shlin_resident_pc_dev.h.
//   a point's place  in the spectrum region, nx being no power of two: the semi-implicit mixed
//                    kernel's way.  The point's row rides in bits 21-27 of its code (one division
//                    per point at launch), and the place is frame offset - row (ld - 2 ldc) -
//                    (2 ld + 2): a multiply and two subtractions where it is used, no division in
//                    the CG loop.
//   shapes           256 x 4 up to 1024 points, 1024 x 4 up to 4096, 512 x 18 to the cap: the
//                    siblings'.  A grid of few rows leaves waves without rows or columns; their
//                    transform loops are empty and they meet every barrier.
//   registers        sigma-dependent values (the Symbol) are formed per Newton iteration from
//                    scalars; the transform loops are not unrolled; sched_barrier keeps one point's
//                    stencil reads in flight.  profiles/sh_resident_mixed.md has the compiler's
//                    figures next to the semi-implicit kernel's.
//   barriers         four block barriers per application of M, seven per CG iteration.  CG's two
//                    reduction buffers alternate (rho: 0, p.q: 1, r.r: 0) so that a buffer is
//                    rewritten only after a barrier every reader of its last use has passed; the F
//                    evaluations, each behind the barrier that publishes its trial point, have
//                    redf.
//
// No block waits for, signals or reads another; every loop is bounded by nsteps, Newton's maxiter,
// inner_maxiter, the line search's amin or the transforms' stage counts.  No inline assembly beyond
// the empty value barrier of shlin_resident_dev.h.
#include <algorithm>
#include <cmath>

#include "shlin_resident_pcm_dev.h"

namespace nk {

namespace {

struct ShPcmArgs {
  ShResidentArgs a;
  PcmStages sx, sy;    // rows (length nx/2), columns (length ny)
  int ldc = 0;         // the spectrum's row stride in complex values
  unsigned rpack = 0;  // reciprocal of nx/4 + 1, the pairs (k, nx/2 - k) of a row
};

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

extern __shared__ __align__(16) double sh_resident_pcm_lds[];

template <int BS, int PPT>
__global__ void __launch_bounds__(BS) sh_resident_pcm_kernel(ShPcmArgs Q) {
  constexpr int NW = BS / 64, NF = 3;
  __shared__ double red[2][1][NW];  // CG's sums
  __shared__ double redf[NF][NW];   // an F evaluation's: |F|^2, max|F|, sum k d
  static_assert(sizeof(red) + sizeof(redf) <= kStaticBytes,
                "the footprint check counts the static sums");
  const ShResidentArgs& A = Q.a;
  const int ny = A.ny, nx = A.nx, n = ny * nx, ld = nx + 4, rowspan = ny * ld;
  const int m = nx >> 1, ldc = Q.ldc;
  const int t = threadIdx.x, lane = t & 63;
  // the wave's number in scalar registers: what it owns, its loop bounds and the stage walk are
  // then uniform
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  double* fr = sh_resident_pcm_lds;
  double* Sd = fr + (ny + 4) * ld;  // an even count of doubles: 16-B aligned
  cd* S = reinterpret_cast<cd*>(Sd);
  cd* twx = S + ny * ldc;
  cd* twy = twx + nx;
  int* permx = reinterpret_cast<int*>(twy + ny);
  int* permy = permx + m;
  {
    double* dst = reinterpret_cast<double*>(twx);
    const int nt = 2 * (nx + ny) + ((m + ny + 1) >> 1);
    for (int i = t; i < nt; i += BS) dst[i] = A.tables[i];  // behind the first barrier
  }
  PcmShare G;
  G.ny = ny;
  G.m = m;
  G.ldc = ldc;
  {
    const int rpw = (ny + NW - 1) / NW, cpw = (m + NW - 1) / NW;
    G.row0 = min(w * rpw, ny);
    G.nr = min(rpw, ny - G.row0);
    G.col0 = min(w * cpw, m);
    G.nc = min(cpw, m - G.col0);
  }
  G.rnc = recip(max(G.nc, 1));  // the one division of the launch besides the points' rows
  G.rpack = Q.rpack;

  const int64_t mb = blockIdx.x;
  const double* Ug = A.U + mb * n;
  double* Un = A.Unew + mb * n;
  // the centre coefficient of L, d, the symbol and sigma depend on the member's r and g
  const double rm = A.r ? A.r[mb] : A.r0, gm = A.g ? A.g[mb] : A.g0;
  const double c0 = A.cbase + rm - 1.0, c1 = A.c1, c2 = A.c2, c3 = A.c3;
  const double k = A.k, ik = 1.0 / A.k;

  int code[PPT];
  double u[PPT], cc[PPT], dx[PPT], res[PPT], q[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = t + j * BS;
    // the point code of the plane, and the point's row above it (bits 21-27; 0 for an unused slot)
    code[j] = point_code(i, ny, nx) | ((i < n ? i / nx : 0) << 21);
    u[j] = i < n ? Ug[i] : 0.0;
    if (i < n) Un[i] = u[j];  // the member's answer until a step completes
    cc[j] = dx[j] = res[j] = q[j] = 0.0;
  }
  // a live point's place in the spectrum region, in doubles: row 2 ldc + col, from its frame
  // offset (row + 2) ld + col + 2 and its row
  const int f0 = 2 * ld + 2, dd = ld - 2 * ldc;
  auto spec = [&](int c) { return (c & 0xffff) - (c >> 21) * dd - f0; };

  int64_t nit = 0, iters = 0, steps = 0, applies = 0, status = kOk;
  double fmx = 0.0, sigma = 0.0;
  // J need not be positive definite, nor the symbol positive (or r, g are not finite).  The
  // member never starts.
  if (!(k * (gm * gm / 6 + rm / 2) < 1.0) || !(k * rm < 2.0)) status = kNonFinite;
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
      vf[2] += act ? k * (1.5 * uj - gm) * uj : 0.0;
      if (act) Sd[spec(c)] = res[j];
      __builtin_amdgcn_sched_barrier(0);  // one point's 13 reads in flight, not all PPT points'
    }
    block_sum_max_all<NF, BS>(vf, redf);  // its barrier publishes the residual's rows as well
    double fn2 = vf[0], dsum = vf[2];
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
      // ---- J dx = -F by preconditioned CG from dx = 0 (res = -F is in place, its rows are in S)
      const double fn = sqrt(fn2), stop = fmin(eta, eta * fn) * fn;
      const double dmean = dsum / double(n);
      sigma = dmean > 0.0 ? dmean : 0.0;
#pragma unroll
      for (int j = 0; j < PPT; ++j) dx[j] = 0.0;
      double rr = fn2, rho = 0.0;
      int64_t cit = 0;
      bool bad = false;
      while (sqrt(rr) > stop && cit < A.inner_maxiter) {
        if (!(rr > 0.0)) {  // above the stop and not positive: non-finite data
          bad = true;
          break;
        }
        // the symbol is formed here, from sigma, and is not held across the iteration
        const Symbol sym{A.ih2, rm, (1.0 + sigma) * ik, 1.0 / double(n)};
        apply_M(S, twx, twy, permx, permy, G, Q.sx, Q.sy, sym, lane);
        ++applies;
        double v1[1] = {0.0};
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]);
          if (c & kLive) v1[0] += res[j] * Sd[spec(c)];
        }
        block_sum_all<1, BS>(v1, red[0]);
        const double rho_old = rho;
        rho = v1[0];
        if (!(rho > 0.0)) {  // M is positive definite: non-finite data
          bad = true;
          break;
        }
        const double beta = cit == 0 ? 0.0 : rho / rho_old;
        // p = z + beta p.  The last readers of the plane and its frame (the stencil, the owner's
        // own read in the update) are behind the r.r barrier; z stays where it is until the next
        // update's stores, which are behind this barrier and the p.q one.
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]);
          if (c & kLive) {
            const double z = Sd[spec(c)];
            put_p(fr, c, cit == 0 ? z : z + beta * fr[c & 0xffff], rowspan, nx);
          }
        }
        __syncthreads();
        v1[0] = 0.0;
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
        block_sum_all<1, BS>(v1, red[1]);
        const double pq = v1[0];
        if (!(pq > 0.0)) {  // J not positive definite at this u, or non-finite data
          bad = true;
          break;
        }
        const double alpha = rho / pq;
        v1[0] = 0.0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const int c = fresh(code[j]);
          if (c & kLive) {
            dx[j] += alpha * fr[c & 0xffff];
            res[j] -= alpha * q[j];
            Sd[spec(c)] = res[j];
            v1[0] += res[j] * res[j];
          }
        }
        block_sum_all<1, BS>(v1, red[0]);
        rr = v1[0];
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
          vf[2] += act ? k * (1.5 * x - gm) * x : 0.0;
          if (act) Sd[spec(c)] = -q[j];  // the next solve's residual, if this trial is accepted
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
      dsum = vf[2];
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
  if (t == 0) A.out[mb] = ShResidentOut{nit, iters, steps, applies, fmx, sigma, status};
}

template <int BS, int PPT>
hipError_t launch_variant(const ShPcmArgs& Q, int64_t batch, hipStream_t s) {
  const size_t lds = shlin_resident_pcm_lds_bytes(Q.a.ny, Q.a.nx);
  // once per variant: whatever shlin_resident_pcm_fits lets through
  if (lds + kStaticBytes > 65536) {
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&sh_resident_pcm_kernel<BS, PPT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, int(kLdsBytes - kStaticBytes));
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL((sh_resident_pcm_kernel<BS, PPT>), dim3(unsigned(batch)), dim3(BS), lds, s, Q);
  return hipGetLastError();
}

}  // namespace

hipError_t sh_resident_pcm_launch(const ShResidentArgs& A, int64_t batch, hipStream_t s) {
  if (!shlin_resident_pcm_fits(A.ny, A.nx) || batch < 1 || batch > 0x7fffffff || !A.U || !A.Unew ||
      !A.out || !A.tables || A.nsteps < 1 || A.maxiter < 1 || A.inner_maxiter < 1 || !(A.k > 0.0))
    return hipErrorInvalidValue;
  ShPcmArgs Q;
  Q.a = A;
  Q.sx = walk_of(A.nx / 2);
  Q.sy = walk_of(A.ny);
  Q.ldc = spectrum_stride(A.nx);
  Q.rpack = recip(A.nx / 4 + 1);
  const int n = A.ny * A.nx;
  // the shapes of the sibling kernels: four waves for few points, four points per thread up to
  // 4096, and at the cap eight waves of eighteen points
  if (n <= 1024) return launch_variant<256, 4>(Q, batch, s);
  if (n <= 4096) return launch_variant<1024, 4>(Q, batch, s);
  static_assert(512 * 18 >= kShLinResidentPcMixedMaxPoints, "every point under the cap needs an owner");
  return launch_variant<512, 18>(Q, batch, s);
}

}  // namespace nk
