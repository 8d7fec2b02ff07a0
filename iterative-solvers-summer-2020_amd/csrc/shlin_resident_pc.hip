// The resident semi-implicit Swift-Hohenberg step (shlin_resident.hip) with the spectral
// preconditioner applied on chip (gfx950): preconditioned CG as ShLinStepper::step runs it with
// NK_PC_SPECTRAL, one workgroup per state, whole steps in one launch.
//
//   sigma = max(mean D, 0),  M = ((1 + sigma) I - L k/2)^-1,  z = M res,  rho = res.z,
//   p = z + (rho / rho_old) p,  alpha = rho / p.Ap,  stop on sqrt(res.res) <= rtol |b|.
//
// The ownership scheme is the plain kernel's: a thread owns the points t, t + BS, ... and keeps
// their x, res, U, Uo in registers, q = A p between the stencil and the update, and the search
// direction is the framed LDS plane.  New is z = M res, a 2-D real FFT, the symbol and the FFT back,
// in a second LDS region; z never takes a register plane (the owner reads it from that region for
// rho and again for the new p), and q's registers are dead while the transform runs.
//
// LDS map (doubles; 128 x 64 in brackets, 140 928 B in all)
//   plane     (ny + 4)(nx + 4)   the framed search direction                        [71 808 B]
//   spectrum  ny (nx + 2)        ny rows of nx/2 + 1 complex values: the residual in natural
//                                layout, then its packed half spectrum (fftpc.hip's: a row of nx
//                                reals is nx/2 complex values, X[0] and X[nx/2] share entry 0),
//                                then z.  The one value of padding per row makes the row stride
//                                odd in 16-B units, so that a wave walking down columns spreads
//                                over the banks.                                    [67 584 B]
//   tables    nx + ny            exp(-2 pi i j/nx), j < nx/2; exp(-2 pi i j/ny), j < ny/2, staged
//                                once per launch from the stepper's device table: twiddles and
//                                the symbol's cosines, no sincos on the device.      [1 536 B]
//   sums      static, 2 x 3 x (waves) doubles
//
// The wave-local transforms and apply_M are in shlin_resident_pc_dev.h, which the resident implicit
// step (sh_resident.hip) includes as well.
//
// Block barriers per application of M: four, one at each change of ownership -- registers to
// rows (the barrier of the r.r sum: the update stores the new residual into the spectrum region
// before that sum), rows to columns, columns to rows, rows to owners -- and a fifth for rho.  With
// the plain kernel's (p published; p.q; r.r) that is seven per CG iteration.  M is applied at the
// top of an iteration, after the stop test: iterations and applications are equal in number.
//
// No block waits for, signals or reads another; every loop is bounded by maxiter, nsteps and the
// transforms' stage counts.
#include <cmath>

#include "shlin_resident_pc_dev.h"

namespace nk {

namespace {

extern __shared__ __align__(16) double resident_pc_lds[];

template <int BS, int PPT>
__global__ void __launch_bounds__(BS) shlin_resident_pc_kernel(ShLinResidentPcArgs P) {
  constexpr int NW = BS / 64;
  __shared__ double red[2][3][NW];
  const ShLinResidentArgs& A = P.a;
  const int ny = A.ny, nx = A.nx, n = ny * nx, ld = nx + 4, rowspan = ny * ld;
  const int lx = 31 - __clz(nx), ly = 31 - __clz(ny), n2 = nx >> 1;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* fr = resident_pc_lds;
  double* Sd = fr + (ny + 4) * ld;  // an even count of doubles: 16-B aligned
  cd* S = reinterpret_cast<cd*>(Sd);
  cd* twx = S + ny * (n2 + 1);
  cd* twy = twx + n2;
  {
    const cd* tab = reinterpret_cast<const cd*>(P.tables);
    for (int i = t; i < (nx + ny) >> 1; i += BS) twx[i] = tab[i];  // behind the first barrier
  }
  const PcShare G = pc_share<NW>(w, lx, ly);

  const int64_t m = blockIdx.x;
  const double* Ug = A.U + m * n;
  const double* Uog = A.Uo + m * n;
  // the centre coefficient of L, D, the symbol and sigma depend on the member's r and g
  const double rm = A.r ? A.r[m] : A.r0, gm = A.g ? A.g[m] : A.g0;
  const double c0 = A.cbase + rm - 1.0, c1 = A.c1, c2 = A.c2, c3 = A.c3;
  const double k = A.k, kh = A.k / 2, gk = gm * A.k;

  int code[PPT];
  double u[PPT], uo[PPT], x[PPT], r[PPT], q[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = t + j * BS;
    code[j] = point_code(i, ny, nx);
    u[j] = i < n ? Ug[i] : 0.0;
    uo[j] = i < n ? Uog[i] : 0.0;
    x[j] = r[j] = q[j] = 0.0;
  }
  // a live point's place in the spectrum region: row stride nx + 2 doubles
  // (formed where it is used, like what derives from a point's code)
  auto spec = [&](int j) {
    const int i = fresh(t) + j * BS;
    return i + 2 * (i >> lx);
  };

  int64_t iters = 0, steps = 0, applies = 0, status = kOk;
  double relres = 0.0, sigma = 0.0;
  // k r >= 2 (or a non-finite r): the symbol need not be positive -- the member never starts
  const bool refused = !(k * rm < 2.0);
  if (refused) status = kNonFinite;
  for (int64_t s = 0; s < A.nsteps && !refused; ++s) {
    // the plane holds U: b = (I + L k/2) U, and the warm start x = U gives r = b - A U
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int c = fresh(code[j]);
      if (c & kLive) put_p(fr, c, u[j], rowspan, nx);
    }
    __syncthreads();
    double v3[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int c = fresh(code[j]);
      const bool act = c & kLive;
      const double a = 5 * u[j] - uo[j];
      const double d = a * a * k / 16 - gk * u[j];
      const double Lu = apply_L(fr, c & 0xffff, ld, c0, c1, c2, c3);
      const double b = act ? u[j] + kh * Lu : 0.0;
      r[j] = act ? b - ((1.0 + d) * u[j] - kh * Lu) : 0.0;
      x[j] = u[j];
      if (act) Sd[spec(j)] = r[j];
      v3[0] += b * b;
      v3[1] += r[j] * r[j];
      v3[2] += act ? d : 0.0;
      __builtin_amdgcn_sched_barrier(0);  // one point's 13 reads in flight, not all PPT points'
    }
    block_sum_all<3, BS>(v3, red[1]);  // its barrier publishes the residual's rows as well
    const double bnorm = sqrt(v3[0]), stop = A.rtol * bnorm;
    const double dmean = v3[2] / double(n);
    sigma = dmean > 0.0 ? dmean : 0.0;
    const Symbol sym{P.ih2, rm, (1.0 + sigma) / k, 1.0 / (k * double(n))};
    double rr = v3[1], rho = 0.0;
    int64_t it = 0;
    bool bad = !isfinite(dmean);
    while (!bad && sqrt(rr) > stop && it < A.maxiter) {
      if (!(rr > 0.0)) {  // above the stop and not positive: non-finite data
        bad = true;
        break;
      }
      apply_M(S, twx, twy, G, sym, lane);
      ++applies;
      double v1[1] = {0.0};
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive) v1[0] += r[j] * Sd[spec(j)];
      }
      block_sum_all<1, BS>(v1, red[0]);
      const double rho_old = rho;
      rho = v1[0];
      if (!(rho > 0.0)) {  // M is positive definite: non-finite data
        bad = true;
        break;
      }
      const double beta = it == 0 ? 0.0 : rho / rho_old;
      // p = z + beta p.  The last readers of the plane and its frame (the stencil, the owner's own
      // read in the update) are behind the r.r barrier; z stays where it is until the next
      // update's stores, which are behind this barrier and the p.q one.
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive) {
          const double z = Sd[spec(j)];
          put_p(fr, c, it == 0 ? z : z + beta * fr[c & 0xffff], rowspan, nx);
        }
      }
      __syncthreads();
      v1[0] = 0.0;
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]), f = c & 0xffff;
        const double uj = fresh(u[j]), a = 5 * uj - uo[j];
        const double d = a * a * k / 16 - gk * uj;
        const double p = fr[f];
        q[j] = (1.0 + d) * p - kh * apply_L(fr, f, ld, c0, c1, c2, c3);
        v1[0] += c & kLive ? p * q[j] : 0.0;
        __builtin_amdgcn_sched_barrier(0);
      }
      block_sum_all<1, BS>(v1, red[1]);
      const double pq = v1[0];
      if (!(pq > 0.0)) {  // not SPD (g k U dominated) or non-finite data
        bad = true;
        break;
      }
      const double alpha = rho / pq;
      v1[0] = 0.0;
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive) {
          x[j] += alpha * fr[c & 0xffff];
          r[j] -= alpha * q[j];
          Sd[spec(j)] = r[j];
          v1[0] += r[j] * r[j];
        }
      }
      block_sum_all<1, BS>(v1, red[0]);
      rr = v1[0];
      ++it;
    }
    iters += it;
    relres = bnorm > 0 ? sqrt(rr) / bnorm : sqrt(rr);
    status = bad || !isfinite(rr) ? kNonFinite : (sqrt(rr) <= stop ? kOk : kNoConv);
    if (status != kOk) break;  // (U, Uo) stay the last accepted pair
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      uo[j] = u[j];
      u[j] = x[j];
    }
    ++steps;
  }

  double* Un = A.Unew + m * n;
  double* Up = A.Uprev ? A.Uprev + m * n : nullptr;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = t + j * BS;
    if (i < n) {
      Un[i] = u[j];
      if (Up) Up[i] = uo[j];
    }
  }
  if (t == 0) {
    A.out[m] = ShLinResidentOut{iters, steps, relres, status};
    P.out[m] = ShLinResidentPcOut{applies, sigma};
  }
}

template <int BS, int PPT>
hipError_t launch_variant(const ShLinResidentPcArgs& P, int64_t batch, hipStream_t s) {
  const size_t lds = resident_pc_lds_bytes(P.a.ny, P.a.nx);
  if (lds > 65536) {  // once per variant: the largest footprint under the cap
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&shlin_resident_pc_kernel<BS, PPT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, int(resident_pc_lds_bytes(128, 64)));
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL((shlin_resident_pc_kernel<BS, PPT>), dim3(unsigned(batch)), dim3(BS), lds, s,
                     P);
  return hipGetLastError();
}

}  // namespace

bool shlin_resident_pc_fits(int64_t ny, int64_t nx) {
  auto side = [](int64_t v) { return v >= 8 && v <= 128 && (v & (v - 1)) == 0; };
  return side(ny) && side(nx) && ny * nx <= kShLinResidentPcMaxPoints;
}

void shlin_resident_pc_tables(int64_t ny, int64_t nx, double* out) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int64_t len : {nx, ny}) {  // sides >= 8: j = len/4 is in the table
    for (int64_t j = 0; j < len / 2; ++j) {
      const long double a = two_pi * static_cast<long double>(j) / static_cast<long double>(len);
      out[2 * j] = static_cast<double>(cosl(a));
      out[2 * j + 1] = static_cast<double>(-sinl(a));
    }
    out[0] = 1.0;
    out[1] = 0.0;
    out[2 * (len / 4)] = 0.0;
    out[2 * (len / 4) + 1] = -1.0;
    out += len;
  }
}

hipError_t shlin_resident_pc_launch(const ShLinResidentPcArgs& P, int64_t batch, hipStream_t s) {
  if (!shlin_resident_pc_fits(P.a.ny, P.a.nx) || batch < 1 || batch > 0x7fffffff || !P.tables ||
      !P.out)
    return hipErrorInvalidValue;
  const int n = P.a.ny * P.a.nx;
  // the plain kernel's shapes: four waves for few points (cheaper barriers, several members per
  // CU), four points per thread up to 64 x 64, and at the cap eight waves of sixteen points (the
  // five register planes are 160 VGPRs of the 256 a thread of such a block may hold)
  if (n <= 1024) return launch_variant<256, 4>(P, batch, s);
  if (n <= 4096) return launch_variant<1024, 4>(P, batch, s);
  static_assert(512 * 16 >= kShLinResidentPcMaxPoints, "every point under the cap needs an owner");
  return launch_variant<512, 16>(P, batch, s);
}

}  // namespace nk
