// The resident preconditioned CG of shlin_resident_pc.hip on grids whose sides are 2^a 3^b 5^c
// (gfx950): one workgroup per state, whole semi-implicit Swift-Hohenberg steps in one launch, with
//   sigma = max(mean D, 0),  M = ((1 + sigma) I - L k/2)^-1,  z = M res
// applied on chip by mixed-radix transforms that never leave a wave.
//
// Taken from shlin_resident_pc.hip as it is: the ownership scheme (thread t owns the points t,
// t + BS, ...; x, res, q, U, Uo in registers), the framed search-direction plane, a second LDS
// region that holds the residual, then its packed half spectrum, then z, in place, the CG body
// (written here a second time: that file stays untouched, so its code generation does), column 0
// carrying DC + Nyquist, 1/(nx ny) in the symbol, and four block barriers per application of M,
// seven per CG iteration.  New is the transform; its device code is in shlin_resident_pcm_dev.h,
// which sh_resident_pcm.hip (the implicit Newton-CG step on these grids) includes as well.
//
// LDS map (doubles; 96 x 96 in brackets, 158 912 B in all, and 128 x 72, the largest footprint
// under the cap, 159 888 B; the static sums add 384 B)
//   plane     (ny + 4)(nx + 4)    the framed search direction                        [80 000 B]
//   spectrum  ny 2 ldc            ny rows of ldc complex values, nx/2 of them used.  ldc = nx/2
//                                 where that is odd, nx/2 + 1 otherwise: the row stride stays odd in
//                                 16-B units, so a wave walking down columns spreads over the
//                                 banks                                               [75 264 B]
//   tables    2 (nx + ny)         every root exp(-2 pi i j/nx), j < nx, and of ny: a mixed stage
//                                 indexes tw[i j n/g] anywhere in the circle, and the symbol's
//                                 cosines are read from it directly                   [3 072 B]
//   perms     (nx/2 + ny + 1)/2   int32: permx, permy                                   [576 B]
//   sums      static, 2 x 3 x (waves) doubles
// staged once per launch from the stepper's device table (host, long double); no sincos here.
//
// Transform.  Length n = r0 r1 ... in FftStages' order (3s, 5s, 4s, then 2: fftpc_mixed.hip says
// why the odd radices come first; the argument is about roundings and holds here).  Forward is
// decimation in frequency: stage t works on groups of g = n/(r0 ... r(t-1)) values, q = g/r apart
// within a butterfly, y_k = W_g^(i k) sum_j W_r^(j k) x[i + j q] stored at i + k q.  Natural order
// in, digit-reversed out: wavenumber p ends at perm[p].  Backward is the same graph reversed with
// conjugate twiddles.  Packing, the Hermitian partner, the symbol and the owners address perm[p]
// directly; nothing is moved to reorder it.  The row pass leaves x-wavenumber k in column permx[k],
// so the column pass, which owns columns by position, needs the inverse: permx's entries carry it
// in their high half.
//
// A wave owns ceil(ny/NW) contiguous rows in the row passes and ceil((nx/2)/NW) columns in the
// column pass; the last working wave fewer, a wave beyond it none (its loops are empty).  A lane
// holds one butterfly, twiddles applied as they are loaded; stages are separated by a wave-local
// fence only.  nx/2 may be odd: k and nx/2 - k are then always distinct.
//
// Index arithmetic.  A stage splits its flat item index into (transform, butterfly) and the
// butterfly into (group, i) -- divisions by n/r, by the wave's column count and by q, none a power
// of two.  They are multiplications by reciprocals: floor(a/d) = umulhi(2a + 1, floor(2^31/d)),
// exact while (2a + 1) d < 2^31 (a < 2^14, d <= 128 here).  The reciprocals of a stage are built on
// the host and passed by value; the one of a wave's column count is formed once per launch.
//
// No block waits for, signals or reads another; every loop is bounded by maxiter, nsteps and the
// transforms' stage counts.
#include <algorithm>
#include <cmath>

#include "shlin_resident_pcm_dev.h"

namespace nk {

namespace {

struct PcmArgs {
  ShLinResidentPcArgs p;
  PcmStages sx, sy;  // rows (length nx/2), columns (length ny)
  int ldc = 0;       // the spectrum's row stride in complex values
  unsigned rpack = 0;  // reciprocal of nx/4 + 1, the pairs (k, nx/2 - k) of a row
};

extern __shared__ __align__(16) double resident_pcm_lds[];

template <int BS, int PPT>
__global__ void __launch_bounds__(BS) shlin_resident_pcm_kernel(PcmArgs Q) {
  constexpr int NW = BS / 64;
  __shared__ double red[2][3][NW];
  static_assert(sizeof(red) <= kStaticBytes, "the footprint check counts the static sums");
  const ShLinResidentPcArgs& P = Q.p;
  const ShLinResidentArgs& A = P.a;
  const int ny = A.ny, nx = A.nx, n = ny * nx, ld = nx + 4, rowspan = ny * ld;
  const int m = nx >> 1, ldc = Q.ldc;
  const int t = threadIdx.x, lane = t & 63;
  // the wave's number in scalar registers: what it owns, its loop bounds and the stage walk are
  // then uniform
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  double* fr = resident_pcm_lds;
  double* Sd = fr + (ny + 4) * ld;  // an even count of doubles: 16-B aligned
  cd* S = reinterpret_cast<cd*>(Sd);
  cd* twx = S + ny * ldc;
  cd* twy = twx + nx;
  int* permx = reinterpret_cast<int*>(twy + ny);
  int* permy = permx + m;
  {
    double* dst = reinterpret_cast<double*>(twx);
    const int nt = 2 * (nx + ny) + ((m + ny + 1) >> 1);
    for (int i = t; i < nt; i += BS) dst[i] = P.tables[i];  // behind the first barrier
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
  G.rnc = recip(max(G.nc, 1));  // the one division of the launch
  G.rpack = Q.rpack;

  const int64_t mb = blockIdx.x;
  const double* Ug = A.U + mb * n;
  const double* Uog = A.Uo + mb * n;
  // the centre coefficient of L, D, the symbol and sigma depend on the member's r and g
  const double rm = A.r ? A.r[mb] : A.r0, gm = A.g ? A.g[mb] : A.g0;
  const double c0 = A.cbase + rm - 1.0, c1 = A.c1, c2 = A.c2, c3 = A.c3;
  const double k = A.k, kh = A.k / 2, gk = gm * A.k;

  int code[PPT];
  double u[PPT], uo[PPT], x[PPT], r[PPT], q[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = t + j * BS;
    // the point code of the plane, and the point's row above it (bits 21-27; 0 for an unused slot)
    code[j] = point_code(i, ny, nx) | ((i < n ? i / nx : 0) << 21);
    u[j] = i < n ? Ug[i] : 0.0;
    uo[j] = i < n ? Uog[i] : 0.0;
    x[j] = r[j] = q[j] = 0.0;
  }
  // a live point's place in the spectrum region, in doubles: row 2 ldc + col, from its frame
  // offset (row + 2) ld + col + 2 and its row
  const int f0 = 2 * ld + 2, dd = ld - 2 * ldc;
  auto spec = [&](int c) { return (c & 0xffff) - (c >> 21) * dd - f0; };

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
      if (act) Sd[spec(c)] = r[j];
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
      apply_M(S, twx, twy, permx, permy, G, Q.sx, Q.sy, sym, lane);
      ++applies;
      double v1[1] = {0.0};
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive) v1[0] += r[j] * Sd[spec(c)];
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
          const double z = Sd[spec(c)];
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
          Sd[spec(c)] = r[j];
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

  double* Un = A.Unew + mb * n;
  double* Up = A.Uprev ? A.Uprev + mb * n : nullptr;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = t + j * BS;
    if (i < n) {
      Un[i] = u[j];
      if (Up) Up[i] = uo[j];
    }
  }
  if (t == 0) {
    A.out[mb] = ShLinResidentOut{iters, steps, relres, status};
    P.out[mb] = ShLinResidentPcOut{applies, sigma};
  }
}

// a side the transforms serve: even, 2^a 3^b 5^c, in [6, 128]
bool mixed_side(int64_t v) {
  if (v < 6 || v > 128 || (v & 1)) return false;
  for (int64_t r : {2, 3, 5})
    while (v % r == 0) v /= r;
  return v == 1;
}

template <int BS, int PPT>
hipError_t launch_variant(const PcmArgs& Q, int64_t batch, hipStream_t s) {
  const size_t lds = shlin_resident_pcm_lds_bytes(Q.p.a.ny, Q.p.a.nx);
  if (lds > 65536) {  // once per variant: whatever shlin_resident_pcm_fits lets through
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&shlin_resident_pcm_kernel<BS, PPT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, int(kLdsBytes - kStaticBytes));
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL((shlin_resident_pcm_kernel<BS, PPT>), dim3(unsigned(batch)), dim3(BS), lds, s,
                     Q);
  return hipGetLastError();
}

}  // namespace

size_t shlin_resident_pcm_lds_bytes(int64_t ny, int64_t nx) {
  return sizeof(double) * (size_t(ny + 4) * size_t(nx + 4) +
                           size_t(ny) * 2 * size_t(spectrum_stride(nx)) +
                           shlin_resident_pcm_table_doubles(ny, nx));
}

bool shlin_resident_pcm_fits(int64_t ny, int64_t nx) {
  auto pow2 = [](int64_t v) { return (v & (v - 1)) == 0; };
  if (!mixed_side(ny) || !mixed_side(nx) || (pow2(ny) && pow2(nx)) ||
      ny * nx > kShLinResidentPcMixedMaxPoints)
    return false;
  if (fftpc_stages_of(int(ny)).ns > kMaxStages || fftpc_stages_of(int(nx / 2)).ns > kMaxStages)
    return false;
  return shlin_resident_pcm_lds_bytes(ny, nx) + kStaticBytes <= kLdsBytes;
}

size_t shlin_resident_pcm_table_doubles(int64_t ny, int64_t nx) {
  return size_t(2 * (nx + ny)) + size_t(nx / 2 + ny + 1) / 2;
}

void shlin_resident_pcm_tables(int64_t ny, int64_t nx, double* out) {
  const int m = int(nx / 2);
  std::fill(out, out + shlin_resident_pcm_table_doubles(ny, nx), 0.0);
  fftpc_roots(nx, out);
  fftpc_roots(ny, out + 2 * nx);
  int32_t* perm = reinterpret_cast<int32_t*>(out + 2 * (nx + ny));
  fftpc_digit_reversal(fftpc_stages_of(m), perm);
  fftpc_digit_reversal(fftpc_stages_of(int(ny)), perm + m);
  for (int k = 0; k < m; ++k) perm[perm[k] & 0xffff] |= k << 16;  // the inverse, in the high half
}

hipError_t shlin_resident_pcm_launch(const ShLinResidentPcArgs& P, int64_t batch, hipStream_t s) {
  if (!shlin_resident_pcm_fits(P.a.ny, P.a.nx) || batch < 1 || batch > 0x7fffffff || !P.tables ||
      !P.out)
    return hipErrorInvalidValue;
  PcmArgs Q;
  Q.p = P;
  Q.sx = walk_of(P.a.nx / 2);
  Q.sy = walk_of(P.a.ny);
  Q.ldc = spectrum_stride(P.a.nx);
  Q.rpack = recip(P.a.nx / 4 + 1);
  const int n = P.a.ny * P.a.nx;
  // the shapes of the other two resident kernels: four waves for few points, four points per
  // thread up to 4096, and at the cap eight waves of eighteen points, the plain kernel's
  if (n <= 1024) return launch_variant<256, 4>(Q, batch, s);
  if (n <= 4096) return launch_variant<1024, 4>(Q, batch, s);
  static_assert(512 * 18 >= kShLinResidentPcMixedMaxPoints, "every point under the cap needs an owner");
  return launch_variant<512, 18>(Q, batch, s);
}

}  // namespace nk
