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
// Transforms are short (4..64 complex values per row, 8..128 per column), so a transform never
// leaves a wave: wave w owns ny / NW whole rows in the row passes and (nx/2) / NW whole columns in
// the column pass, a lane takes radix-4 butterflies (one radix-2 stage where the length is an odd
// power of two), and the stages of a pass are separated by a wave-local fence only -- LDS
// executes a wave's accesses in order.  Decimation in frequency forward (natural in,
// bit-reversed out), decimation in time backward; everything between the two addresses the
// bit-reversed positions, and it does so in place: the row pass leaves X[k] at position brev(k) of
// its row, the column pass wavenumber p in row brev(p), so no value is ever moved to reorder it.
// Column 0 carries the DC and Nyquist columns as one complex column; they are separated by their
// Hermitian symmetry before the symbol, as in fftpc_cols.  The 1/(nx ny) is folded into the symbol.
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

#include "fftpc_dev.h"
#include "shlin_resident_dev.h"

namespace nk {

namespace {

__device__ __forceinline__ int brev(int k, int L) { return int(__brev(unsigned(k)) >> (32 - L)); }

// Orders a wave's LDS accesses across a stage boundary: the hardware runs them in program order,
// the fences keep the compiler from moving them.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 2^lnb transforms of length N = 2^L (L >= 2) by one wave, in place: transform b starts at
// base + b ts, its element j is at + j es.  tw[j tws] = exp(-2 pi i j / N), j < N/2.  BFast: the
// lanes of a butterfly index run over the transforms first (columns: neighbouring lanes touch
// neighbouring addresses), else over a transform's butterflies first (rows).  `on` false: a wave
// without work walks the stages with empty loops.
template <bool BFast>
__device__ __forceinline__ void wave_fft_fwd(cd* base, int L, int lnb, int ts, int es,
                                             const cd* tw, int tws, int lane, bool on) {
  const int N = 1 << L, nbm = (1 << lnb) - 1;
  const int total = on ? 1 << (lnb + L - 2) : 0;
  int s = L;  // the groups still to split have 2^s elements
  while (s >= 2) {
    const int q = 1 << (s - 2), st = (N >> s) * tws, qe = q * es;
#pragma nounroll
    for (int idx = lane; idx < total; idx += 64) {
      const int b = BFast ? idx & nbm : idx >> (L - 2);
      const int rr = BFast ? idx >> lnb : idx & ((N >> 2) - 1);
      const int i = rr & (q - 1), g = rr >> (s - 2);
      cd* e = base + b * ts + ((g << s) + i) * es;
      const cd x0 = e[0], x1 = e[qe], x2 = e[2 * qe], x3 = e[3 * qe];
      const cd wA = tw[i * st], wB = tw[2 * i * st];
      // half size 2q: pairs (0, 2), (1, 3); the second pair's twiddle is wA * (-i)
      const cd a0 = cadd(x0, x2), a1 = cadd(x1, x3);
      const cd a2 = cmul(csub(x0, x2), wA);
      const cd t = csub(x1, x3);
      const cd a3 = cmul(cd{t.y, -t.x}, wA);
      // half size q: pairs (0, 1), (2, 3)
      e[0] = cadd(a0, a1);
      e[qe] = cmul(csub(a0, a1), wB);
      e[2 * qe] = cadd(a2, a3);
      e[3 * qe] = cmul(csub(a2, a3), wB);
    }
    wave_sync();
    s -= 2;
  }
  if (s == 1) {
#pragma nounroll
    for (int idx = lane; idx < 2 * total; idx += 64) {
      const int b = BFast ? idx & nbm : idx >> (L - 1);
      const int j = BFast ? idx >> lnb : idx & ((N >> 1) - 1);
      cd* e = base + b * ts + 2 * j * es;
      const cd x0 = e[0], x1 = e[es];
      e[0] = cadd(x0, x1);
      e[es] = csub(x0, x1);
    }
    wave_sync();
  }
}

// The flow graph above backwards with conjugate twiddles: bit-reversed in, natural out, N times
// the inverse transform.
template <bool BFast>
__device__ __forceinline__ void wave_fft_inv(cd* base, int L, int lnb, int ts, int es,
                                             const cd* tw, int tws, int lane, bool on) {
  const int N = 1 << L, nbm = (1 << lnb) - 1;
  const int total = on ? 1 << (lnb + L - 2) : 0;
  int s = 0;  // the groups already merged have 2^s elements
  if (L & 1) {
#pragma nounroll
    for (int idx = lane; idx < 2 * total; idx += 64) {
      const int b = BFast ? idx & nbm : idx >> (L - 1);
      const int j = BFast ? idx >> lnb : idx & ((N >> 1) - 1);
      cd* e = base + b * ts + 2 * j * es;
      const cd x0 = e[0], x1 = e[es];
      e[0] = cadd(x0, x1);
      e[es] = csub(x0, x1);
    }
    wave_sync();
    s = 1;
  }
  while (s < L) {
    const int q = 1 << s, st = (N >> (s + 2)) * tws, qe = q * es;
#pragma nounroll
    for (int idx = lane; idx < total; idx += 64) {
      const int b = BFast ? idx & nbm : idx >> (L - 2);
      const int rr = BFast ? idx >> lnb : idx & ((N >> 2) - 1);
      const int i = rr & (q - 1), g = rr >> s;
      cd* e = base + b * ts + ((g << (s + 2)) + i) * es;
      const cd x0 = e[0], x1 = e[qe], x2 = e[2 * qe], x3 = e[3 * qe];
      const cd wA = tw[i * st], wB = tw[2 * i * st];
      const cd t1 = cmulc(x1, wB), t3 = cmulc(x3, wB);
      const cd a0 = cadd(x0, t1), a1 = csub(x0, t1);
      const cd a2 = cadd(x2, t3), a3 = csub(x2, t3);
      const cd t2 = cmulc(a2, wA);
      const cd u = cmulc(a3, wA);
      const cd v = cd{-u.y, u.x};  // the second pair's twiddle is conj(wA * (-i))
      e[0] = cadd(a0, t2);
      e[qe] = cadd(a1, v);
      e[2 * qe] = csub(a0, t2);
      e[3 * qe] = csub(a1, v);
    }
    wave_sync();
    s += 2;
  }
}

// What a wave owns in the transform: 2^lrw rows from row0, 2^lcw columns from col0.
struct PcShare {
  int ly, lx2, ldc;  // log2 ny, log2 (nx/2), the row stride in complex values (nx/2 + 1)
  int lrw, row0, lcw, col0;
  bool row_on, col_on;
};

// z = M res in place in the spectrum region S: in, the residual's rows behind a block barrier;
// out, z behind one.
__device__ __forceinline__ void apply_M(cd* S, const cd* twx, const cd* twy, const PcShare& G,
                                        const Symbol& sym, int lane) {
  const int ly = G.ly, lx2 = G.lx2, ldc = G.ldc, ny = 1 << ly, n2 = 1 << lx2, hy = ny >> 1;
  cd* rows = S + G.row0 * ldc;
  cd* cols = S + G.col0;
  const int row_items = G.row_on ? 1 << (G.lrw + lx2 - 1) : 0;  // n2/2 per row

  // rows, real to complex.  A row x[0..nx) is z[j] = x[2j] + i x[2j+1]; X[k] = E[k] + w^k O[k]
  // with E[k] = (Z[k] + conj Z[n2-k])/2, O[k] = (Z[k] - conj Z[n2-k])/(2i), w = exp(-2 pi i/nx).
  // The pair (k, n2 - k) is read from and written to the positions brev(k), brev(n2 - k).
  wave_fft_fwd<false>(rows, lx2, G.lrw, ldc, 1, twx, 2, lane, G.row_on);
#pragma nounroll
  for (int idx = lane; idx < row_items; idx += 64) {
    const int b = idx >> (lx2 - 1), j = idx & ((n2 >> 1) - 1);
    cd* z = rows + b * ldc;
    if (j == 0) {  // this item takes k = 0 beside the self-paired k = n2/2
      const cd z0 = z[0];
      z[0] = cd{z0.x + z0.y, z0.x - z0.y};  // (X[0], X[n2])
    }
    const int k = j ? j : n2 >> 1, m = n2 - k;
    const int ik = brev(k, lx2), im = brev(m, lx2);
    const cd zk = z[ik], zm = z[im];
    const cd E = cd{0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y)};
    const cd D = cd{0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y)};  // (Z[k] - conj Z[m]) / 2
    const cd wO = cmul(cd{D.y, -D.x}, twx[k]);
    z[ik] = cadd(E, wO);
    if (m != k) {  // X[n2-k] = conj(E[k] - w^k O[k])
      const cd c = csub(E, wO);
      z[im] = cd{c.x, -c.y};
    }
  }
  __syncthreads();  // rows -> columns

  wave_fft_fwd<true>(cols, ly, G.lcw, 1, ldc, twy, 1, lane, G.col_on);
  auto cosy = [&](int p) -> double {
    return p < hy ? twy[p].x : (p == hy ? -1.0 : twy[ny - p].x);
  };
  if (G.col_on && G.col0 == 0) {  // column 0 = (DC column) + i (Nyquist column)
    for (int p = lane; p <= hy; p += 64) {
      const int m = (ny - p) & (ny - 1);
      const int i = brev(p, ly) * ldc, im = brev(m, ly) * ldc;
      const cd a = S[i], b = S[im];
      const double cp = cosy(p);
      const double s0 = sym(cp, 1.0), s1 = sym(cp, -1.0);
      // A[p] = (Y[p] + conj Y[m])/2, i B[p] = (Y[p] - conj Y[m])/2, each times its own symbol
      const cd A = cd{0.5 * (a.x + b.x), 0.5 * (a.y - b.y)};
      const cd iB = cd{0.5 * (a.x - b.x), 0.5 * (a.y + b.y)};
      S[i] = cd{s0 * A.x + s1 * iB.x, s0 * A.y + s1 * iB.y};
      // A[m] = conj A[p], i B[m] = -conj(i B[p])
      if (m != p) S[im] = cd{s0 * A.x - s1 * iB.x, s1 * iB.y - s0 * A.y};
    }
  }
  const int col_items = G.col_on ? 1 << (G.lcw + ly) : 0;
#pragma nounroll
  for (int idx = lane; idx < col_items; idx += 64) {
    const int c = G.col0 + (idx & ((1 << G.lcw) - 1)), i = idx >> G.lcw;
    if (c == 0) continue;
    const double sv = sym(cosy(brev(i, ly)), twx[brev(c, lx2)].x);
    cd* e = S + i * ldc + c;
    const cd y = *e;
    *e = cd{y.x * sv, y.y * sv};
  }
  wave_sync();
  wave_fft_inv<true>(cols, ly, G.lcw, 1, ldc, twy, 1, lane, G.col_on);
  __syncthreads();  // columns -> rows

  // rows, complex to real (factors of 2 left to the symbol): Z[k] = E + i O with
  // E = X[k] + conj X[n2-k], O = conj(w^k) (X[k] - conj X[n2-k])
#pragma nounroll
  for (int idx = lane; idx < row_items; idx += 64) {
    const int b = idx >> (lx2 - 1), j = idx & ((n2 >> 1) - 1);
    cd* z = rows + b * ldc;
    if (j == 0) {
      const cd x0 = z[0];
      z[0] = cd{x0.x + x0.y, x0.x - x0.y};
    }
    const int k = j ? j : n2 >> 1, m = n2 - k;
    const int ik = brev(k, lx2), im = brev(m, lx2);
    const cd xk = z[ik], xm = z[im];
    const cd E = cd{xk.x + xm.x, xk.y - xm.y};
    const cd O = cmulc(cd{xk.x - xm.x, xk.y + xm.y}, twx[k]);
    z[ik] = cd{E.x - O.y, E.y + O.x};
    if (m != k) z[im] = cd{E.x + O.y, O.x - E.y};  // conj(E) + i conj(O)
  }
  wave_sync();
  wave_fft_inv<false>(rows, lx2, G.lrw, ldc, 1, twx, 2, lane, G.row_on);
  __syncthreads();  // rows -> owners
}

extern __shared__ __align__(16) double resident_pc_lds[];

template <int BS, int PPT>
__global__ void __launch_bounds__(BS) shlin_resident_pc_kernel(ShLinResidentPcArgs P) {
  constexpr int NW = BS / 64, LNW = NW == 4 ? 2 : (NW == 8 ? 3 : 4);
  static_assert(NW == 4 || NW == 8 || NW == 16, "waves per block: a power of two");
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
  PcShare G;
  G.ly = ly;
  G.lx2 = lx - 1;
  G.ldc = n2 + 1;
  G.lrw = ny >= NW ? ly - LNW : 0;
  G.row_on = w < ny;
  G.row0 = G.row_on ? w << G.lrw : 0;
  G.lcw = n2 >= NW ? lx - 1 - LNW : 0;
  G.col_on = w < n2;
  G.col0 = G.col_on ? w << G.lcw : 0;

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

size_t pc_lds_bytes(int ny, int nx) {
  return sizeof(double) * (size_t(ny + 4) * size_t(nx + 4) + size_t(ny) * size_t(nx + 2) +
                           size_t(nx + ny));
}

template <int BS, int PPT>
hipError_t launch_variant(const ShLinResidentPcArgs& P, int64_t batch, hipStream_t s) {
  const size_t lds = pc_lds_bytes(P.a.ny, P.a.nx);
  if (lds > 65536) {  // once per variant: the largest footprint under the cap
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&shlin_resident_pc_kernel<BS, PPT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, int(pc_lds_bytes(128, 64)));
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
