// The spectral preconditioner applied inside a resident workgroup: what shlin_resident_pc.hip (the
// semi-implicit step) and sh_resident.hip (the implicit Newton-CG step) share.
//
// z = M res with M = (ik I - L/2)^-1 scale' (the Symbol carries ik and the scale): a 2-D real FFT,
// the symbol and the FFT back, in an LDS region of ny rows of nx/2 + 1 complex values -- the
// residual in natural layout, then its packed half spectrum (fftpc.hip's: a row of nx reals is
// nx/2 complex values, X[0] and X[nx/2] share entry 0), then z.  The one value of padding per row
// makes the row stride odd in 16-B units, so that a wave walking down columns spreads over the
// banks.  Behind the region: exp(-2 pi i j/nx), j < nx/2, and exp(-2 pi i j/ny), j < ny/2, staged
// once per launch from the stepper's device table (twiddles and the symbol's cosines, no sincos on
// the device).
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
// Block barriers per application of M: four, one at each change of ownership -- registers to rows
// (the caller's: the residual's rows are stored before a block sum), rows to columns, columns to
// rows, rows to owners.
#pragma once

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

// Wave w's share in a block of NW waves (a power of two); lx = log2 nx, ly = log2 ny.
template <int NW>
__device__ __forceinline__ PcShare pc_share(int w, int lx, int ly) {
  static_assert(NW == 4 || NW == 8 || NW == 16, "waves per block: a power of two");
  constexpr int LNW = NW == 4 ? 2 : (NW == 8 ? 3 : 4);
  const int ny = 1 << ly, n2 = 1 << (lx - 1);
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
  return G;
}

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

// LDS of a preconditioned resident block (bytes): the framed plane, the spectrum region, the tables
inline size_t resident_pc_lds_bytes(int ny, int nx) {
  return sizeof(double) * (size_t(ny + 4) * size_t(nx + 4) + size_t(ny) * size_t(nx + 2) +
                           size_t(nx + ny));
}

}  // namespace

}  // namespace nk
