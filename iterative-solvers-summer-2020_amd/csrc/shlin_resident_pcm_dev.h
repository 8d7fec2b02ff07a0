// The spectral preconditioner on grids whose sides are 2^a 3^b 5^c, applied inside a resident
// workgroup by wave-local mixed-radix transforms: what shlin_resident_pcm.hip (the semi-implicit
// step) and sh_resident_pcm.hip (the implicit Newton-CG step) share.  shlin_resident_pcm.hip's
// header has the LDS map, the transform and the index arithmetic; the code below is that file's,
// moved here as it was.
#pragma once

#include "fftpc.h"
#include "fftpc_dev.h"
#include "shlin_resident_dev.h"

namespace nk {

namespace {

constexpr int kMaxStages = 4;          // 2 3^4 = 162 > 128: no length here has five
constexpr size_t kLdsBytes = 163840;   // a gfx950 workgroup's
constexpr size_t kStaticBytes = 768;   // the sums of the widest shape: 2 x 3 x 16 doubles

// One transform's stages as the kernel walks them, reciprocals included (see the header).
struct PcmStages {
  int n = 0, ns = 0;
  int radix[kMaxStages] = {}, q[kMaxStages] = {}, per[kMaxStages] = {}, tstep[kMaxStages] = {};
  unsigned rq[kMaxStages] = {}, rper[kMaxStages] = {};
};

constexpr unsigned recip(int d) { return (1u << 31) / unsigned(d); }
// floor(a / d) for 0 <= a < 2^14 and the reciprocal of d <= 128
__device__ __forceinline__ int qdiv(int a, unsigned rd) {
  return int(__umulhi(2u * unsigned(a) + 1u, rd));
}

// Orders a wave's LDS accesses across a stage boundary: the hardware runs them in program order,
// the fences keep the compiler from moving them.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One radix-R stage of nb transforms by one wave, in place: transform b starts at base + b ts, its
// element j is at + j es; groups of q R values.  tw[j] for every j the stage reaches (step already
// holds the table's stride).  BFast: the lanes run over the transforms first (columns: neighbouring
// lanes touch neighbouring addresses), else over a transform's butterflies first (rows).
template <int R, bool Inv, bool BFast>
__device__ __forceinline__ void wave_stage(cd* base, int nb, unsigned rnb, int ts, int es, int q,
                                           unsigned rq, int per, unsigned rper, int step,
                                           const cd* tw, int lane) {
  const int total = nb * per, qe = q * es;
#pragma nounroll
  for (int idx = lane; idx < total; idx += 64) {
    int b, rr;
    if (BFast) {
      rr = qdiv(idx, rnb);
      b = idx - rr * nb;
    } else {
      b = qdiv(idx, rper);
      rr = idx - b * per;
    }
    const int i = rr - qdiv(rr, rq) * q;  // rr = group q + i; the butterfly starts at group q R + i
    cd* e = base + b * ts + (rr * R - i * (R - 1)) * es;
    const int wi = i * step;
    cd x[R];
#pragma unroll
    for (int j = 0; j < R; ++j) x[j] = e[j * qe];
    if (Inv) {
#pragma unroll
      for (int j = 1; j < R; ++j) x[j] = cmulc(x[j], tw[j * wi]);  // i j < q R: inside the table
    }
    dft<R, Inv>(x);
    if (!Inv) {
#pragma unroll
      for (int j = 1; j < R; ++j) x[j] = cmul(x[j], tw[j * wi]);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) e[j * qe] = x[j];
  }
  wave_sync();
}

// nb transforms by one wave (nb = 0: the stages with empty loops).  Forward: natural order in,
// digit-reversed out.  Inv: digit-reversed in, natural out, n times the inverse transform.
template <bool Inv, bool BFast>
__device__ __forceinline__ void wave_mfft(cd* base, int nb, unsigned rnb, int ts, int es,
                                          const PcmStages& st, const cd* tw, int tws, int lane) {
  for (int k = 0; k < st.ns; ++k) {
    const int t = Inv ? st.ns - 1 - k : k;
    const int q = st.q[t], per = st.per[t], step = st.tstep[t] * tws;
    const unsigned rq = st.rq[t], rper = st.rper[t];
    switch (st.radix[t]) {
      case 3: wave_stage<3, Inv, BFast>(base, nb, rnb, ts, es, q, rq, per, rper, step, tw, lane); break;
      case 5: wave_stage<5, Inv, BFast>(base, nb, rnb, ts, es, q, rq, per, rper, step, tw, lane); break;
      case 4: wave_stage<4, Inv, BFast>(base, nb, rnb, ts, es, q, rq, per, rper, step, tw, lane); break;
      default: wave_stage<2, Inv, BFast>(base, nb, rnb, ts, es, q, rq, per, rper, step, tw, lane); break;
    }
  }
}

// What a wave owns in the transform: nr rows from row0, nc columns from col0 (either may be 0).
struct PcmShare {
  int ny, m, ldc;  // m = nx/2
  int row0, nr, col0, nc;
  unsigned rnc, rpack;  // reciprocals of max(nc, 1) and of m/2 + 1
};

// z = M res in place in the spectrum region S: in, the residual's rows behind a block barrier;
// out, z behind one.
__device__ __forceinline__ void apply_M(cd* S, const cd* twx, const cd* twy, const int* permx,
                                        const int* permy, const PcmShare& G, const PcmStages& sx,
                                        const PcmStages& sy, const Symbol& sym, int lane) {
  const int ny = G.ny, m = G.m, ldc = G.ldc, hy = ny >> 1;
  cd* rows = S + G.row0 * ldc;
  cd* cols = S + G.col0;
  const int pairs = (m >> 1) + 1;  // k = 0 .. floor(m/2), each with its partner m - k
  const int row_items = G.nr * pairs;

  // rows, real to complex.  A row x[0..nx) is z[j] = x[2j] + i x[2j+1]; X[k] = E[k] + w^k O[k]
  // with E[k] = (Z[k] + conj Z[m-k])/2, O[k] = (Z[k] - conj Z[m-k])/(2i), w = exp(-2 pi i/nx).
  // The pair is read from and written to the positions permx[k], permx[m-k].
  wave_mfft<false, false>(rows, G.nr, 0u, ldc, 1, sx, twx, 2, lane);
#pragma nounroll
  for (int idx = lane; idx < row_items; idx += 64) {
    const int b = qdiv(idx, G.rpack), k = idx - b * pairs;
    cd* z = rows + b * ldc;
    if (k == 0) {
      const cd z0 = z[0];
      z[0] = cd{z0.x + z0.y, z0.x - z0.y};  // (X[0], X[m])
      continue;
    }
    const int mk = m - k;  // != k for every k when m is odd
    const int ik = permx[k] & 0xffff, im = permx[mk] & 0xffff;
    const cd zk = z[ik], zm = z[im];
    const cd E = cd{0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y)};
    const cd D = cd{0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y)};  // (Z[k] - conj Z[m-k]) / 2
    const cd wO = cmul(cd{D.y, -D.x}, twx[k]);
    z[ik] = cadd(E, wO);
    if (mk != k) {  // X[m-k] = conj(E[k] - w^k O[k])
      const cd c = csub(E, wO);
      z[im] = cd{c.x, -c.y};
    }
  }
  __syncthreads();  // rows -> columns

  wave_mfft<false, true>(cols, G.nc, G.rnc, 1, ldc, sy, twy, 1, lane);
  if (G.nc > 0 && G.col0 == 0) {  // column 0 = (DC column) + i (Nyquist column)
    for (int p = lane; p <= hy; p += 64) {
      const int pm = p ? ny - p : 0;
      const int i = permy[p] * ldc, im = permy[pm] * ldc;
      const cd a = S[i], b = S[im];
      const double cp = twy[p].x;
      const double s0 = sym(cp, 1.0), s1 = sym(cp, -1.0);
      // A[p] = (Y[p] + conj Y[pm])/2, i B[p] = (Y[p] - conj Y[pm])/2, each times its own symbol
      const cd A = cd{0.5 * (a.x + b.x), 0.5 * (a.y - b.y)};
      const cd iB = cd{0.5 * (a.x - b.x), 0.5 * (a.y + b.y)};
      S[i] = cd{s0 * A.x + s1 * iB.x, s0 * A.y + s1 * iB.y};
      // A[pm] = conj A[p], i B[pm] = -conj(i B[p])
      if (pm != p) S[im] = cd{s0 * A.x - s1 * iB.x, s1 * iB.y - s0 * A.y};
    }
  }
  // every other column, by y-wavenumber: the value is in row permy[p]; the column at position c
  // holds the x-wavenumber permx[c] >> 16
  const int col_items = G.nc * ny;
#pragma nounroll
  for (int idx = lane; idx < col_items; idx += 64) {
    const int p = qdiv(idx, G.rnc), c = G.col0 + idx - p * G.nc;
    if (c == 0) continue;
    const double sv = sym(twy[p].x, twx[permx[c] >> 16].x);
    cd* e = S + permy[p] * ldc + c;
    const cd y = *e;
    *e = cd{y.x * sv, y.y * sv};
  }
  wave_sync();
  wave_mfft<true, true>(cols, G.nc, G.rnc, 1, ldc, sy, twy, 1, lane);
  __syncthreads();  // columns -> rows

  // rows, complex to real (factors of 2 left to the symbol): Z[k] = E + i O with
  // E = X[k] + conj X[m-k], O = conj(w^k) (X[k] - conj X[m-k])
#pragma nounroll
  for (int idx = lane; idx < row_items; idx += 64) {
    const int b = qdiv(idx, G.rpack), k = idx - b * pairs;
    cd* z = rows + b * ldc;
    if (k == 0) {
      const cd x0 = z[0];
      z[0] = cd{x0.x + x0.y, x0.x - x0.y};
      continue;
    }
    const int mk = m - k;
    const int ik = permx[k] & 0xffff, im = permx[mk] & 0xffff;
    const cd xk = z[ik], xm = z[im];
    const cd E = cd{xk.x + xm.x, xk.y - xm.y};
    const cd O = cmulc(cd{xk.x - xm.x, xk.y + xm.y}, twx[k]);
    z[ik] = cd{E.x - O.y, E.y + O.x};
    if (mk != k) z[im] = cd{E.x + O.y, O.x - E.y};  // conj(E) + i conj(O)
  }
  wave_sync();
  wave_mfft<true, false>(rows, G.nr, 0u, ldc, 1, sx, twx, 2, lane);
  __syncthreads();  // rows -> owners
}

// host: the spectrum's row stride in complex values, and a length's stage walk
inline int spectrum_stride(int64_t nx) { return int(nx / 2) | 1; }  // nx/2 if odd, else nx/2 + 1

inline PcmStages walk_of(int n) {
  const FftStages f = fftpc_stages_of(n);
  PcmStages st;
  st.n = n;
  st.ns = f.ns;
  int g = n;
  for (int t = 0; t < f.ns && t < kMaxStages; ++t) {
    const int r = f.radix[t];
    st.radix[t] = r;
    st.q[t] = g / r;
    st.per[t] = n / r;
    st.tstep[t] = n / g;
    st.rq[t] = recip(st.q[t]);
    st.rper[t] = recip(st.per[t]);
    g /= r;
  }
  return st;
}

}  // namespace

}  // namespace nk
