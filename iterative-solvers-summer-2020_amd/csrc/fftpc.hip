// Spectral preconditioner z = IFFT2( FFT2(v) / A0^ ) for gfx950 (see fftpc.h), hand-written: no
// FFT library is linked.
//
// Three passes over the data, 48 B per grid point (each reads and writes one vector's worth):
//   1. rows, real to complex: a row of nx reals is transformed as nx/2 complex values in LDS (the
//      even/odd split), and its half spectrum X[0..nx/2] written PACKED into nx/2 complex values:
//      X[0] and X[nx/2] are real and share entry 0 as (X[0], X[nx/2]).  The half spectrum then has
//      exactly the footprint of a real vector (ny * nx doubles).
//   2. columns: a block holds `cols` whole columns in LDS, transforms them forward, multiplies by
//      the symbol and transforms them back -- one read and one write of the half spectrum.  Column
//      0 carries two real columns (DC and Nyquist) as one complex column; their transforms A, B
//      have different symbols S0, S1 and are separated by the Hermitian symmetry of each before
//      the multiply: A[p] = (Y[p] + conj Y[ny-p])/2, i B[p] = (Y[p] - conj Y[ny-p])/2,
//      Y'[p] = S0 A[p] + S1 i B[p].
//   3. rows, complex to real: the inverse of pass 1.
// The 1/(nx ny) of the inverse transforms is folded into the symbol.
//
// Transforms: in-place radix-2 decimation in frequency forward (natural order in, bit-reversed
// out) and decimation in time backward (bit-reversed in, natural out), two radix-2 stages per
// LDS round trip.  Everything between the two (the symbol, the packing) addresses the
// bit-reversed positions directly, so no reordering pass exists.  Twiddles and the symbol's
// cosines come from tables built on the host in long double (one per length); there is no
// sincos on the device.
//
// Column tiles are narrow (2 columns of 4096 rows = 128 KB of LDS, 8 columns up to 512 rows): a
// 4096-long complex column is 64 KB, so the tile's rows are 32..128-B runs of the half spectrum.
// The blocks are numbered so that the ones sharing an L2 (blockIdx % 8) work on neighbouring
// columns, which lets the other half of a 128-B line come from that L2.  Transposed tiles out of
// the row pass would make these runs long, at the cost of short runs in the row passes'
// stores (a row of 4096 is already 32 KB of LDS per row).
//
// Sides of 8192 and 16384 take other kernels, and every grid with both sides <= 4096 launches the
// three above exactly as before.  A column longer than 4096 (256 KB at 16384) does not fit on
// chip: pass 2 becomes three trips over the half spectrum, the column length in two factors
// (fftpc_cols_outer / fftpc_cols_inner below, 80 B per point in all).  A row longer than 4096 is
// 64 or 128 KB of LDS: one row per block of 1024 threads (fftpc_rows_*_long), whose blocks take
// several rows in turn where there are more than 4096, so that a row pass never leaves more than
// 4096 dot partials.
#include "fftpc.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/nkhip.h"
#include "nk_device.h"

namespace nk {

namespace {

using cd = double2;

constexpr int kRowThreads = 256;
constexpr int kColThreadsMax = 1024;
constexpr int kLongThreads = 1024;  // block of the row passes that take several row groups in turn
constexpr int kRowElems = 2048;  // complex values of LDS per block of a row pass (32 KB)

__device__ __forceinline__ cd cadd(cd a, cd b) { return cd{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd csub(cd a, cd b) { return cd{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cd cmul(cd a, cd w) {
  return cd{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x};
}
// a * conj(w)
__device__ __forceinline__ cd cmulc(cd a, cd w) {
  return cd{a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y};
}
__device__ __forceinline__ int brev(int k, int L) { return int(__brev(unsigned(k)) >> (32 - L)); }

// nb transforms of length N = 2^L (>= 2), transform b at buf + b*N, by the whole block.
// tw[j * tws] = exp(-2 pi i j / N) for j < N/2.  Natural order in, bit-reversed order out.
__device__ void fft_fwd(cd* buf, int L, int nb, const cd* __restrict__ tw, int tws) {
  const int N = 1 << L;
  int s = L;  // the groups still to split have 2^s elements
  while (s >= 2) {
    const int q = 1 << (s - 2);
    const int st = (N >> s) * tws;
    const int total = nb << (L - 2);
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int b = idx >> (L - 2), rr = idx & ((N >> 2) - 1);
      const int i = rr & (q - 1), g = rr >> (s - 2);
      cd* e = buf + (b << L) + (g << s) + i;
      const cd x0 = e[0], x1 = e[q], x2 = e[2 * q], x3 = e[3 * q];
      const cd wA = tw[i * st], wB = tw[2 * i * st];
      // half size 2q: pairs (0, 2), (1, 3); the second pair's twiddle is wA * (-i)
      const cd a0 = cadd(x0, x2), a1 = cadd(x1, x3);
      const cd a2 = cmul(csub(x0, x2), wA);
      const cd t = csub(x1, x3);
      const cd a3 = cmul(cd{t.y, -t.x}, wA);
      // half size q: pairs (0, 1), (2, 3)
      e[0] = cadd(a0, a1);
      e[q] = cmul(csub(a0, a1), wB);
      e[2 * q] = cadd(a2, a3);
      e[3 * q] = cmul(csub(a2, a3), wB);
    }
    __syncthreads();
    s -= 2;
  }
  if (s == 1) {
    const int total = nb << (L - 1);
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      cd* e = buf + 2 * idx;
      const cd x0 = e[0], x1 = e[1];
      e[0] = cadd(x0, x1);
      e[1] = csub(x0, x1);
    }
    __syncthreads();
  }
}

// The flow graph of fft_fwd backwards with conjugate twiddles: bit-reversed order in, natural
// order out, N times the inverse transform.
__device__ void fft_inv(cd* buf, int L, int nb, const cd* __restrict__ tw, int tws) {
  const int N = 1 << L;
  int s = 0;  // the groups already merged have 2^s elements
  if (L & 1) {
    const int total = nb << (L - 1);
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      cd* e = buf + 2 * idx;
      const cd x0 = e[0], x1 = e[1];
      e[0] = cadd(x0, x1);
      e[1] = csub(x0, x1);
    }
    __syncthreads();
    s = 1;
  }
  while (s < L) {
    const int q = 1 << s;
    const int st = (N >> (s + 2)) * tws;
    const int total = nb << (L - 2);
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int b = idx >> (L - 2), rr = idx & ((N >> 2) - 1);
      const int i = rr & (q - 1), g = rr >> s;
      cd* e = buf + (b << L) + (g << (s + 2)) + i;
      const cd x0 = e[0], x1 = e[q], x2 = e[2 * q], x3 = e[3 * q];
      const cd wA = tw[i * st], wB = tw[2 * i * st];
      const cd t1 = cmulc(x1, wB), t3 = cmulc(x3, wB);
      const cd a0 = cadd(x0, t1), a1 = csub(x0, t1);
      const cd a2 = cadd(x2, t3), a3 = csub(x2, t3);
      const cd t2 = cmulc(a2, wA);
      const cd u = cmulc(a3, wA);
      const cd v = cd{-u.y, u.x};  // the second pair's twiddle is conj(wA * (-i))
      e[0] = cadd(a0, t2);
      e[q] = cadd(a1, v);
      e[2 * q] = csub(a0, t2);
      e[3 * q] = csub(a1, v);
    }
    __syncthreads();
    s += 2;
  }
}

extern __shared__ double2 fft_lds[];

// Pass 1: `rows` rows per block.  A row x[0..nx) is read as z[j] = x[2j] + i x[2j+1], transformed
// (length n2 = nx/2), and X[k] = E[k] + w^k O[k] (w = exp(-2 pi i/nx), E / O the transforms of the
// even / odd samples, E[k] = (Z[k] + conj Z[n2-k])/2, O[k] = (Z[k] - conj Z[n2-k])/(2i)) written
// for k = 0..n2 in the packed layout.
__device__ __forceinline__ void rows_fwd_body(const double* __restrict__ in, cd* __restrict__ H,
                                              int n2, int lx2, int rows, int64_t row0,
                                              const cd* __restrict__ twx) {
  cd* buf = fft_lds;
  const cd* src = reinterpret_cast<const cd*>(in) + row0 * n2;
  const int total = rows * n2;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) buf[idx] = src[idx];
  __syncthreads();
  fft_fwd(buf, lx2, rows, twx, 2);
  const int per = (n2 >> 1) + 1;  // k = 0 .. n2/2, with its partner n2 - k
  for (int idx = threadIdx.x; idx < rows * per; idx += blockDim.x) {
    const int b = idx / per, k = idx - b * per;
    const cd* z = buf + (b << lx2);
    cd* dst = H + (row0 + b) * n2;
    if (k == 0) {
      const cd z0 = z[0];
      dst[0] = cd{z0.x + z0.y, z0.x - z0.y};  // (X[0], X[n2])
      continue;
    }
    const int m = n2 - k;
    const cd zk = z[brev(k, lx2)], zm = z[brev(m, lx2)];
    const cd E = cd{0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y)};
    const cd D = cd{0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y)};  // (Z[k] - conj Z[m]) / 2
    const cd wO = cmul(cd{D.y, -D.x}, twx[k]);
    dst[k] = cadd(E, wO);
    if (m != k) {  // X[n2-k] = conj(E[k] - w^k O[k])
      const cd c = csub(E, wO);
      dst[m] = cd{c.x, -c.y};
    }
  }
}

__global__ __launch_bounds__(kRowThreads) void fftpc_rows_fwd(const double* __restrict__ in,
                                                              cd* __restrict__ H, int nx, int lx2,
                                                              int rows,
                                                              const cd* __restrict__ twx) {
  rows_fwd_body(in, H, nx >> 1, lx2, rows, int64_t(blockIdx.x) * rows, twx);
}

// Pass 1 for the grids the kernel above does not serve: rows longer than 4096 (one row of nx/2 =
// 4096 or 8192 complex values is 64 or 128 KB of LDS, held by a block of 1024 threads), and
// grids with more than 4096 row groups.  A block takes `iters` consecutive groups of `rows` rows
// in turn, so a row pass never has more than 4096 blocks (fftpc_dot_blocks).
__global__ __launch_bounds__(kLongThreads) void fftpc_rows_fwd_long(const double* __restrict__ in,
                                                                    cd* __restrict__ H, int nx,
                                                                    int lx2, int rows, int iters,
                                                                    const cd* __restrict__ twx) {
  for (int it = 0; it < iters; ++it) {
    rows_fwd_body(in, H, nx >> 1, lx2, rows, (int64_t(blockIdx.x) * iters + it) * rows, twx);
    __syncthreads();  // the next group's loads overwrite the rows just stored from
  }
}

// Pass 3: the inverse of pass 1 (factors of 2 left to the symbol's normalisation): Z[k] = E + i O
// with E = X[k] + conj X[n2-k], O = conj(w^k) (X[k] - conj X[n2-k]); the backward transform of Z
// is nx (x[2j] + i x[2j+1]).  The block's rows are left in fft_lds, row-major, behind a barrier;
// the two kernels below differ only in how they store them.
__device__ __forceinline__ void rows_inv_lds(const cd* __restrict__ H, int n2, int lx2, int rows,
                                             int64_t row0, const cd* __restrict__ twx) {
  cd* buf = fft_lds;
  const int per = (n2 >> 1) + 1;
  for (int idx = threadIdx.x; idx < rows * per; idx += blockDim.x) {
    const int b = idx / per, k = idx - b * per;
    cd* z = buf + (b << lx2);
    const cd* src = H + (row0 + b) * n2;
    if (k == 0) {
      const cd x0 = src[0];
      z[0] = cd{x0.x + x0.y, x0.x - x0.y};
      continue;
    }
    const int m = n2 - k;
    const cd xk = src[k], xm = src[m];
    const cd E = cd{xk.x + xm.x, xk.y - xm.y};
    const cd O = cmulc(cd{xk.x - xm.x, xk.y + xm.y}, twx[k]);
    z[brev(k, lx2)] = cd{E.x - O.y, E.y + O.x};
    if (m != k) z[brev(m, lx2)] = cd{E.x + O.y, O.x - E.y};  // conj(E) + i conj(O)
  }
  __syncthreads();
  fft_inv(buf, lx2, rows, twx, 2);
}

__global__ __launch_bounds__(kRowThreads) void fftpc_rows_inv(const cd* __restrict__ H,
                                                              double* __restrict__ out, int nx,
                                                              int lx2, int rows,
                                                              const cd* __restrict__ twx) {
  const cd* buf = fft_lds;
  const int n2 = nx >> 1;
  const int64_t row0 = int64_t(blockIdx.x) * rows;
  rows_inv_lds(H, n2, lx2, rows, row0, twx);
  cd* dst = reinterpret_cast<cd*>(out) + row0 * n2;
  const int total = rows * n2;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) dst[idx] = buf[idx];
}

// Pass 3 with the dot product w . out: the same pass, and every value about to be stored is also
// multiplied by the matching entry of w; a thread sums its products in store order, the block in
// block_reduce's fixed tree, and partial[blockIdx.x] receives the block's sum (reduce_final then
// adds the blocks in a fixed order: the dot is deterministic).  8 B per point more than the pass
// alone, against 16 for a separate dot pass.  w may be `out` or the vector the application
// started from (each entry is read by the thread that then overwrites it): no __restrict__.
__global__ __launch_bounds__(kRowThreads) void fftpc_rows_inv_dot(const cd* __restrict__ H,
                                                                  double* out, int nx, int lx2,
                                                                  int rows,
                                                                  const cd* __restrict__ twx,
                                                                  const double* w,
                                                                  double* __restrict__ partial) {
  const cd* buf = fft_lds;
  const int n2 = nx >> 1;
  const int64_t row0 = int64_t(blockIdx.x) * rows;
  rows_inv_lds(H, n2, lx2, rows, row0, twx);
  cd* dst = reinterpret_cast<cd*>(out) + row0 * n2;
  const cd* wv = reinterpret_cast<const cd*>(w) + row0 * n2;
  const int total = rows * n2;
  double acc[1] = {0.0};
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const cd zv = buf[idx], ww = wv[idx];
    acc[0] += ww.x * zv.x + ww.y * zv.y;
    dst[idx] = zv;
  }
  const double v = block_reduce<1, 1, kRowThreads>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// Pass 3 for the grids of fftpc_rows_fwd_long, with the dot (Dot) or without it.  A thread adds
// its products in store order across the block's row groups, so the block's partial, and with it
// the dot, stays a fixed-order sum.
template <bool Dot>
__global__ __launch_bounds__(kLongThreads) void fftpc_rows_inv_long(const cd* __restrict__ H,
                                                                    double* out, int nx, int lx2,
                                                                    int rows, int iters,
                                                                    const cd* __restrict__ twx,
                                                                    const double* w,
                                                                    double* __restrict__ partial) {
  const cd* buf = fft_lds;
  const int n2 = nx >> 1;
  const int total = rows * n2;
  double acc[1] = {0.0};
  for (int it = 0; it < iters; ++it) {
    const int64_t row0 = (int64_t(blockIdx.x) * iters + it) * rows;
    rows_inv_lds(H, n2, lx2, rows, row0, twx);
    cd* dst = reinterpret_cast<cd*>(out) + row0 * n2;
    const cd* wv = reinterpret_cast<const cd*>(w) + row0 * n2;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const cd zv = buf[idx];
      if (Dot) {
        const cd ww = wv[idx];
        acc[0] += ww.x * zv.x + ww.y * zv.y;
      }
      dst[idx] = zv;
    }
    __syncthreads();  // the next group's loads overwrite the rows just stored from
  }
  if (Dot) {
    const double v = block_reduce<1, 1, kLongThreads>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
  }
}

struct Symbol {
  double ih2, r, ik, scale;
  // scale / A0^ from the two cosines
  __device__ double operator()(double cp, double cq) const {
    const double s = (2.0 * cp + 2.0 * cq - 4.0) * ih2;
    const double lh = -s * s - 2.0 * s + (r - 1.0);
    return scale / (ik - 0.5 * lh);
  }
};

// Pass 2: `cols` = 2^lc whole columns per block, in place on the packed half spectrum.
__global__ __launch_bounds__(kColThreadsMax) void fftpc_cols(cd* __restrict__ H, int ny, int n2,
                                                              int ly, int lc,
                                                              const cd* __restrict__ twy,
                                                              const cd* __restrict__ twx,
                                                              Symbol sym) {
  cd* buf = fft_lds;
  const int cols = 1 << lc;
  // blocks that share an L2 (blockIdx % 8) take neighbouring column tiles
  int blk = blockIdx.x;
  const int nblk = gridDim.x;
  if ((nblk & 7) == 0) blk = (blk & 7) * (nblk >> 3) + (blk >> 3);
  const int c0 = blk * cols;
  const int total = ny << lc;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int p = idx >> lc, c = idx & (cols - 1);
    buf[(c << ly) + p] = H[int64_t(p) * n2 + c0 + c];
  }
  __syncthreads();
  fft_fwd(buf, ly, cols, twy, 1);
  const int hy = ny >> 1;
  auto cosy = [&](int p) -> double {
    return p < hy ? twy[p].x : (p == hy ? -1.0 : twy[ny - p].x);
  };
  if (c0 == 0) {  // column 0 = (DC column) + i (Nyquist column)
    for (int p = threadIdx.x; p <= hy; p += blockDim.x) {
      const int m = (ny - p) & (ny - 1);
      const int i = brev(p, ly), im = brev(m, ly);
      const cd a = buf[i], b = buf[im];
      const double cp = cosy(p);
      const double s0 = sym(cp, 1.0), s1 = sym(cp, -1.0);
      // unpacked first: A[p] = (Y[p] + conj Y[m])/2, i B[p] = (Y[p] - conj Y[m])/2.  (The symbols
      // differ by up to cond(A0): combining them first, (s0+s1)/2 and (s0-s1)/2, would cancel.)
      const cd A = cd{0.5 * (a.x + b.x), 0.5 * (a.y - b.y)};
      const cd iB = cd{0.5 * (a.x - b.x), 0.5 * (a.y + b.y)};
      buf[i] = cd{s0 * A.x + s1 * iB.x, s0 * A.y + s1 * iB.y};
      // A[m] = conj A[p], i B[m] = -conj(i B[p])
      if (m != p) buf[im] = cd{s0 * A.x - s1 * iB.x, s1 * iB.y - s0 * A.y};
    }
  }
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int c = idx >> ly, i = idx & (ny - 1);
    const int q = c0 + c;
    if (q == 0) continue;
    const double sv = sym(cosy(brev(i, ly)), twx[q].x);
    const cd y = buf[idx];
    buf[idx] = cd{y.x * sv, y.y * sv};
  }
  __syncthreads();
  fft_inv(buf, ly, cols, twy, 1);
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int p = idx >> lc, c = idx & (cols - 1);
    H[int64_t(p) * n2 + c0 + c] = buf[(c << ly) + p];
  }
}

// ---- Columns too long for one block's LDS (ny > the plan's split length; 8192 and 16384 always).
// The four-step form with ny = f1 * f2, row j = j1 f2 + j2, wavenumber p = k1 + f1 k2:
//   Y[p] = sum_j2 W_f2^(j2 k2) [ W_ny^(k1 j2) sum_j1 W_f1^(j1 k1) x[j1 f2 + j2] ]
// in three trips over the half spectrum, all in place:
//   A. fftpc_cols_outer<false>: per j2, the f1-long transform of the stride-f2 sub-column, times
//      the inter-factor twiddle W_ny^(k1 j2).  fft_fwd leaves k1 at position brev(k1) of the
//      sub-column, i.e. in row brev(k1) f2 + j2: no reordering pass here either.
//   B. fftpc_cols_inner: per k1, the f2-long transform of the f2 consecutive rows brev(k1) f2 + j2,
//      the symbol at p = k1 + f1 k2, and the transform back.
//   C. fftpc_cols_outer<true>: A backwards (conjugate twiddle, then the f1-long inverse).
// 80 B per grid point with the two row passes instead of 48.  A tile holds only f1 (A, C) or
// 2 f2 (B) values per column, so it is wide: 64 KB of LDS is 32 columns = 512-B runs of the half
// spectrum at f1 = 128, and 16 columns = 256-B runs at f2 = 128 in B.
// The length-f1 and length-f2 twiddles are strided reads of twy (strides f2 and f1), the
// inter-factor twiddle is twy[m] or -twy[m - ny/2].

// blocks that share an L2 (blockIdx % 8) take neighbouring tiles, as in fftpc_cols
__device__ __forceinline__ int l2_block_order() {
  int blk = blockIdx.x;
  const int nblk = gridDim.x;
  if ((nblk & 7) == 0) blk = (blk & 7) * (nblk >> 3) + (blk >> 3);
  return blk;
}

// Trips A (Inv = false) and C (Inv = true): block (j2, column tile of 2^lw), hw = nx/2 columns.
template <bool Inv>
__global__ __launch_bounds__(kColThreadsMax) void fftpc_cols_outer(cd* __restrict__ H, int hw,
                                                                    int l1, int l2, int lw,
                                                                    const cd* __restrict__ twy) {
  cd* buf = fft_lds;
  const int f1 = 1 << l1, f2 = 1 << l2, W = 1 << lw;
  const int hy = (f1 >> 1) << l2;  // ny / 2
  const int blk = l2_block_order();
  const int ntile = hw >> lw;
  const int tile = blk & (ntile - 1), j2 = blk / ntile;
  cd* base = H + int64_t(j2) * hw + (tile << lw);
  const int64_t rs = int64_t(f2) * hw;  // from one row of the sub-column to the next
  const int total = f1 << lw;
  // exp(-2 pi i k1 j2 / ny), k1 j2 < ny
  auto twid = [&](int m) -> cd {
    if (m < hy) return twy[m];
    const cd t = twy[m - hy];
    return cd{-t.x, -t.y};
  };
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int r = idx >> lw, c = idx & (W - 1);
    const cd v = base[r * rs + c];
    buf[(c << l1) + r] = Inv ? cmulc(v, twid(brev(r, l1) * j2)) : v;
  }
  __syncthreads();
  if (Inv)
    fft_inv(buf, l1, W, twy, f2);
  else
    fft_fwd(buf, l1, W, twy, f2);
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int r = idx >> lw, c = idx & (W - 1);
    const cd v = buf[(c << l1) + r];
    base[r * rs + c] = Inv ? v : cmul(v, twid(brev(r, l1) * j2));
  }
}

// Trip B: block (pair of k1 groups, column tile of 2^lw).  Wavenumber p = k1 + f1 k2 has its
// Hermitian partner ny - p in group f1 - k1 (mod f1), which column 0's unpacking needs beside it:
// a block holds the two groups {k1, f1 - k1}, or {0, f1/2}, which are their own partners.
__global__ __launch_bounds__(kColThreadsMax) void fftpc_cols_inner(cd* __restrict__ H, int hw,
                                                                    int l1, int l2, int lw,
                                                                    const cd* __restrict__ twy,
                                                                    const cd* __restrict__ twx,
                                                                    Symbol sym) {
  cd* buf = fft_lds;
  const int f1 = 1 << l1, f2 = 1 << l2, W = 1 << lw;
  const int ny = f1 << l2, hy = ny >> 1;
  const int blk = l2_block_order();
  const int ntile = hw >> lw;
  const int tile = blk & (ntile - 1), pr = blk / ntile;  // pr < f1/2
  const int c0 = tile << lw;
  const int ka = pr, kb = pr ? f1 - pr : f1 >> 1;
  const int64_t rowa = int64_t(brev(ka, l1)) << l2, rowb = int64_t(brev(kb, l1)) << l2;
  const int total = f2 << (lw + 1);
  // buf[(((g << lw) + c) << l2) + j2]: group g, column c of the tile, row j2 of the group
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int c = idx & (W - 1), t = idx >> lw;
    const int j2 = t & (f2 - 1), g = t >> l2;
    buf[(((g << lw) + c) << l2) + j2] = H[((g ? rowb : rowa) + j2) * hw + c0 + c];
  }
  __syncthreads();
  fft_fwd(buf, l2, 2 * W, twy, f1);
  auto cosy = [&](int p) -> double {
    return p < hy ? twy[p].x : (p == hy ? -1.0 : twy[ny - p].x);
  };
  if (c0 == 0) {  // column 0 = (DC column) + i (Nyquist column), unpacked as in fftpc_cols
    for (int idx = threadIdx.x; idx < 2 * f2; idx += blockDim.x) {
      const int g = idx >> l2, i0 = idx & (f2 - 1);
      const int p = (g ? kb : ka) + (brev(i0, l2) << l1);
      const int m = (ny - p) & (ny - 1);
      if (p > m) continue;  // each pair once, by its smaller wavenumber
      const int gm = (m & (f1 - 1)) == ka ? 0 : 1;
      const int i = (g << (lw + l2)) + i0, im = (gm << (lw + l2)) + brev(m >> l1, l2);
      const cd a = buf[i], b = buf[im];
      const double cp = cosy(p);
      const double s0 = sym(cp, 1.0), s1 = sym(cp, -1.0);
      const cd A = cd{0.5 * (a.x + b.x), 0.5 * (a.y - b.y)};
      const cd iB = cd{0.5 * (a.x - b.x), 0.5 * (a.y + b.y)};
      buf[i] = cd{s0 * A.x + s1 * iB.x, s0 * A.y + s1 * iB.y};
      if (m != p) buf[im] = cd{s0 * A.x - s1 * iB.x, s1 * iB.y - s0 * A.y};
    }
  }
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int i = idx & (f2 - 1), t = idx >> l2;
    const int c = t & (W - 1), g = t >> lw;
    const int q = c0 + c;
    if (q == 0) continue;
    const int p = (g ? kb : ka) + (brev(i, l2) << l1);
    const double sv = sym(cosy(p), twx[q].x);
    const cd y = buf[idx];
    buf[idx] = cd{y.x * sv, y.y * sv};
  }
  __syncthreads();
  fft_inv(buf, l2, 2 * W, twy, f1);
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int c = idx & (W - 1), t = idx >> lw;
    const int j2 = t & (f2 - 1), g = t >> l2;
    H[((g ? rowb : rowa) + j2) * hw + c0 + c] = buf[(((g << lw) + c) << l2) + j2];
  }
}

int ilog2(int64_t v) {
  int l = 0;
  while ((int64_t(1) << l) < v) ++l;
  return l;
}

// exp(-2 pi i j / n), j < n/2, in long double, rounded once
void twiddles(int64_t n, double* out) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int64_t j = 0; j < n / 2; ++j) {
    const long double a = two_pi * static_cast<long double>(j) / static_cast<long double>(n);
    out[2 * j] = static_cast<double>(cosl(a));
    out[2 * j + 1] = static_cast<double>(-sinl(a));
  }
  out[0] = 1.0;
  out[1] = 0.0;
  out[2 * (n / 4)] = 0.0;  // n >= 8
  out[2 * (n / 4) + 1] = -1.0;
}

// The longest column kept on chip: 4096, or NKHIP_FFTPC_SPLIT where that is a power of two in
// [16, 4096] (tests put short columns through the split path with it).
int64_t split_length() {
  const char* e = std::getenv("NKHIP_FFTPC_SPLIT");
  if (!e || !*e) return 4096;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  if (*end || v < 16 || v > 4096 || (v & (v - 1))) return 4096;
  return v;
}

template <class K>
bool allow_lds(K kernel, size_t lds) {
  if (lds <= 65536) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) == hipSuccess)
    return true;
  (void)hipGetLastError();
  return false;
}

}  // namespace

int fftpc_check(int64_t ny, int64_t nx, double h, double r, double k) {
  auto pow2 = [](int64_t v) { return v >= 8 && v <= 16384 && (v & (v - 1)) == 0; };
  if (!pow2(ny) || !pow2(nx)) return NK_EINVAL;
  if (!(h > 0.0) || !(k > 0.0) || !std::isfinite(r) || !(k * r < 2.0)) return NK_EINVAL;
  return NK_OK;
}

int fftpc_create(FftPcPlan* p, int64_t ny, int64_t nx, double h, double r, double k,
                 double* work) {
  if (!p) return NK_EINVAL;
  const int rc = fftpc_check(ny, nx, h, r, k);
  if (rc) return rc;
  *p = FftPcPlan{};
  p->ny = ny;
  p->nx = nx;
  p->ly = ilog2(ny);
  p->lx2 = ilog2(nx / 2);
  p->ih2 = 1.0 / (h * h);
  p->r = r;
  p->ik = 1.0 / k;
  const int64_t n2 = nx / 2;
  p->rows = int(std::max<int64_t>(1, std::min<int64_t>(ny, kRowElems / n2)));
  // rows longer than 4096 (one row is 64 or 128 KB of LDS) and grids with more than 4096 row
  // groups go to the kernels whose blocks take several groups in turn
  const int64_t groups = ny / p->rows;
  if (nx > 4096 || groups > 4096) {
    p->row_iters = int(std::max<int64_t>(1, groups / 4096));
    const size_t lds = sizeof(cd) * size_t(p->rows) * size_t(n2);
    if (!allow_lds(fftpc_rows_fwd_long, lds) || !allow_lds(fftpc_rows_inv_long<false>, lds) ||
        !allow_lds(fftpc_rows_inv_long<true>, lds))
      return NK_EHIP;
  }
  if (ny > split_length()) {
    // ny = f1 f2 with f1 = min(split, 128): 128-long sub-columns make 32-column tiles of 64 KB,
    // and the other factor is then 64 or 128 for the lengths that need the split
    p->l1 = ilog2(std::min<int64_t>(split_length(), 128));
    p->l2 = p->ly - p->l1;
    p->lw1 = ilog2(std::min<int64_t>(n2, 4096 >> p->l1));
    p->lw2 = ilog2(std::min<int64_t>(n2, std::max(1, 2048 >> p->l2)));
  } else {
    // 64 KB of LDS per block of the column pass, 128 KB where two columns need it (ny = 4096)
    p->cols = int(std::min<int64_t>(n2, std::max<int64_t>(2, std::min<int64_t>(8, 4096 / ny))));
    if (!allow_lds(fftpc_cols, sizeof(cd) * size_t(ny) * size_t(p->cols))) return NK_EHIP;
  }
  std::vector<double> tab(size_t(nx + ny));
  twiddles(nx, tab.data());
  twiddles(ny, tab.data() + nx);
  if (hipMalloc(reinterpret_cast<void**>(&p->tables), sizeof(double) * tab.size()) != hipSuccess) {
    p->tables = nullptr;
    (void)hipGetLastError();
    return NK_ENOMEM;
  }
  if (hipMemcpy(p->tables, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) !=
      hipSuccess) {
    fftpc_destroy(p);
    return NK_EHIP;
  }
  if (work) {
    p->work = work;
  } else {
    if (hipMalloc(reinterpret_cast<void**>(&p->work), sizeof(double) * size_t(ny * nx)) !=
        hipSuccess) {
      p->work = nullptr;
      (void)hipGetLastError();
      fftpc_destroy(p);
      return NK_ENOMEM;
    }
    p->own_work = true;
  }
  return NK_OK;
}

void fftpc_destroy(FftPcPlan* p) {
  if (!p) return;
  if (p->tables) hipFree(p->tables);
  if (p->own_work && p->work) hipFree(p->work);
  *p = FftPcPlan{};
}

// The passes: out = IFFT2(FFT2(in) * scale / (ik - L^/2)), the transforms' 1/(nx ny) folded
// into the symbol; with w, the last pass also leaves the block partials of w . out.
hipError_t fftpc_apply(const FftPcPlan& p, const double* in, double* out, double ik, double scale,
                       const double* w, double* partial, int64_t* nblk, hipStream_t s) {
  if (!p.tables || !p.work || !in || !out || in == p.work || out == p.work || w == p.work)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) |
       reinterpret_cast<uintptr_t>(w)) & 15u)
    return hipErrorInvalidValue;
  if ((w == nullptr) != (partial == nullptr)) return hipErrorInvalidValue;
  if (!(ik > 0.5 * (p.r - 1.0)) || !std::isfinite(ik) || !std::isfinite(scale))
    return hipErrorInvalidValue;  // the symbol ik - L^/2 >= ik - (r - 1)/2 must stay positive
  if (nblk) *nblk = fftpc_dot_blocks(p);
  const int nx = int(p.nx), ny = int(p.ny), n2 = nx / 2;
  const cd* twx = reinterpret_cast<const cd*>(p.tables);
  const cd* twy = reinterpret_cast<const cd*>(p.tables + p.nx);
  cd* H = reinterpret_cast<cd*>(p.work);
  const size_t row_lds = sizeof(cd) * size_t(p.rows) * size_t(n2);
  const size_t col_lds = sizeof(cd) * size_t(ny) * size_t(p.cols);
  const int col_threads = std::min(kColThreadsMax, std::max(64, (ny * p.cols) / 4));
  Symbol sym{p.ih2, p.r, ik, scale / (double(p.nx) * double(p.ny))};
  const int row_blocks = int(fftpc_dot_blocks(p));
  auto threads_for = [](int elems) { return std::min(kColThreadsMax, std::max(64, elems / 4)); };
  if (p.row_iters)
    fftpc_rows_fwd_long<<<dim3(row_blocks), dim3(kLongThreads), row_lds, s>>>(
        in, H, nx, p.lx2, p.rows, p.row_iters, twx);
  else
    fftpc_rows_fwd<<<dim3(ny / p.rows), dim3(kRowThreads), row_lds, s>>>(in, H, nx, p.lx2, p.rows,
                                                                        twx);
  if (p.l1) {
    const int e1 = 1 << (p.l1 + p.lw1), e2 = 1 << (p.l2 + p.lw2 + 1);
    const dim3 g1((n2 >> p.lw1) << p.l2), g2((n2 >> p.lw2) << (p.l1 - 1));
    fftpc_cols_outer<false><<<g1, dim3(threads_for(e1)), sizeof(cd) * e1, s>>>(H, n2, p.l1, p.l2,
                                                                             p.lw1, twy);
    fftpc_cols_inner<<<g2, dim3(threads_for(e2)), sizeof(cd) * e2, s>>>(H, n2, p.l1, p.l2, p.lw2,
                                                                      twy, twx, sym);
    fftpc_cols_outer<true><<<g1, dim3(threads_for(e1)), sizeof(cd) * e1, s>>>(H, n2, p.l1, p.l2,
                                                                            p.lw1, twy);
  } else {
    fftpc_cols<<<dim3(n2 / p.cols), dim3(col_threads), col_lds, s>>>(H, ny, n2, p.ly,
                                                                    ilog2(p.cols), twy, twx, sym);
  }
  if (p.row_iters) {
    if (w)
      fftpc_rows_inv_long<true><<<dim3(row_blocks), dim3(kLongThreads), row_lds, s>>>(
          H, out, nx, p.lx2, p.rows, p.row_iters, twx, w, partial);
    else
      fftpc_rows_inv_long<false><<<dim3(row_blocks), dim3(kLongThreads), row_lds, s>>>(
          H, out, nx, p.lx2, p.rows, p.row_iters, twx, nullptr, nullptr);
  } else if (w)
    fftpc_rows_inv_dot<<<dim3(ny / p.rows), dim3(kRowThreads), row_lds, s>>>(
        H, out, nx, p.lx2, p.rows, twx, w, partial);
  else
    fftpc_rows_inv<<<dim3(ny / p.rows), dim3(kRowThreads), row_lds, s>>>(H, out, nx, p.lx2,
                                                                        p.rows, twx);
  return hipGetLastError();
}

}  // namespace nk
