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
#include "fftpc.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/nkhip.h"
#include "nk_device.h"

namespace nk {

namespace {

using cd = double2;

constexpr int kRowThreads = 256;
constexpr int kColThreadsMax = 1024;
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
__global__ __launch_bounds__(kRowThreads) void fftpc_rows_fwd(const double* __restrict__ in,
                                                              cd* __restrict__ H, int nx, int lx2,
                                                              int rows,
                                                              const cd* __restrict__ twx) {
  cd* buf = fft_lds;
  const int n2 = nx >> 1;
  const int64_t row0 = int64_t(blockIdx.x) * rows;
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

}  // namespace

int fftpc_check(int64_t ny, int64_t nx, double h, double r, double k) {
  auto pow2 = [](int64_t v) { return v >= 8 && v <= 4096 && (v & (v - 1)) == 0; };
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
  // 64 KB of LDS per block of the column pass, 128 KB where two columns need it (ny = 4096)
  p->cols = int(std::min<int64_t>(n2, std::max<int64_t>(2, std::min<int64_t>(8, 4096 / ny))));
  const size_t lds = sizeof(cd) * size_t(ny) * size_t(p->cols);
  if (lds > 65536 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(fftpc_cols),
                          hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return NK_EHIP;
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

// The three passes: out = IFFT2(FFT2(in) * scale / (ik - L^/2)), the transforms' 1/(nx ny) folded
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
  fftpc_rows_fwd<<<dim3(ny / p.rows), dim3(kRowThreads), row_lds, s>>>(in, H, nx, p.lx2, p.rows,
                                                                      twx);
  fftpc_cols<<<dim3(n2 / p.cols), dim3(col_threads), col_lds, s>>>(H, ny, n2, p.ly,
                                                                  ilog2(p.cols), twy, twx, sym);
  if (w)
    fftpc_rows_inv_dot<<<dim3(ny / p.rows), dim3(kRowThreads), row_lds, s>>>(
        H, out, nx, p.lx2, p.rows, twx, w, partial);
  else
    fftpc_rows_inv<<<dim3(ny / p.rows), dim3(kRowThreads), row_lds, s>>>(H, out, nx, p.lx2,
                                                                        p.rows, twx);
  return hipGetLastError();
}

}  // namespace nk
