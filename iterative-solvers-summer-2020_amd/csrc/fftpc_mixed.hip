// The spectral preconditioner (fftpc.h) on grids whose sides are 2^a 3^b 5^c: the three passes of
// fftpc.hip -- rows real to complex into the packed half spectrum, whole columns forward + symbol +
// inverse on chip, rows complex to real (with the fused dot) -- 48 B per grid point, with
// mixed-radix transforms in the place of the radix-2 ones.  Hand-written for gfx950; no FFT
// library, no sincos on the device.
//
// Transform (mfft): length n = r0 r1 ... (FftStages: 3s, 5s, then 4s, then 2), in place in LDS.
// Forward is decimation in frequency.  Stage t works on groups of g = n / (r0 ... r(t-1))
// consecutive values, q = g / r apart within a butterfly:
//     y_k = W_g^(i k) sum_j W_r^(j k) x[i + j q],  stored at i + k q     (i < q, k < r),
// after which sub-group k holds the length-q problem of the wavenumbers = k (mod r).  Natural
// order in, digit-reversed order out: wavenumber p = k0 + r0 (k1 + r1 (k2 + ...)) ends at position
// k0 n/r0 + k1 n/(r0 r1) + ...  That permutation is a table built on the host (perm[p]); the
// packing, the Hermitian partner and the symbol address perm[p] directly, so no reordering pass
// exists.  Backward is the same flow graph reversed with conjugate twiddles (digit-reversed in,
// natural out, n times the inverse).  Twiddles W_g^(i k) = tw[i k n/g] come from a host table of
// all n roots in long double; the radix-3 and radix-5 butterflies' own constants are literals.
//
// Stage order.  The odd radices come first in the forward transform.  Their butterflies cancel equal
// inputs exactly, and while q is even a constant or an alternating (Nyquist) input reaches them as
// equal inputs: the odd stages then leave one exact nonzero per group and exact zeros, which take
// no rounding from the twiddles, and the stages of 4 and 2 that follow are exact on +-1 patterns.
// With 4 and 2 first the alternating input met an inexact twiddle before the odd stages, and
// the rounding it left in low wavenumbers -- where the symbol is cond(A0) ~ 4e5 times smaller
// than at the Nyquist wavenumber -- cost up to 1.3e-12 of the result (150 x 8), as it does NumPy.
//
// Work split: in every stage the block's threads share the nb n/r butterflies of all the block's
// transforms (n/3 or n/5 per transform in those stages); a thread holds one butterfly.  A radix-5
// butterfly is 10 doubles of data, 8 of sums and differences in flight and one twiddle (2) at a
// time, loaded as it is applied: the kernels compile to 56-63 VGPRs, no scratch, 8 waves per SIMD
// -- half of the 128 a thread of a 1024-thread block may use, so registers never limit the column
// kernel; its tile's LDS does (one block per CU above 80 KB).
//
// Ragged edges: ny need not be a multiple of the rows per group (the last block of a row pass
// holds fewer rows and still writes one dot partial), nx/2 need not be a multiple of the tile
// width (the last column tile is narrower), and nx/2 may be odd (k and its partner nx/2 - k are
// then always distinct).  Column tiles are stored ny + 1 apart in LDS: consecutive threads of the
// load and store loops walk across the tile's columns, which an even stride would put on one bank.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/nkhip.h"
#include "fftpc.h"
#include "fftpc_dev.h"
#include "nk_device.h"

namespace nk {

namespace {

constexpr int kRowThreads = 256;
constexpr int kColThreadsMax = 1024;
constexpr int kRowElems = 2048;  // complex values of LDS per block of a row pass (32 KB)

// One stage of nb transforms of length n (transform b at buf + b * stride): groups of g values,
// radix R.  tw[j * tws] = exp(-2 pi i j/n) for every j < n.
template <int R, bool Inv>
__device__ __forceinline__ void stage(cd* buf, int stride, int nb, int n, int g,
                                      const cd* __restrict__ tw, int tws) {
  const int q = g / R, per = n / R;
  const int ts = (n / g) * tws;
  const int total = nb * per;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int b = idx / per, rr = idx - b * per;
    const int grp = rr / q, i = rr - grp * q;
    cd* e = buf + b * stride + grp * g + i;
    cd x[R];
#pragma unroll
    for (int j = 0; j < R; ++j) x[j] = e[j * q];
    if (Inv) {
#pragma unroll
      for (int j = 1; j < R; ++j) x[j] = cmulc(x[j], tw[i * j * ts]);  // i j < g: inside the table
    }
    dft<R, Inv>(x);
    if (!Inv) {
#pragma unroll
      for (int j = 1; j < R; ++j) x[j] = cmul(x[j], tw[i * j * ts]);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) e[j * q] = x[j];
  }
  __syncthreads();
}

template <bool Inv>
__device__ __forceinline__ void stage_any(int r, cd* buf, int stride, int nb, int n, int g,
                                          const cd* __restrict__ tw, int tws) {
  switch (r) {
    case 4: stage<4, Inv>(buf, stride, nb, n, g, tw, tws); break;
    case 2: stage<2, Inv>(buf, stride, nb, n, g, tw, tws); break;
    case 3: stage<3, Inv>(buf, stride, nb, n, g, tw, tws); break;
    default: stage<5, Inv>(buf, stride, nb, n, g, tw, tws); break;
  }
}

// nb transforms by the whole block, behind a barrier on return.  Forward: natural order in,
// digit-reversed out.  Inv: digit-reversed in, natural out, n times the inverse transform.
template <bool Inv>
__device__ void mfft(cd* buf, int stride, int nb, const FftStages& st,
                     const cd* __restrict__ tw, int tws) {
  if (!Inv) {
    int g = st.n;
    for (int t = 0; t < st.ns; ++t) {
      stage_any<false>(st.radix[t], buf, stride, nb, st.n, g, tw, tws);
      g /= st.radix[t];
    }
  } else {
    int g = 1;
    for (int t = st.ns - 1; t >= 0; --t) {
      g *= st.radix[t];
      stage_any<true>(st.radix[t], buf, stride, nb, st.n, g, tw, tws);
    }
  }
}

extern __shared__ double2 mixed_lds[];

// Pass 1, as fftpc_rows_fwd: a row x[0..nx) is z[j] = x[2j] + i x[2j+1], transformed (length
// m = nx/2), and X[k] = E[k] + w^k O[k] written packed, (X[0], X[m]) in entry 0.  The block holds
// the rows [row0, row0 + nr), nr < rows in the last block.
__global__ __launch_bounds__(kRowThreads) void fftpc_mixed_rows_fwd(
    const double* __restrict__ in, cd* __restrict__ H, int ny, int m, int rows, FftStages st,
    const cd* __restrict__ twx, const int* __restrict__ permx) {
  cd* buf = mixed_lds;
  const int64_t row0 = int64_t(blockIdx.x) * rows;
  const int nr = ny - row0 < rows ? int(ny - row0) : rows;
  const cd* src = reinterpret_cast<const cd*>(in) + row0 * m;
  const int total = nr * m;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) buf[idx] = src[idx];
  __syncthreads();
  mfft<false>(buf, m, nr, st, twx, 2);
  const int per = (m >> 1) + 1;  // k = 0 .. floor(m/2), with its partner m - k
  for (int idx = threadIdx.x; idx < nr * per; idx += blockDim.x) {
    const int b = idx / per, k = idx - b * per;
    const cd* z = buf + b * m;
    cd* dst = H + (row0 + b) * m;
    if (k == 0) {
      const cd z0 = z[0];
      dst[0] = cd{z0.x + z0.y, z0.x - z0.y};  // (X[0], X[m])
      continue;
    }
    const int mk = m - k;  // != k for every k when m is odd
    const cd zk = z[permx[k]], zm = z[permx[mk]];
    const cd E = cd{0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y)};
    const cd D = cd{0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y)};  // (Z[k] - conj Z[m-k]) / 2
    const cd wO = cmul(cd{D.y, -D.x}, twx[k]);
    dst[k] = cadd(E, wO);
    if (mk != k) {  // X[m-k] = conj(E[k] - w^k O[k])
      const cd c = csub(E, wO);
      dst[mk] = cd{c.x, -c.y};
    }
  }
}

// Pass 3, as fftpc_rows_inv / fftpc_rows_inv_dot: the inverse of pass 1, and with Dot the block's
// sum of w_i out_i in store order into partial[blockIdx.x] (w may be `out` or the vector the
// application started from: each entry is read by the thread that then overwrites it).
template <bool Dot>
__global__ __launch_bounds__(kRowThreads) void fftpc_mixed_rows_inv(
    const cd* __restrict__ H, double* out, int ny, int m, int rows, FftStages st,
    const cd* __restrict__ twx, const int* __restrict__ permx, const double* w,
    double* __restrict__ partial) {
  cd* buf = mixed_lds;
  const int64_t row0 = int64_t(blockIdx.x) * rows;
  const int nr = ny - row0 < rows ? int(ny - row0) : rows;
  const int per = (m >> 1) + 1;
  for (int idx = threadIdx.x; idx < nr * per; idx += blockDim.x) {
    const int b = idx / per, k = idx - b * per;
    cd* z = buf + b * m;
    const cd* src = H + (row0 + b) * m;
    if (k == 0) {
      const cd x0 = src[0];
      z[0] = cd{x0.x + x0.y, x0.x - x0.y};
      continue;
    }
    const int mk = m - k;
    const cd xk = src[k], xm = src[mk];
    const cd E = cd{xk.x + xm.x, xk.y - xm.y};
    const cd O = cmulc(cd{xk.x - xm.x, xk.y + xm.y}, twx[k]);
    z[permx[k]] = cd{E.x - O.y, E.y + O.x};
    if (mk != k) z[permx[mk]] = cd{E.x + O.y, O.x - E.y};  // conj(E) + i conj(O)
  }
  __syncthreads();
  mfft<true>(buf, m, nr, st, twx, 2);
  cd* dst = reinterpret_cast<cd*>(out) + row0 * m;
  const cd* wv = reinterpret_cast<const cd*>(w) + row0 * m;
  const int total = nr * m;
  double acc[1] = {0.0};
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const cd zv = buf[idx];
    if (Dot) {
      const cd ww = wv[idx];
      acc[0] += ww.x * zv.x + ww.y * zv.y;
    }
    dst[idx] = zv;
  }
  if (Dot) {
    const double v = block_reduce<1, 1, kRowThreads>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
  }
}

// Pass 2, as fftpc_cols: the block holds the nc columns [c0, c0 + nc) of the half spectrum whole
// (nc < cols in the last tile), column c at buf + c (ny + 1).
__global__ __launch_bounds__(kColThreadsMax) void fftpc_mixed_cols(
    cd* __restrict__ H, int ny, int m, int cols, FftStages st, const cd* __restrict__ twy,
    const cd* __restrict__ twx, const int* __restrict__ permy, Symbol sym) {
  cd* buf = mixed_lds;
  // blocks that share an L2 (blockIdx % 8) take neighbouring column tiles
  int blk = blockIdx.x;
  const int nblk = gridDim.x;
  if ((nblk & 7) == 0) blk = (blk & 7) * (nblk >> 3) + (blk >> 3);
  const int c0 = blk * cols;
  const int nc = m - c0 < cols ? m - c0 : cols;
  const int cs = ny + 1;
  const int total = ny * nc;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int p = idx / nc, c = idx - p * nc;
    buf[c * cs + p] = H[int64_t(p) * m + c0 + c];
  }
  __syncthreads();
  mfft<false>(buf, cs, nc, st, twy, 1);
  const int hy = ny >> 1;
  if (c0 == 0) {  // column 0 = (DC column) + i (Nyquist column)
    for (int p = threadIdx.x; p <= hy; p += blockDim.x) {
      const int pm = p ? ny - p : 0;
      const int i = permy[p], im = permy[pm];
      const cd a = buf[i], b = buf[im];
      const double cp = twy[p].x;
      const double s0 = sym(cp, 1.0), s1 = sym(cp, -1.0);
      // unpacked first: A[p] = (Y[p] + conj Y[pm])/2, i B[p] = (Y[p] - conj Y[pm])/2.  (The
      // symbols differ by up to cond(A0): combining them first, (s0+s1)/2 and (s0-s1)/2, would
      // cancel.)
      const cd A = cd{0.5 * (a.x + b.x), 0.5 * (a.y - b.y)};
      const cd iB = cd{0.5 * (a.x - b.x), 0.5 * (a.y + b.y)};
      buf[i] = cd{s0 * A.x + s1 * iB.x, s0 * A.y + s1 * iB.y};
      // A[pm] = conj A[p], i B[pm] = -conj(i B[p])
      if (pm != p) buf[im] = cd{s0 * A.x - s1 * iB.x, s1 * iB.y - s0 * A.y};
    }
  }
  // every other column, by wavenumber: the cosines are read in order, the value is at perm[p]
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int c = idx / ny, p = idx - c * ny;
    const int q = c0 + c;
    if (q == 0) continue;
    const double sv = sym(twy[p].x, twx[q].x);
    cd* y = buf + c * cs + permy[p];
    *y = cd{y->x * sv, y->y * sv};
  }
  __syncthreads();
  mfft<true>(buf, cs, nc, st, twy, 1);
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int p = idx / nc, c = idx - p * nc;
    H[int64_t(p) * m + c0 + c] = buf[c * cs + p];
  }
}

int col_threads(const FftPcPlan& p) {
  const int want = int(p.ny) * p.cols / 4;
  return std::min(kColThreadsMax, std::max(64, (want + 63) / 64 * 64));
}
size_t col_lds(const FftPcPlan& p) { return sizeof(cd) * size_t(p.ny + 1) * size_t(p.cols); }

}  // namespace

// the 3s, the 5s, 4 while two factors of 2 remain, then 2 (see the header: stage order)
FftStages fftpc_stages_of(int n) {
  FftStages st;
  st.n = n;
  int v = n;
  for (int r : {3, 5, 4, 2})
    while (v % r == 0) {
      st.radix[st.ns++] = r;
      v /= r;
    }
  return st;
}

// perm[p]: where the forward transform leaves wavenumber p = k0 + r0 (k1 + r1 (...))
void fftpc_digit_reversal(const FftStages& st, int32_t* perm) {
  for (int p = 0; p < st.n; ++p) {
    int rem = p, span = st.n, pos = 0;
    for (int t = 0; t < st.ns; ++t) {
      span /= st.radix[t];
      pos += (rem % st.radix[t]) * span;
      rem /= st.radix[t];
    }
    perm[p] = pos;
  }
}

// exp(-2 pi i j / n) for every j < n (n even), in long double, rounded once; the roots on the axes
// exact
void fftpc_roots(int64_t n, double* out) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int64_t j = 0; j < n; ++j) {
    const long double a = two_pi * static_cast<long double>(j) / static_cast<long double>(n);
    out[2 * j] = static_cast<double>(cosl(a));
    out[2 * j + 1] = static_cast<double>(-sinl(a));
  }
  auto axis = [&](int64_t j, double c, double s) {
    out[2 * j] = c;
    out[2 * j + 1] = s;
  };
  axis(0, 1.0, 0.0);
  axis(n / 2, -1.0, 0.0);
  if (n % 4 == 0) {
    axis(n / 4, 0.0, -1.0);
    axis(3 * n / 4, 0.0, 1.0);
  }
}

int fftpc_mixed_create(FftPcPlan* p, int64_t ny, int64_t nx, double h, double r, double k,
                       double* work) {
  *p = FftPcPlan{};
  p->mixed = true;
  p->ny = ny;
  p->nx = nx;
  p->ih2 = 1.0 / (h * h);
  p->r = r;
  p->ik = 1.0 / k;
  const int64_t m = nx / 2;
  p->sx = fftpc_stages_of(int(m));
  p->sy = fftpc_stages_of(int(ny));
  p->rows = int(std::max<int64_t>(1, std::min<int64_t>(ny, kRowElems / m)));
  // 64 KB of LDS per block of the column pass where at least two columns fit in it, two columns
  // otherwise (ny > 2048: up to 128 KB).  The kernel's limit is raised once to the family's
  // largest tile, so that no later plan with a shorter column lowers it under a live one
  p->cols = int(std::min<int64_t>(m, std::max<int64_t>(2, std::min<int64_t>(8, 4096 / ny))));
  if (col_lds(*p) > 65536 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(fftpc_mixed_cols),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(sizeof(cd) * 4097 * 2)) != hipSuccess) {
    (void)hipGetLastError();
    return NK_EHIP;
  }
  // twx, twy (doubles), then permx, permy (int32)
  const size_t nd = size_t(2 * (nx + ny)), ni = size_t(m + ny);
  std::vector<double> tab(nd + (ni + 1) / 2);
  fftpc_roots(nx, tab.data());
  fftpc_roots(ny, tab.data() + 2 * nx);
  int32_t* perm = reinterpret_cast<int32_t*>(tab.data() + nd);
  fftpc_digit_reversal(p->sx, perm);
  fftpc_digit_reversal(p->sy, perm + m);
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

hipError_t fftpc_mixed_apply(const FftPcPlan& p, const double* in, double* out, double ik,
                             double scale, const double* w, double* partial, hipStream_t s) {
  const int nx = int(p.nx), ny = int(p.ny), m = nx / 2;
  const cd* twx = reinterpret_cast<const cd*>(p.tables);
  const cd* twy = twx + nx;
  const int* permx = reinterpret_cast<const int*>(p.tables + 2 * (p.nx + p.ny));
  const int* permy = permx + m;
  cd* H = reinterpret_cast<cd*>(p.work);
  const size_t row_lds = sizeof(cd) * size_t(p.rows) * size_t(m);
  const dim3 row_grid(static_cast<unsigned>(fftpc_dot_blocks(p)));
  const dim3 col_grid(static_cast<unsigned>((m + p.cols - 1) / p.cols));
  const Symbol sym{p.ih2, p.r, ik, scale / (double(p.nx) * double(p.ny))};
  hipLaunchKernelGGL(fftpc_mixed_rows_fwd, row_grid, dim3(kRowThreads), row_lds, s, in, H, ny, m,
                     p.rows, p.sx, twx, permx);
  hipLaunchKernelGGL(fftpc_mixed_cols, col_grid, dim3(col_threads(p)), col_lds(p), s, H, ny, m,
                     p.cols, p.sy, twy, twx, permy, sym);
  if (w)
    hipLaunchKernelGGL(fftpc_mixed_rows_inv<true>, row_grid, dim3(kRowThreads), row_lds, s, H, out,
                       ny, m, p.rows, p.sx, twx, permx, w, partial);
  else
    hipLaunchKernelGGL(fftpc_mixed_rows_inv<false>, row_grid, dim3(kRowThreads), row_lds, s, H,
                       out, ny, m, p.rows, p.sx, twx, permx, w, partial);
  return hipGetLastError();
}

}  // namespace nk
