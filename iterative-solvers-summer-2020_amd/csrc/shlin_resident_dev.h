// Device pieces the resident SH kernels share (shlin_resident.hip: the semi-implicit step with plain
// CG; shlin_resident_pc.hip, shlin_resident_pcm.hip: with the spectral preconditioner on chip;
// sh_resident.hip: the implicit step by Newton-CG): the fixed-order block sums,
// the point code of the framed LDS plane, and the 13-point stencil on it.
#pragma once

#include "nk_device.h"
#include "nk_kernels.h"

namespace nk {

namespace {

// status codes of include/nkhip.h (NK_OK, NK_NO_CONVERGENCE, NK_NONFINITE)
constexpr int64_t kOk = 0, kNoConv = 1, kNonFinite = 2;

// a value every lane holds alike, moved to scalar registers (uniform branches, fewer VGPRs)
__device__ __forceinline__ double uniform(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(b));
  const unsigned hi = __builtin_amdgcn_readfirstlane(unsigned(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Block sums of NV values, returned to every thread with the same bits (see the header).
template <int NV, int BS>
__device__ __forceinline__ void block_sum_all(double (&v)[NV], double (*sm)[BS / 64]) {
  constexpr int NW = BS / 64;
  wave_sum<NV>(v);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sm[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double acc = sm[k][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += sm[k][w];
    v[k] = uniform(acc);
  }
}

// Point code: bits 0-15 the frame offset of the point, 16-17 / 18-19 its row / column mirror
// (0 none, 1 within two of the low edge: mirrored past the high edge, 2 the reverse), bit 20 set
// for a point of the grid.  A thread's unused slots stand on point 0 with bit 20 clear: their
// reads stay inside the frame, their values are zero and they store nothing.
constexpr int kLive = 1 << 20;
__device__ __forceinline__ int point_code(int i, int ny, int nx) {
  const bool live = i < ny * nx;
  if (!live) i = 0;
  const int row = i / nx, col = i - row * nx;
  const int rf = row < 2 ? 1 : (row >= ny - 2 ? 2 : 0);
  const int cf = col < 2 ? 1 : (col >= nx - 2 ? 2 : 0);
  return ((row + 2) * (nx + 4) + col + 2) | (rf << 16) | (cf << 18) | (live ? kLive : 0);
}

// Everything derived from a point's code or from its U and Uo (offsets, neighbour addresses, the
// mirror and live predicates, D) is invariant in the CG loop.  Left alone, the compiler hoists all
// of it out of the loop and holds it in registers for every point of the thread, which is far more
// than the five planes the design keeps there.  The empty asm hides a value's origin, so what is
// derived from it is formed where it is used.
template <class T>
__device__ __forceinline__ T fresh(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// p of one point into the plane and into the frame cells that mirror it.  Sides >= 5: a point is
// never within two of both edges of a direction.  Offsets reach [0, (ny + 4)(nx + 4)) exactly.
__device__ __forceinline__ void put_p(double* fr, int code, double v, int rowspan, int nx) {
  const int f = code & 0xffff, rf = (code >> 16) & 3, cf = (code >> 18) & 3;
  const int dr = rf == 1 ? rowspan : -rowspan, dc = cf == 1 ? nx : -nx;
  fr[f] = v;
  if (rf) fr[f + dr] = v;
  if (cf) fr[f + dc] = v;
  if (rf && cf) fr[f + dr + dc] = v;
}

// (L p) at frame offset f
__device__ __forceinline__ double apply_L(const double* fr, int f, int ld, double c0, double c1,
                                          double c2, double c3) {
  const double a1 = fr[f - 1] + fr[f + 1] + fr[f - ld] + fr[f + ld];
  const double dg = fr[f - ld - 1] + fr[f - ld + 1] + fr[f + ld - 1] + fr[f + ld + 1];
  const double a2 = fr[f - 2] + fr[f + 2] + fr[f - 2 * ld] + fr[f + 2 * ld];
  return c0 * fr[f] + c1 * a1 + c2 * dg + c3 * a2;
}

}  // namespace

}  // namespace nk
