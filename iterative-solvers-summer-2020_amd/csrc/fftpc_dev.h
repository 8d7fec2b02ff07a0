// Device pieces the two kernel families of the spectral preconditioner share (fftpc.hip: sides
// that are powers of two; fftpc_mixed.hip: sides 2^a 3^b 5^c): complex arithmetic on double2 and
// the symbol.
#pragma once

#include <hip/hip_runtime.h>

namespace nk {

namespace {

using cd = double2;

__device__ __forceinline__ cd cadd(cd a, cd b) { return cd{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd csub(cd a, cd b) { return cd{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cd cmul(cd a, cd w) {
  return cd{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x};
}
// a * conj(w)
__device__ __forceinline__ cd cmulc(cd a, cd w) {
  return cd{a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y};
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

}  // namespace

}  // namespace nk
