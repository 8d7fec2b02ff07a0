// Device pieces the two kernel families of the spectral preconditioner share (fftpc.hip: sides
// that are powers of two; fftpc_mixed.hip: sides 2^a 3^b 5^c) and the resident kernels
// (shlin_resident_pc.hip, shlin_resident_pcm.hip) share: complex arithmetic on double2, the
// butterflies of radix 2, 3, 4 and 5, and the symbol.
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

// The butterflies of the mixed-radix transforms (fftpc_mixed.hip, shlin_resident_pcm.hip).
constexpr double kC3 = 0.86602540378443864676;   // sin(2 pi/3)
constexpr double kR5 = 0.55901699437494742410;   // sqrt(5)/4 = (cos(2 pi/5) - cos(4 pi/5))/2
constexpr double kS51 = 0.95105651629515357212;  // sin(2 pi/5)
constexpr double kS52 = 0.58778525229247312917;  // sin(4 pi/5)

// -i a forward, +i a backward
template <bool Inv>
__device__ __forceinline__ cd rot(cd a) {
  return Inv ? cd{-a.y, a.x} : cd{a.y, -a.x};
}
__device__ __forceinline__ cd cscale(double s, cd a) { return cd{s * a.x, s * a.y}; }

// x <- the length-R transform of x with W_R = exp(-2 pi i/R) (Inv: its conjugate)
template <int R, bool Inv>
__device__ __forceinline__ void dft(cd (&x)[R]) {
  if constexpr (R == 2) {
    const cd a = x[0];
    x[0] = cadd(a, x[1]);
    x[1] = csub(a, x[1]);
  } else if constexpr (R == 3) {
    const cd t = cadd(x[1], x[2]);
    const cd b = rot<Inv>(cscale(kC3, csub(x[1], x[2])));
    const cd a = cd{x[0].x - 0.5 * t.x, x[0].y - 0.5 * t.y};
    x[0] = cadd(x[0], t);
    x[1] = cadd(a, b);
    x[2] = csub(a, b);
  } else if constexpr (R == 4) {
    const cd a = cadd(x[0], x[2]), b = csub(x[0], x[2]);
    const cd c = cadd(x[1], x[3]), d = rot<Inv>(csub(x[1], x[3]));
    x[0] = cadd(a, c);
    x[1] = cadd(b, d);
    x[2] = csub(a, c);
    x[3] = csub(b, d);
  } else {
    static_assert(R == 5, "radix 2, 3, 4 or 5");
    const cd t1 = cadd(x[1], x[4]), t2 = cadd(x[2], x[3]);
    const cd t3 = csub(x[1], x[4]), t4 = csub(x[2], x[3]);
    // cos(2 pi/5) + cos(4 pi/5) = -1/2, their difference sqrt(5)/2: in this form a constant input
    // (t1 = t2 = 2 x0) leaves a1 = a2 = 0 exactly, as the other radices do, so a row or column of
    // equal values puts no rounding into the wavenumbers whose symbol is cond(A0) times smaller
    const cd s = cadd(t1, t2), d = cscale(kR5, csub(t1, t2));
    const cd c = cd{x[0].x - 0.25 * s.x, x[0].y - 0.25 * s.y};
    const cd a1 = cadd(c, d), a2 = csub(c, d);
    const cd b1 = rot<Inv>(cd{kS51 * t3.x + kS52 * t4.x, kS51 * t3.y + kS52 * t4.y});
    const cd b2 = rot<Inv>(cd{kS52 * t3.x - kS51 * t4.x, kS52 * t3.y - kS51 * t4.y});
    x[0] = cadd(x[0], s);
    x[1] = cadd(a1, b1);
    x[2] = cadd(a2, b2);
    x[3] = csub(a2, b2);
    x[4] = csub(a1, b1);
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

}  // namespace

}  // namespace nk
