// The semi-implicit Swift-Hohenberg step (shlin.cpp) for small grids, resident on one CU (gfx950).
//
// ShLinStepper::step spends a 64 x 64 step on launch and read-back latency: about 90 CG iterations
// of two launches and two host read-backs each around a few hundred nanoseconds of arithmetic.
// Here one workgroup owns one state and runs whole steps -- diagonal, right-hand side, warm start,
// the CG loop with the stepper's stopping rule and guards, and the (U, Uo) <- (x, U) hand-over --
// in a single launch; a batch of independent states is one block each.  No block waits for,
// signals or reads another, and every loop is bounded by maxiter and nsteps.
//
// Where the data live
//   p        the search direction, the only vector the stencil reads: one LDS plane with a
//            two-point periodic frame, (ny + 4) x (nx + 4) doubles, so the 13 reads of a point are
//            plain offsets with no wrap arithmetic.  The owner of a point within two of an edge
//            stores its new p into the frame cells that mirror it as well (one, or three at a
//            corner); one barrier then publishes plane and frame together.
//   x r q    registers of the thread that owns the point, with U and Uo (the diagonal
//   U Uo     D = (5U - Uo)^2 k/16 - g k U is four flops from them and is recomputed where it is
//            used, which is cheaper than a sixth register plane; both are the member's answer if
//            the step fails).
// A thread owns the points t, t + BS, t + 2 BS, ... (PPT of them): global reads and writes are
// coalesced and a wave's LDS reads walk along rows.  The frame offset and the two mirror flags of
// a point are packed into one register.  HBM sees U and Uo once, the result once, and 32 bytes of
// per-member results.
//
// Reductions.  p.q and r.r (and |b|^2 with the first r.r) are summed per thread over its points in
// index order, over the wave by the xor butterfly (nk_device.h wave_sum), and across the waves by
// every thread adding the per-wave values from LDS in wave order.  All threads therefore hold the
// same bits, the loop's branches are uniform, and a member's result depends on its own inputs
// alone: not on the batch size, its place in the batch, or the run.
//
// Barriers per CG iteration: three (p published; p.q; r.r).  The two reduction buffers alternate,
// so a buffer is rewritten only after a barrier that every reader of its last use has passed.
#include "shlin_resident_dev.h"

namespace nk {

namespace {

extern __shared__ double resident_frame[];

template <int BS, int PPT>
__global__ void __launch_bounds__(BS) shlin_resident_kernel(ShLinResidentArgs A) {
  constexpr int NW = BS / 64;
  __shared__ double red[2][2][NW];
  double* fr = resident_frame;
  const int ny = A.ny, nx = A.nx, n = ny * nx, ld = nx + 4, rowspan = ny * ld;
  const int t = threadIdx.x;
  const int64_t m = blockIdx.x;
  const double* Ug = A.U + m * n;
  const double* Uog = A.Uo + m * n;
  // only the centre coefficient of L and D depend on the member's r and g
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

  int64_t iters = 0, steps = 0, status = kOk;
  double relres = 0.0;
  for (int64_t s = 0; s < A.nsteps; ++s) {
    // the plane holds U: b = (I + L k/2) U, and the warm start x = U gives r = b - A U
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int c = fresh(code[j]);
      if (c & kLive) put_p(fr, c, u[j], rowspan, nx);
    }
    __syncthreads();
    double v2[2] = {0.0, 0.0};
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
      v2[0] += b * b;
      v2[1] += r[j] * r[j];
      __builtin_amdgcn_sched_barrier(0);  // one point's 13 reads in flight, not all PPT points'
    }
    block_sum_all<2, BS>(v2, red[1]);
    const double bnorm = sqrt(v2[0]), stop = A.rtol * bnorm;
    double rr = v2[1], beta = 0.0;
    int64_t it = 0;
    bool bad = false;
    while (sqrt(rr) > stop && it < A.maxiter) {
      if (!(rr > 0.0)) {  // above the stop and not positive: non-finite data
        bad = true;
        break;
      }
      // p = r + beta p.  The last readers of the plane and its frame (the stencil below, the
      // owner's own read in the update) are behind the r.r barrier.
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive)
          put_p(fr, c, it == 0 ? r[j] : r[j] + beta * fr[c & 0xffff], rowspan, nx);
      }
      __syncthreads();
      double v1[1] = {0.0};
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
      block_sum_all<1, BS>(v1, red[0]);
      const double pq = v1[0];
      if (!(pq > 0.0)) {  // not SPD (g k U dominated) or non-finite data
        bad = true;
        break;
      }
      const double alpha = rr / pq, rr_old = rr;
      v1[0] = 0.0;
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        const int c = fresh(code[j]);
        if (c & kLive) {
          x[j] += alpha * fr[c & 0xffff];
          r[j] -= alpha * q[j];
          v1[0] += r[j] * r[j];
        }
      }
      block_sum_all<1, BS>(v1, red[1]);
      rr = v1[0];
      beta = rr / rr_old;
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
  if (t == 0) A.out[m] = ShLinResidentOut{iters, steps, relres, status};
}

template <int BS, int PPT>
hipError_t launch_variant(const ShLinResidentArgs& A, int64_t batch, hipStream_t s) {
  const size_t lds = sizeof(double) * size_t(A.ny + 4) * size_t(A.nx + 4);
  if (lds > 65536) {  // once per variant: the largest frame under the cap (ny = 5)
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&shlin_resident_kernel<BS, PPT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, int(kShLinResidentMaxLds));
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL((shlin_resident_kernel<BS, PPT>), dim3(unsigned(batch)), dim3(BS), lds, s,
                     A);
  return hipGetLastError();
}

}  // namespace

bool shlin_resident_fits(int64_t ny, int64_t nx) {
  return ny >= 5 && nx >= 5 && ny <= kShLinResidentMaxPoints / nx &&
         ny * nx <= kShLinResidentMaxPoints;
}

hipError_t shlin_resident_launch(const ShLinResidentArgs& A, int64_t batch, hipStream_t s) {
  if (!shlin_resident_fits(A.ny, A.nx) || batch < 1 || batch > 0x7fffffff)
    return hipErrorInvalidValue;
  const int n = A.ny * A.nx;
  // few points: four waves (cheaper barriers, several members per CU); up to 64 x 64: four
  // points per thread; to the cap: nine
  if (n <= 1024) return launch_variant<256, 4>(A, batch, s);
  if (n <= 4096) return launch_variant<1024, 4>(A, batch, s);
  static_assert(512 * 18 >= kShLinResidentMaxPoints, "every point under the cap needs an owner");
  return launch_variant<512, 18>(A, batch, s);
}

}  // namespace nk
