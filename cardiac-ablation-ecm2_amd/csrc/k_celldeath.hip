// k_celldeath.hip -- the cell-death state's kernels (gfx950): the per-entry update (celldeath_math.hpp's
// celldeath_update) and the lesion measure.  Vector streams (FP64 vectors read or written) per 16-byte pass
// (vec_pass.hpp):
//   celldeath_step      7 (8 with T1)   T0 [, T1], N, U, D read; N, U, D written in place     flat chunks
//   celldeath_measure   2               w and D read once for sum w D, sum w [D >= theta], sum w   flat chunks
// Both are k_dot_partial's flat grid of contiguous chunks (k_pcg.hip, for the reason recorded there) and park one
// partial per workgroup in a fixed order (park_partial) for a one-workgroup final pass (sum_partials_fixed): no
// atomics, two runs are bitwise equal.  The step's partial is its count of invalid entries (exact in a double).
// The update is arithmetic-heavy (three rate exponentials and four propagator exponentials per substep), so the
// chunk's trips and a pair's two entries run one after the other, not interleaved: the live set stays one entry's.
#include "vec_pass.hpp"
#include "celldeath.hpp"

#include <algorithm>

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kCdTrips = 4, kCdChunk = 256 * kCdTrips;  // pairs per workgroup: kern::step_parts' chunk

// celldeath_update on a pair's entries in index order, or on one entry; bad += the entries left untouched
__device__ __forceinline__ void cd_update(const CellDeathParams &P, v2d t0, v2d dT, double dt, int nsub, v2d &N, v2d &U,
                                          v2d &D, double &bad)
{
   double n = N.x, u = U.x, d = D.x;
   if (!celldeath_update(P, t0.x, dT.x, dt, nsub, n, u, d)) { bad += 1.0; }
   N.x = n; U.x = u; D.x = d;
   n = N.y; u = U.y; d = D.y;
   if (!celldeath_update(P, t0.y, dT.y, dt, nsub, n, u, d)) { bad += 1.0; }
   N.y = n; U.y = u; D.y = d;
}
__device__ __forceinline__ void cd_update(const CellDeathParams &P, double t0, double dT, double dt, int nsub,
                                          double &N, double &U, double &D, double &bad)
{
   if (!celldeath_update(P, t0, dT, dt, nsub, N, U, D)) { bad += 1.0; }
}

__global__ void __launch_bounds__(256)
k_celldeath_step(int n, CellDeathParams P, const double *__restrict__ T0, const double *__restrict__ T1, double dt,
                 int nsub, double *__restrict__ N, double *__restrict__ U, double *__restrict__ D,
                 double *__restrict__ partials)
{
   __shared__ double red[4];
   double bad = 0.0;
   const long n2 = n / 2, base = (long)blockIdx.x * kCdChunk + threadIdx.x;
   auto body = [&](auto k) {
      const auto t0 = ld(T0, k);
      const auto dT = T1 ? ld(T1, k) - t0 : t0 * 0.0;
      auto nv = ld(N, k), uv = ld(U, k), dv = ld(D, k);
      // (without T1 a non-finite t0 gives dT = NaN: the entry is invalid either way)
      cd_update(P, t0, dT, dt, nsub, nv, uv, dv, bad);
      st(N, k, nv);
      st(U, k, uv);
      st(D, k, dv);
   };
#pragma unroll 1
   for (int k = 0; k < kCdTrips; k++)
   {
      const long i = base + 256 * k;
      if (i < n2) { body(Pair{i}); }
   }
   if ((n & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) { body(Entry{(long)n - 1}); }
   park_partial(bad, partials, red);
}

__global__ void __launch_bounds__(kFinalThreads)
k_celldeath_count(int nparts, const double *__restrict__ partials, int *__restrict__ count)
{
   __shared__ double red[kFinalThreads / 64];
   const double v = sum_partials_fixed(nparts, partials, red);
   if (threadIdx.x == 0) { *count = (int)v; }
}

// The measure's first pass: lists 0, 1, 2 (stride np) = the partials of sum w D, sum w [D >= theta], sum w.  A
// thread's chain is its trips' pairs in index order (then the tail entry); the tree above it: park_partial's.
__global__ void __launch_bounds__(256)
k_celldeath_measure(int n, const double *__restrict__ D, const double *__restrict__ w, double theta, int np,
                    double *__restrict__ partials)
{
   __shared__ double red[12];
   double s0 = 0.0, s1 = 0.0, s2 = 0.0;
   const long n2 = n / 2, base = (long)blockIdx.x * kCdChunk + threadIdx.x;
   auto one = [&](double wv, double dv) {
      s0 += wv * dv;
      s1 += dv >= theta ? wv : 0.0;
      s2 += wv;
   };
#pragma unroll
   for (int k = 0; k < kCdTrips; k++)
   {
      const long i = base + 256 * k;
      if (i < n2)
      {
         const v2d wv = ld(w, Pair{i}), dv = ld(D, Pair{i});
         one(wv.x, dv.x);
         one(wv.y, dv.y);
      }
   }
   if ((n & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) { one(w[n - 1], D[n - 1]); }
   park_partial(s0, partials, red);
   park_partial(s1, partials + np, red + 4);
   park_partial(s2, partials + 2 * (long)np, red + 8);
}

__global__ void __launch_bounds__(kFinalThreads)
k_celldeath_measure_final(int nparts, int np, const double *__restrict__ partials, double *__restrict__ sums)
{
   constexpr int NW = kFinalThreads / 64;
   __shared__ double red[3 * NW];
   for (int l = 0; l < 3; l++)
   {
      const double v = sum_partials_fixed(nparts, partials + (long)l * np, red + l * NW);
      if (threadIdx.x == 0) { sums[l] = v; }
   }
}

} // namespace

namespace kern
{

int celldeath_parts(int n) { return std::max(1, (int)((n / 2 + kCdChunk - 1) / kCdChunk)); }

void celldeath_step(int n, const CellDeathParams &p, const double *T0, const double *T1, double dt, int nsub,
                    double *N, double *U, double *D, double *partials, hipStream_t s)
{
   hipLaunchKernelGGL(k_celldeath_step, dim3(celldeath_parts(n)), dim3(256), 0, s, n, p, T0, T1, dt, nsub, N, U, D,
                      partials);
   ECM2_HIP(hipGetLastError());
}

void celldeath_count(int nparts, const double *partials, int *count, hipStream_t s)
{
   hipLaunchKernelGGL(k_celldeath_count, dim3(1), dim3(kFinalThreads), 0, s, nparts, partials, count);
   ECM2_HIP(hipGetLastError());
}

void celldeath_measure(int n, const double *D, const double *w, double theta, double *partials, double *sums,
                       hipStream_t s)
{
   const int np = celldeath_parts(n);
   hipLaunchKernelGGL(k_celldeath_measure, dim3(np), dim3(256), 0, s, n, D, w, theta, np, partials);
   ECM2_HIP(hipGetLastError());
   hipLaunchKernelGGL(k_celldeath_measure_final, dim3(1), dim3(kFinalThreads), 0, s, np, np, partials, sums);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
