// k_cheb.hip -- the vector passes of OperatorChebyshevSmoother (linalg/solvers.cpp:619-658) and of the power
// method behind its eigenvalue estimate (PowerMethod::EstimateLargestEigenvalue, linalg/operator.cpp:871-928), for
// gfx950.  The smoother is y = sum_k c_k (D^-1 A~)^k D^-1 x; per entry the reference's operations in its order:
// t *= dinv, then y += c_k t.  Vector streams (FP64 vectors read or written) per pass:
//   cheb_first        4 (3 for the last term of order 1)   t = dinv .* x, y = c_0 t
//   cheb_accum        5 (4 last term; +1 with the r.y sum) t = dinv .* h, y += c_k t
//   cheb_power_pass   4                                    v1 = dinv .* h, (v0, v1), (v1, v1)
//   cheb_scale        2                                    v *= 1 / sqrt(norm)
// (The PCG that takes the smoother as its preconditioner fuses the first term into its residual step:
// k_pcg.hip, k_pcg_step_r<PCG_STEP_CHEB>.)  All grid-stride sweeps of vec_pass.hpp over kBlocks workgroups: 16-byte
// accesses, the last thread takes an odd n's tail entry with the same body; the passes that sum park one partial per
// workgroup in a fixed order (park_partial) for kern::dot_final -- no atomics, so two applications are bitwise equal;
// with a LoopCtl every kernel returns at once when the loop has stopped.
#include "vec_pass.hpp"

namespace ecm2
{
namespace
{
using namespace dev;
using kern::LoopCtl;

constexpr int kBlocks = kern::kDotPartials;

// t = dinv .* x (stored unless t is null: the only term of order 1), y = c0 t
__global__ void __launch_bounds__(256)
k_cheb_first(int n, const double *__restrict__ dinv, const double *__restrict__ x, double c0, double *__restrict__ t,
             double *__restrict__ y)
{
   each_entry(Sweep(n), n, [&](auto k) {
      const auto tv = ld(x, k) * ld(dinv, k);
      if (t) { st(t, k, tv); }
      st(y, k, c0 * tv);
   });
}

// t = dinv .* h (h = A~ t_prev; stored unless t is null: the last term), y += ck t; with r (the PCG's last
// term): the workgroup's partial of r.y
__global__ void __launch_bounds__(256)
k_cheb_accum(int n, const double *__restrict__ dinv, const double *__restrict__ h, double ck, double *__restrict__ t,
             double *__restrict__ y, const double *__restrict__ r, double *__restrict__ partials, const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }  // (wave-uniform)
   __shared__ double red[4];
   double s = 0.0;
   each_entry(Sweep(n), n, [&](auto k) {
      const auto tv = ld(h, k) * ld(dinv, k);
      if (t) { st(t, k, tv); }
      const auto yn = ld(y, k) + ck * tv;
      st(y, k, yn);
      if (r) { dot_acc(s, ld(r, k), yn); }
   });
   if (r) { park_partial(s, partials, red); }
}

// One power step's pass: v1 = dinv .* h (h = A~ v0) with the partials of (v0, v1) at partials[0, kBlocks) and
// of (v1, v1) -- the next step's norm -- at partials[kBlocks, 2 kBlocks)
__global__ void __launch_bounds__(256)
k_cheb_power_pass(int n, const double *__restrict__ dinv, const double *__restrict__ h, const double *__restrict__ v0,
                  double *__restrict__ v1, double *__restrict__ partials)
{
   __shared__ double red0[4], red1[4];
   double s0 = 0.0, s1 = 0.0;
   each_entry(Sweep(n), n, [&](auto k) {
      const auto v = ld(h, k) * ld(dinv, k);
      st(v1, k, v);
      dot_acc(s0, ld(v0, k), v);
      dot_acc(s1, v, v);
   });
   park_partial(s0, partials, red0);
   park_partial(s1, partials + gridDim.x, red1);
}

// v0 /= sqrt(normV0) as Vector::operator/= does it: m = 1 / sqrt(*norm), v *= m
__global__ void __launch_bounds__(256) k_cheb_scale(int n, const double *__restrict__ norm, double *__restrict__ v)
{
   const double m = 1.0 / sqrt(*norm);
   each_entry(Sweep(n), n, [&](auto k) { st(v, k, ld(v, k) * m); });
}

// The power method's default start vector: v[i] = (h(i) + 0.5) / 2^32 in (0, 1), h the 32-bit mix
//    h = i + 1; h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16
// (a bijection of the 32-bit integers, so no two entries are equal).  The reference draws from glibc's
// rand() seeded with 12345 (Vector::Randomize, linalg/vector.cpp:955-966), which is not reproduced.
__global__ void k_cheb_fill_hash(int n, double *__restrict__ v)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) { return; }
   unsigned h = (unsigned)i + 1u;
   h ^= h >> 16;
   h *= 0x7feb352du;
   h ^= h >> 15;
   h *= 0x846ca68bu;
   h ^= h >> 16;
   v[i] = ((double)h + 0.5) * (1.0 / 4294967296.0);
}

} // namespace

namespace kern
{

void cheb_first(int n, const double *dinv, const double *x, double c0, double *t, double *y, hipStream_t s)
{
   hipLaunchKernelGGL(k_cheb_first, dim3(kBlocks), dim3(256), 0, s, n, dinv, x, c0, t, y);
   ECM2_HIP(hipGetLastError());
}

void cheb_accum(int n, const double *dinv, const double *h, double ck, double *t, double *y, hipStream_t s,
                const double *r, double *partials, const LoopCtl *ctl)
{
   ECM2_VERIFY(!r || partials, ERR_INTERNAL, "cheb_accum: the r.y sum needs its partials");
   hipLaunchKernelGGL(k_cheb_accum, dim3(kBlocks), dim3(256), 0, s, n, dinv, h, ck, t, y, r, partials, ctl);
   ECM2_HIP(hipGetLastError());
}

void cheb_power_pass(int n, const double *dinv, const double *h, const double *v0, double *v1, double *partials,
                     hipStream_t s)
{
   hipLaunchKernelGGL(k_cheb_power_pass, dim3(kBlocks), dim3(256), 0, s, n, dinv, h, v0, v1, partials);
   ECM2_HIP(hipGetLastError());
}

void cheb_scale(int n, const double *norm, double *v, hipStream_t s)
{
   hipLaunchKernelGGL(k_cheb_scale, dim3(kBlocks), dim3(256), 0, s, n, norm, v);
   ECM2_HIP(hipGetLastError());
}

void cheb_fill_hash(int n, double *v, hipStream_t s)
{
   if (n <= 0) { return; }
   hipLaunchKernelGGL(k_cheb_fill_hash, dim3(grid_for(n, 256)), dim3(256), 0, s, n, v);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
