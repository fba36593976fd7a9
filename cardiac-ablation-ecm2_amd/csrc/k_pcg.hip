// k_pcg.hip -- the device PCG's kernels (CGSolver::Mult, linalg/solvers.cpp:869-1004) for gfx950, shared by its three
// preconditioners (csrc/solvers.cpp pcg_loop: Jacobi or none, the Chebyshev smoother, the multigrid cycle): the
// deterministic two-pass dot, the stopping tests, the two halves of CGSolver's update, and the essential save /
// restore around a constrained Mult.  Vector streams (FP64 vectors read or written) per 16-byte pass (vec_pass.hpp):
//   dot_partial             2 (3 with c)        the partials of (a, b) [and (a, c)]          flat chunks
//   pcg_step_r<ONLY>        3                   r -= alpha (A d)                             grid-stride
//   pcg_step_r<JACOBI>      4 (3 without dinv)  ... and the partials of r.(dinv .* r)        grid-stride
//   pcg_step_r<CHEB>        6 (5 at order 1)    ... t = dinv .* r, z = c_0 t [, r.z]         grid-stride
//   pcg_update_xd           6 (5 without dinv)  x += alpha d, d = dinv .* r + beta d         flat, a pair per thread
//   pcg_update_xd_z         5                   x += alpha d, d = z + beta d                 grid-stride
//   pcg_residual            3                   r = b - ap (iterative_mode's start, once)    flat, a pair per thread
// The passes that sum park one partial per workgroup in a fixed order (park_partial) for k_dot_final -- no atomics,
// so two solves are bitwise equal; with a LoopCtl every kernel returns at once when the loop has stopped.
#include "vec_pass.hpp"

#include <algorithm>
#include <type_traits>

namespace ecm2
{
namespace
{
using namespace dev;
using kern::LoopCtl;
using kern::PcgStop;
using kern::PCG_RUNNING;
using kern::PCG_CONVERGED;
using kern::PCG_MAX_ITER;
using kern::PCG_NEG_BR;
using kern::PCG_DEN_ZERO;
using kern::PCG_NONFINITE;

// CGSolver's stopping tests (solvers.cpp:950-1000) as the device-driven loop runs them.
// kind 0: the test of iteration `it` on betanom = (B r, r): not finite -> MFEM_VERIFY's abort
// (PCG_NONFINITE, the host raises ECM2_ERR_NUMERIC); < 0 -> not converged (the preconditioner is not
// positive definite, :955-964); <= r0 -> converged (:972-977); it + 1 > max_iter -> stopped (:979-982).
// kind 1: the test of den = (A d, d) in iteration it's tail, after ++i (`it` is then the next
// iteration's number, :993-1004): not finite -> abort; == 0 -> stopped, not converged, final_iter = it.
__device__ void pcg_check_one(double v, const PcgStop &c)
{
   if (c.ctl->done) { return; }
   int done;
   double fin = v;
   if (c.kind == 0)
   {
      done = !isfinite(v) ? PCG_NONFINITE
             : v < 0.0    ? PCG_NEG_BR
             : v <= c.r0  ? PCG_CONVERGED
             : (c.it + 1 > c.max_iter ? PCG_MAX_ITER : PCG_RUNNING);
   }
   else
   {
      done = !isfinite(v) ? PCG_NONFINITE : (v == 0.0 ? PCG_DEN_ZERO : PCG_RUNNING);
      fin = *c.betanom;  // (final_norm = sqrt(betanom) of the iteration, :1047)
   }
   if (done) { loop_set_done(c.ctl, c.host, done, c.it, fin); }
   if (c.kind == 0) { loop_mark_checked(c.host, c.it); }
}

// Deterministic dot, pass 1: each workgroup writes its sum (park_partial: a fixed order per workgroup).  (A
// one-pass form -- the last workgroup to arrive on a counter sums the parks -- was measured slower:
// the 1,024 arrivals on one counter serialise, 16.6 vs 6.5 us per dot at a rank's 1.28M dofs,
// profiles/r5/dot_probe.txt.)
// (ctl: read only when no check writes it in the same kernel -- no __restrict__ on it)
// A flat grid of contiguous chunks: workgroup b sums pairs [b kStepChunk, (b + 1) kStepChunk) -- grid-stride
// loops stream 15-35% slower on this chip (profiles/r6/copy_probe.json: a 16-byte copy 6.67 TB/s flat against
// 4.4-5.4 TB/s grid-stride).
// lists 0 and 1 (stride np): the partials of (a, b) and, with c, of (a, c); c == a: a read once
constexpr int kStepK = 4, kStepChunk = 256 * kStepK;
__global__ void __launch_bounds__(256)
k_dot_partial(int n, const double *__restrict__ a, const double *__restrict__ b, const double *c, int np,
              double *__restrict__ partials, const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }  // (wave-uniform)
   __shared__ double red[8];
   double s0 = 0.0, s1 = 0.0;
   const long n2 = n / 2, base = (long)blockIdx.x * kStepChunk + threadIdx.x;
   const bool self = c == a;
   // (the chunk loop once per case of c, chosen here: a test of c inside it keeps the four trips' loads apart,
   // 26.6 against 24.3 us at 10.2M dofs)
   auto chunk = [&](auto two) {
      auto body = [&](auto k) {
         const auto u = ld(a, k);
         dot_acc(s0, u, ld(b, k));
         if constexpr (decltype(two)::value) { dot_acc(s1, u, self ? u : ld(c, k)); }
      };
#pragma unroll
      for (int k = 0; k < kStepK; k++)
      {
         const long i = base + 256 * k;
         if (i < n2) { body(Pair{i}); }
      }
      if ((n & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) { body(Entry{(long)n - 1}); }
   };
   if (c) { chunk(std::true_type{}); }
   else { chunk(std::false_type{}); }
   park_partial(s0, partials, red);
   if (c) { park_partial(s1, partials + np, red + 4); }
}

// pass 2 (one workgroup of kFinalThreads, sum_partials_fixed): the partials in a fixed order; with stop.ctl, a
// stopping test on the result.
__global__ void __launch_bounds__(kFinalThreads)
k_dot_final(int nparts, const double *__restrict__ partials, double *__restrict__ out, double *__restrict__ hout,
            const LoopCtl *ctl, PcgStop stop)
{
   if (ctl && ctl->done) { return; }
   __shared__ double red[kFinalThreads / 64];
   const double v = sum_partials_fixed(nparts, partials, red);
   if (threadIdx.x != 0) { return; }
   *out = v;
   if (hout) { *hout = v; }  // mapped pinned host mirror (the solver's read-back)
   if (stop.ctl) { pcg_check_one(v, stop); }
}

// The residual half of CGSolver's update (solvers.cpp:930-947): alpha = nom/den (-> *alpha_out: alpha of the last
// step run); r -= alpha ap (ap holds A d); then what AFTER names (kernels.hpp PcgStepAfter), the first piece of the
// preconditioner, on the entry just written:
//   ONLY    nothing: the cycle is applied to the stored r
//   JACOBI  z = dinv .* r (or r) and the partial sums of r.z, one per workgroup in a fixed order, finished by
//           k_dot_final.  z is not stored (k_pcg_update_xd forms it again from r where it is consumed: 4 vector
//           streams here instead of 8)
//   CHEB    the smoother's first term (solvers.cpp:631-656): t = dinv .* r (stored unless null: order 1), z = c0 t;
//           with `sum` (order 1: z is complete) the workgroup's partial of r.z
// x += alpha d is deferred to k_pcg_update_xd / k_pcg_update_xd_z (or k_pcg_finish_x after the stop), which read d
// anyway.  Same arithmetic per entry as CGSolver's add / Mult(prec) / Dot.  16-byte accesses, a grid-stride loop over
// kStepBlocks workgroups.  (The flat chunked grid of k_dot_partial was tried here too: a GPU test later in the same
// process aborted in garbage collection with it, reproducibly, and passed with this form -- profiles/r6/gpu5-gpu9;
// not diagnosed further, so this form stays.)
constexpr int kStepBlocks = kern::kDotPartials;
template <int AFTER>
__global__ void __launch_bounds__(256)
k_pcg_step_r(int n, const double *__restrict__ nom, const double *__restrict__ den, const double *__restrict__ ap,
             double *__restrict__ r, const double *__restrict__ dinv, double c0, double *__restrict__ t,
             double *__restrict__ z, double *__restrict__ partials, double *__restrict__ alpha_out, bool sum,
             const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }  // (wave-uniform)
   const double alpha = *nom / *den;
   if (blockIdx.x == 0 && threadIdx.x == 0) { *alpha_out = alpha; }
   double s = 0.0;
   each_entry(Sweep(n), n, [&](auto k) {
      const auto rn = ld(r, k) + (-alpha) * ld(ap, k);
      st(r, k, rn);
      if constexpr (AFTER == kern::PCG_STEP_JACOBI)
      {
         if (dinv) { dot_acc(s, rn, ld(dinv, k) * rn); }
         else { dot_acc(s, rn, rn); }
      }
      if constexpr (AFTER == kern::PCG_STEP_CHEB)
      {
         const auto tv = rn * ld(dinv, k);
         if (t) { st(t, k, tv); }
         const auto zv = c0 * tv;
         st(z, k, zv);
         if (sum) { dot_acc(s, rn, zv); }
      }
   });
   if constexpr (AFTER != kern::PCG_STEP_ONLY)
   {
      __shared__ double red[4];
      if (AFTER == kern::PCG_STEP_JACOBI || sum) { park_partial(s, partials, red); }
   }
}

// The direction half (solvers.cpp:930, 985-990): x += alpha d (this iteration's alpha = nom/den,
// deferred from k_pcg_step_r), then d = z + (betanom/nom) d with z = dinv .* r formed here.
// 6 vector streams (x, d, r, dinv read; x, d written) instead of k_pcg_step's x part and
// k_pcg_update_d's 3 + the stored z.  A flat grid, a pair per thread.
__global__ void __launch_bounds__(256)
k_pcg_update_xd(int n, const double *__restrict__ nom, const double *__restrict__ den,
                const double *__restrict__ betanom, double *__restrict__ x, double *__restrict__ d,
                const double *__restrict__ r, const double *__restrict__ dinv, const LoopCtl *ctl)
{
   const Flat w(n);
   if (w.t > w.n2 || (ctl && ctl->done)) { return; }
   const double alpha = *nom / *den, beta = *betanom / *nom;
   each_entry(w, n, [&](auto k) {
      const auto dold = ld(d, k);
      st(x, k, ld(x, k) + alpha * dold);
      const auto z = dinv ? ld(dinv, k) * ld(r, k) : ld(r, k);
      st(d, k, z + beta * dold);
   });
}

// The direction half with the stored z = B r: x += alpha d (this iteration's alpha = nom/den), d = z +
// (betanom/nom) d.  Grid-stride.
__global__ void __launch_bounds__(256)
k_pcg_update_xd_z(int n, const double *__restrict__ nom, const double *__restrict__ den,
                  const double *__restrict__ betanom, double *__restrict__ x, double *__restrict__ d,
                  const double *__restrict__ z, const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }
   const double alpha = *nom / *den, beta = *betanom / *nom;
   each_entry(Sweep(n), n, [&](auto k) {
      const auto dold = ld(d, k);
      st(x, k, ld(x, k) + alpha * dold);
      st(d, k, ld(z, k) + beta * dold);
   });
}

// After the loop: the stopping iteration's x += alpha d, when the stop came from its betanom test
// (converged, max_iter, (B r, r) < 0: CGSolver has already added alpha d then); a den == 0 stop
// comes after k_pcg_update_xd has run (x complete).
__global__ void k_pcg_finish_x(int n, const double *__restrict__ alpha, const double *__restrict__ d,
                               double *__restrict__ x, const LoopCtl *ctl)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   const int done = ctl->done;
   if (i >= n || !(done == PCG_CONVERGED || done == PCG_MAX_ITER || done == PCG_NEG_BR)) { return; }
   x[i] = x[i] + *alpha * d[i];
}

// The start of a solve with iterative_mode = true (CGSolver::Mult, solvers.cpp:875-884; BiCGSTABSolver::Mult,
// :1618-1627): r = b - ap, ap = A~ x of the caller's x.  Before the loop: no LoopCtl.  A flat grid, a pair per thread.
__global__ void __launch_bounds__(256)
k_pcg_residual(int n, const double *__restrict__ b, const double *__restrict__ ap, double *__restrict__ r)
{
   const Flat w(n);
   each_entry(w, n, [&](auto k) { st(r, k, ld(b, k) - ld(ap, k)); });
}

// ConstrainedOperator around a Mult without a vector copy: saved = v[ess], v[ess] = 0 ...
__global__ void k_ess_save_zero(int n, const int *__restrict__ idx, double *__restrict__ v,
                                double *__restrict__ saved)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { saved[i] = v[idx[i]]; v[idx[i]] = 0.0; }
}

// ... then v[ess] = y[ess] = saved (DIAG_ONE rows); sq_parts (optional): the block's sum of saved^2,
// the ess rows' part of (A v, v) = (A v~, v~) + sum_ess v^2 with v~ = v, ess zeroed
__global__ void __launch_bounds__(256)
k_ess_restore(int n, const int *__restrict__ idx, const double *__restrict__ saved, double *__restrict__ v,
              double *__restrict__ y, double *__restrict__ sq_parts)
{
   __shared__ double red[4];
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   double sq = 0.0;
   if (i < n)
   {
      const double sv = saved[i];
      v[idx[i]] = sv;
      y[idx[i]] = sv;
      sq = sv * sv;
   }
   if (sq_parts) { park_partial(sq, sq_parts, red); }
}

__global__ void k_pcg_precond(int n, const double *__restrict__ dinv, const double *__restrict__ r,
                              double *__restrict__ z)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { z[i] = dinv ? dinv[i] * r[i] : r[i]; }
}

// one thread: a stopping test after a distributed dot's all-reduce
__global__ void k_pcg_check(const double *__restrict__ v, PcgStop stop) { pcg_check_one(*v, stop); }

template <int AFTER>
void launch_step_r(const kern::PcgStepR &a, hipStream_t s)
{
   hipLaunchKernelGGL(k_pcg_step_r<AFTER>, dim3(kStepBlocks), dim3(256), 0, s, a.n, a.nom, a.den, a.ap, a.r, a.dinv,
                      a.c0, a.t, a.z, a.partials, a.alpha, a.sum, a.ctl);
   ECM2_HIP(hipGetLastError());
}

} // namespace

namespace kern
{

int step_parts(int n) { return std::max(1, (int)((n / 2 + kStepChunk - 1) / kStepChunk)); }

int dot_partials(int n, const double *a, const double *b, const double *c, int np, double *partials, hipStream_t s,
                 const LoopCtl *ctl)
{
   const int nb = step_parts(n);
   hipLaunchKernelGGL(k_dot_partial, dim3(nb), dim3(256), 0, s, n, a, b, c, np, partials, ctl);
   ECM2_HIP(hipGetLastError());
   return nb;
}

void dot(int n, const double *a, const double *b, double *partials, double *out, hipStream_t s, double *hout,
         const LoopCtl *ctl, const PcgStop *stop)
{
   const int nb = dot_partials(n, a, b, nullptr, 0, partials, s, ctl);
   dot_final(nb, partials, out, s, ctl, stop, hout);
}

void dot_final(int nparts, const double *partials, double *out, hipStream_t s, const LoopCtl *ctl,
               const PcgStop *stop, double *hout)
{
   hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(kFinalThreads), 0, s, nparts, partials, out, hout, ctl,
                      stop ? *stop : PcgStop{});
   ECM2_HIP(hipGetLastError());
}

void pcg_step_r(const PcgStepR &a, hipStream_t s)
{
   if (a.after == PCG_STEP_JACOBI) { launch_step_r<PCG_STEP_JACOBI>(a, s); }
   else if (a.after == PCG_STEP_CHEB) { launch_step_r<PCG_STEP_CHEB>(a, s); }
   else { launch_step_r<PCG_STEP_ONLY>(a, s); }
}

void pcg_update_xd(int n, const double *nom, const double *den, const double *betanom, double *x, double *d,
                   const double *r, const double *dinv, hipStream_t s, const LoopCtl *ctl)
{
   if (n == 0) { return; }
   hipLaunchKernelGGL(k_pcg_update_xd, dim3(grid_for(n / 2 + 1, 256)), dim3(256), 0, s, n, nom, den, betanom, x, d,
                      r, dinv, ctl);
   ECM2_HIP(hipGetLastError());
}

void pcg_update_xd_z(int n, const double *nom, const double *den, const double *betanom, double *x, double *d,
                     const double *z, hipStream_t s, const LoopCtl *ctl)
{
   hipLaunchKernelGGL(k_pcg_update_xd_z, dim3(kStepBlocks), dim3(256), 0, s, n, nom, den, betanom, x, d, z, ctl);
   ECM2_HIP(hipGetLastError());
}

void pcg_finish_x(int n, const double *alpha, const double *d, double *x, hipStream_t s, const LoopCtl *ctl)
{
   if (n == 0) { return; }
   hipLaunchKernelGGL(k_pcg_finish_x, dim3(grid_for(n, 256)), dim3(256), 0, s, n, alpha, d, x, ctl);
   ECM2_HIP(hipGetLastError());
}

void pcg_residual(int n, const double *b, const double *ap, double *r, hipStream_t s)
{
   if (n == 0) { return; }
   hipLaunchKernelGGL(k_pcg_residual, dim3(grid_for(n / 2 + 1, 256)), dim3(256), 0, s, n, b, ap, r);
   ECM2_HIP(hipGetLastError());
}

void pcg_check(const double *v, const PcgStop &stop, hipStream_t s)
{
   hipLaunchKernelGGL(k_pcg_check, dim3(1), dim3(1), 0, s, v, stop);
   ECM2_HIP(hipGetLastError());
}

void ess_save_zero(int n, const int *idx, double *v, double *saved, hipStream_t s)
{
   if (n <= 0) { return; }
   hipLaunchKernelGGL(k_ess_save_zero, dim3(grid_for(n, 256)), dim3(256), 0, s, n, idx, v, saved);
   ECM2_HIP(hipGetLastError());
}

void ess_restore(int n, const int *idx, const double *saved, double *v, double *y, hipStream_t s, double *sq_parts)
{
   if (n <= 0) { return; }
   hipLaunchKernelGGL(k_ess_restore, dim3(grid_for(n, 256)), dim3(256), 0, s, n, idx, saved, v, y, sq_parts);
   ECM2_HIP(hipGetLastError());
}

int ess_parts(int n) { return n > 0 ? grid_for(n, 256) : 0; }

void pcg_precond(int n, const double *dinv, const double *r, double *z, hipStream_t s)
{
   hipLaunchKernelGGL(k_pcg_precond, dim3(grid_for(n, 256)), dim3(256), 0, s, n, dinv, r, z);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
