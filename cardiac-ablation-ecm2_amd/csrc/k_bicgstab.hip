// k_bicgstab.hip -- the vector passes of the device BiCGSTAB (gfx950): BiCGSTABSolver::Mult's iteration
// (linalg/solvers.cpp:1650-1784) around its two Mults, fused into five passes of 16-byte accesses
//   bcg_update_p   6 streams   p = r + beta (p - omega v), phat = dinv .* p
//   dot_partials   2           (r~, v)                                             (k_pcg.hip)
//   bcg_update_s   5           s = r - alpha v (into r), shat = dinv .* s, ||s||^2
//   dot_partials   2           (t, s) and (t, t) in one pass
//   bcg_update_xr  8           x = (x + alpha phat) + omega shat, r = s - omega t, ||r||^2, (r~, r)
// -- 23 vector streams an iteration.  Each pass that reduces parks one partial per workgroup in a fixed
// order (dev_common.hpp park_partial) and a one-workgroup final pass sums them in a fixed order (no atomics:
// two solves are bitwise equal) and runs the reference's stopping decision (bicgstab_stop.hpp) on the device;
// once one stops, every later kernel of the solve returns at once (kernels.hpp, LoopCtl).
#include "vec_pass.hpp"
#include "bicgstab_stop.hpp"

#include <algorithm>

namespace ecm2
{
namespace
{
using namespace dev;
using kern::LoopCtl;
using kern::BcgScal;
using kern::BcgFinal;

// The read-only reductions are kern::dot_partials' flat grid of contiguous chunks (k_pcg.hip); the direction is a
// flat grid with a pair per thread; the passes that write vectors and park partials take k_pcg_step_r's grid-stride
// form over kBlocks workgroups (see the comment there).  Each states its arithmetic once (vec_pass.hpp).
constexpr int kBlocks = 1024;

// The direction (solvers.cpp:1676-1693): it == 1 copies r; else beta = (rho_1 / rho_2) (alpha / omega),
// p = p - omega v, p = r + beta p; then phat = M^{-1} p.  Reads p, v, r, dinv; writes p, phat.
__global__ void __launch_bounds__(256)
k_bcg_update_p(int n, int it, const BcgScal *__restrict__ sc, double *__restrict__ p, const double *__restrict__ v,
               const double *__restrict__ r, const double *__restrict__ dinv, double *__restrict__ phat,
               const LoopCtl *ctl)
{
   const Flat w(n);
   if (w.t > w.n2 || ctl->done) { return; }
   const bool first = it == 1;
   const double omega = first ? 0.0 : sc->omega;
   const double beta = first ? 0.0 : (sc->rho1 / sc->rho2) * (sc->alpha / omega);
   each_entry(w, n, [&](auto k) {
      auto pn = ld(r, k);
      if (!first)
      {
         const auto t = ld(p, k) + (-omega) * ld(v, k);
         pn = pn + beta * t;
      }
      st(p, k, pn);
      st(phat, k, dinv ? ld(dinv, k) * pn : pn);
   });
}

// The first half step (solvers.cpp:1695-1730): alpha = rho_1 / (r~, v); s = r - alpha v, written into
// r's storage (r is not read again: the reference's r = s - omega t overwrites it); shat = M^{-1} s
// (without dinv s itself serves); the partials of ||s||^2.  Reads r, v, dinv; writes r, shat.
__global__ void __launch_bounds__(256)
k_bcg_update_s(int n, BcgScal *sc, double *__restrict__ r, const double *__restrict__ v,
               const double *__restrict__ dinv, double *__restrict__ shat, double *__restrict__ partials,
               const LoopCtl *ctl)
{
   if (ctl->done) { return; }
   __shared__ double red[4];
   const double alpha = sc->rho1 / sc->rtv;
   double s = 0.0;
   each_entry(Sweep(n), n, [&](auto k) {
      const auto sn = ld(r, k) + (-alpha) * ld(v, k);
      st(r, k, sn);
      if (dinv) { st(shat, k, ld(dinv, k) * sn); }
      dot_acc(s, sn, sn);
   });
   park_partial(s, partials, red);
   // (every thread has read rho1 and rtv; nothing in this kernel reads alpha)
   if (blockIdx.x == 0 && threadIdx.x == 0) { sc->alpha = alpha; }
}

// The second half step (solvers.cpp:1732-1738): omega = (t, s) / (t, t); x += alpha phat; x += omega shat;
// r = s - omega t (s lives in r's storage; shat null: shat = s); the partials of ||r||^2 and of the next
// iteration's rho_1 = (r~, r).  Reads x, phat, shat, r, t, r~; writes x, r.
__global__ void __launch_bounds__(256)
k_bcg_update_xr(int n, BcgScal *sc, double *__restrict__ x, const double *__restrict__ phat, const double *shat,
                double *r, const double *__restrict__ tv, const double *__restrict__ rt, int np,
                double *__restrict__ partials, const LoopCtl *ctl)
{
   if (ctl->done) { return; }
   __shared__ double red[8];
   const double alpha = sc->alpha, omega = sc->ts / sc->tt;
   double s0 = 0.0, s1 = 0.0;
   each_entry(Sweep(n), n, [&](auto k) {
      const auto sv = ld(r, k);
      const auto sh = shat ? ld(shat, k) : sv;
      const auto xa = ld(x, k) + alpha * ld(phat, k);
      st(x, k, xa + omega * sh);
      const auto rn = sv + (-omega) * ld(tv, k);
      st(r, k, rn);
      dot_acc(s0, rn, rn);
      dot_acc(s1, ld(rt, k), rn);
   });
   park_partial(s0, partials, red);
   park_partial(s1, partials + np, red + 4);
   if (blockIdx.x == 0 && threadIdx.x == 0) { sc->omega = omega; }
}

// After the loop: x += alpha phat when it stopped at a ||s|| test (solvers.cpp:1699-1701).
__global__ void k_bcg_finish_x(int n, const BcgScal *__restrict__ sc, const double *__restrict__ phat,
                               double *__restrict__ x, const LoopCtl *ctl)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n || ctl->done != BCG_CONVERGED_S) { return; }
   x[i] = x[i] + sc->alpha * phat[i];
}

// ---- the final pass: one workgroup sums 1-2 partial lists in a fixed order (sum_partials_fixed) and decides ----
__global__ void __launch_bounds__(kFinalThreads)
k_bcg_final(int nparts, int np, const double *__restrict__ partials, BcgFinal f)
{
   if (f.ctl->done) { return; }
   constexpr int NW = kFinalThreads / 64;
   __shared__ double red[2 * NW];
   const bool two = f.mode == kern::BCG_FINAL_DOT2 || f.mode == kern::BCG_FINAL_R;
   const double v0 = sum_partials_fixed(nparts, partials, red);
   const double v1 = two ? sum_partials_fixed(nparts, partials + np, red + NW) : 0.0;
   if (threadIdx.x != 0) { return; }
   BcgScal *sc = f.sc;
   if (f.mode == kern::BCG_FINAL_DOT)
   {
      *f.out = v0;
      if (f.hout) { *f.hout = v0; }
   }
   else if (f.mode == kern::BCG_FINAL_DOT2)
   {
      sc->ts = v0;
      sc->tt = v1;
   }
   else if (f.mode == kern::BCG_FINAL_S)
   {
      const double resid = sqrt(v0);
      sc->resid = resid;
      const int done = bcg_stop(BCG_TEST_S, resid, f.tol_goal, f.it, f.max_iter);
      if (done) { loop_set_done(f.ctl, f.host, done, f.it, resid); }
   }
   else
   {
      const double resid = sqrt(v0);
      sc->resid = resid;
      int done = bcg_stop(BCG_TEST_R, resid, f.tol_goal, f.it, f.max_iter);
      if (!done) { done = bcg_stop(BCG_TEST_OMEGA, sc->omega, f.tol_goal, f.it, f.max_iter); }
      int iters = done == BCG_MAX_ITER ? f.max_iter : f.it;
      if (!done)
      {
         // rho_2 = rho_1 (:1737) and the next iteration's rho_1 with its test (:1652-1675: final_iter = it + 1,
         // final_norm = this iteration's ||r||)
         sc->rho2 = sc->rho1;
         sc->rho1 = v1;
         done = bcg_stop(BCG_TEST_RHO, v1, f.tol_goal, f.it + 1, f.max_iter);
         iters = f.it + 1;
      }
      if (done) { loop_set_done(f.ctl, f.host, done, iters, resid); }
      loop_mark_checked(f.host, f.it);
   }
}

} // namespace

namespace kern
{

int bcg_parts(int n) { return std::max(kBlocks, step_parts(n)); }

static void bcg_final(int nparts, int n, const double *partials, const BcgFinal &f, hipStream_t s)
{
   hipLaunchKernelGGL(k_bcg_final, dim3(1), dim3(kFinalThreads), 0, s, nparts, bcg_parts(n), partials, f);
   ECM2_HIP(hipGetLastError());
}

void bcg_dot(int n, const double *a, const double *b, const double *c, double *partials, const BcgFinal &f, hipStream_t s)
{
   bcg_final(dot_partials(n, a, b, c, bcg_parts(n), partials, s, f.ctl), n, partials, f, s);
}

void bcg_update_p(int n, int it, const BcgScal *sc, double *p, const double *v, const double *r, const double *dinv,
                  double *phat, const LoopCtl *ctl, hipStream_t s)
{
   if (n == 0) { return; }
   hipLaunchKernelGGL(k_bcg_update_p, dim3(grid_for(n / 2 + 1, 256)), dim3(256), 0, s, n, it, sc, p, v, r, dinv, phat,
                      ctl);
   ECM2_HIP(hipGetLastError());
}

void bcg_update_s(int n, BcgScal *sc, double *r, const double *v, const double *dinv, double *shat, double *partials,
                  const BcgFinal &f, hipStream_t s)
{
   hipLaunchKernelGGL(k_bcg_update_s, dim3(kBlocks), dim3(256), 0, s, n, sc, r, v, dinv, shat, partials, f.ctl);
   ECM2_HIP(hipGetLastError());
   bcg_final(kBlocks, n, partials, f, s);
}

void bcg_update_xr(int n, BcgScal *sc, double *x, const double *phat, const double *shat, double *r, const double *t,
                   const double *rt, double *partials, const BcgFinal &f, hipStream_t s)
{
   hipLaunchKernelGGL(k_bcg_update_xr, dim3(kBlocks), dim3(256), 0, s, n, sc, x, phat, shat, r, t, rt, bcg_parts(n),
                      partials, f.ctl);
   ECM2_HIP(hipGetLastError());
   bcg_final(kBlocks, n, partials, f, s);
}

void bcg_finish_x(int n, const BcgScal *sc, const double *phat, double *x, const LoopCtl *ctl, hipStream_t s)
{
   if (n == 0) { return; }
   hipLaunchKernelGGL(k_bcg_finish_x, dim3(grid_for(n, 256)), dim3(256), 0, s, n, sc, phat, x, ctl);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
