// k_bicgstab.hip -- the vector passes of the device BiCGSTAB (gfx950): BiCGSTABSolver::Mult's iteration
// (linalg/solvers.cpp:1650-1784) around its two Mults, fused into five passes of 16-byte accesses
//   bcg_update_p   6 streams   p = r + beta (p - omega v), phat = dinv .* p
//   bcg_dot        2           (r~, v)
//   bcg_update_s   5           s = r - alpha v (into r), shat = dinv .* s, ||s||^2
//   bcg_dot        2           (t, s) and (t, t) in one pass
//   bcg_update_xr  8           x = (x + alpha phat) + omega shat, r = s - omega t, ||r||^2, (r~, r)
// -- 23 vector streams an iteration.  Each pass that reduces parks one partial per workgroup in a fixed
// order (dev_common.hpp park_partial) and a one-workgroup final pass sums them in a fixed order (no atomics:
// two solves are bitwise equal) and runs the reference's stopping decision (bicgstab_stop.hpp) on the device;
// once one stops, every later kernel of the solve returns at once (kernels.hpp, LoopCtl).
#include "dev_common.hpp"
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

// The read-only reductions take k_dot_partial's flat grid of contiguous chunks (workgroup b sums pairs
// [b kChunk, (b + 1) kChunk)); the passes that write vectors and park partials take k_pcg_step_r's
// grid-stride form over kBlocks workgroups (see the comment there).
constexpr int kK = 4, kChunk = 256 * kK, kBlocks = 1024;

// lists 0 and 1 (stride np): the partials of (a, b) and, with c, of (a, c); c == a: a read once
__global__ void __launch_bounds__(256)
k_bcg_dot(int n, const double *__restrict__ a, const double *__restrict__ b, const double *c, int np,
          double *__restrict__ partials, const LoopCtl *ctl)
{
   if (ctl->done) { return; }  // (wave-uniform)
   __shared__ double red[8];
   double s0 = 0.0, s1 = 0.0;
   const long n2 = n / 2, base = (long)blockIdx.x * kChunk + threadIdx.x;
   const v2d *a2 = reinterpret_cast<const v2d *>(a), *b2 = reinterpret_cast<const v2d *>(b);
   const v2d *c2 = reinterpret_cast<const v2d *>(c);
   const bool self = c == a;
#pragma unroll
   for (int k = 0; k < kK; k++)
   {
      const long i = base + 256 * k;
      if (i < n2)
      {
         const v2d u = a2[i], v = b2[i];
         s0 += u.x * v.x;
         s0 += u.y * v.y;
         if (c)
         {
            const v2d w = self ? u : c2[i];
            s1 += u.x * w.x;
            s1 += u.y * w.y;
         }
      }
   }
   if ((n & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255)
   {
      s0 += a[n - 1] * b[n - 1];
      if (c) { s1 += a[n - 1] * c[n - 1]; }
   }
   park_partial(s0, partials, red);
   if (c) { park_partial(s1, partials + np, red + 4); }
}

// The direction (solvers.cpp:1676-1693): it == 1 copies r; else beta = (rho_1 / rho_2) (alpha / omega),
// p = p - omega v, p = r + beta p; then phat = M^{-1} p.  Reads p, v, r, dinv; writes p, phat.
__global__ void __launch_bounds__(256)
k_bcg_update_p(int n, int it, const BcgScal *__restrict__ sc, double *__restrict__ p, const double *__restrict__ v,
               const double *__restrict__ r, const double *__restrict__ dinv, double *__restrict__ phat,
               const LoopCtl *ctl)
{
   // entries 2i, 2i + 1 per lane (the last lane of an odd n takes the tail)
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, n2 = n / 2;
   if (i > n2 || ctl->done) { return; }
   const bool first = it == 1;
   const double omega = first ? 0.0 : sc->omega;
   const double beta = first ? 0.0 : (sc->rho1 / sc->rho2) * (sc->alpha / omega);
   if (i < n2)
   {
      v2d *p2 = reinterpret_cast<v2d *>(p), *h2 = reinterpret_cast<v2d *>(phat);
      const v2d *v2 = reinterpret_cast<const v2d *>(v), *r2 = reinterpret_cast<const v2d *>(r);
      const v2d *q2 = reinterpret_cast<const v2d *>(dinv);
      v2d pn = r2[i];
      if (!first)
      {
         const v2d t = p2[i] + (-omega) * v2[i];
         pn = pn + beta * t;
      }
      p2[i] = pn;
      h2[i] = dinv ? q2[i] * pn : pn;
   }
   else if (n & 1)
   {
      const long j = n - 1;
      double pn = r[j];
      if (!first)
      {
         const double t = p[j] + (-omega) * v[j];
         pn = pn + beta * t;
      }
      p[j] = pn;
      phat[j] = dinv ? dinv[j] * pn : pn;
   }
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
   const long n2 = n / 2, stride = (long)gridDim.x * blockDim.x, t = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const v2d *v2 = reinterpret_cast<const v2d *>(v), *q2 = reinterpret_cast<const v2d *>(dinv);
   v2d *r2 = reinterpret_cast<v2d *>(r), *h2 = reinterpret_cast<v2d *>(shat);
   for (long i = t; i < n2; i += stride)
   {
      const v2d sn = r2[i] + (-alpha) * v2[i];
      r2[i] = sn;
      if (dinv) { h2[i] = q2[i] * sn; }
      s += sn.x * sn.x;
      s += sn.y * sn.y;
   }
   if ((n & 1) && t == stride - 1)  // the odd tail
   {
      const long i = n - 1;
      const double sn = r[i] + (-alpha) * v[i];
      r[i] = sn;
      if (dinv) { shat[i] = dinv[i] * sn; }
      s += sn * sn;
   }
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
   const long n2 = n / 2, stride = (long)gridDim.x * blockDim.x, t = (long)blockIdx.x * blockDim.x + threadIdx.x;
   const v2d *ph2 = reinterpret_cast<const v2d *>(phat), *sh2 = reinterpret_cast<const v2d *>(shat);
   const v2d *t2 = reinterpret_cast<const v2d *>(tv), *rt2 = reinterpret_cast<const v2d *>(rt);
   v2d *x2 = reinterpret_cast<v2d *>(x), *r2 = reinterpret_cast<v2d *>(r);
   for (long i = t; i < n2; i += stride)
   {
      const v2d sv = r2[i];
      const v2d sh = shat ? sh2[i] : sv;
      const v2d xa = x2[i] + alpha * ph2[i];
      x2[i] = xa + omega * sh;
      const v2d rn = sv + (-omega) * t2[i];
      r2[i] = rn;
      const v2d w = rt2[i];
      s0 += rn.x * rn.x;
      s0 += rn.y * rn.y;
      s1 += w.x * rn.x;
      s1 += w.y * rn.y;
   }
   if ((n & 1) && t == stride - 1)  // the odd tail
   {
      const long i = n - 1;
      const double sv = r[i];
      const double sh = shat ? shat[i] : sv;
      const double xa = x[i] + alpha * phat[i];
      x[i] = xa + omega * sh;
      const double rn = sv + (-omega) * tv[i];
      r[i] = rn;
      s0 += rn * rn;
      s1 += rt[i] * rn;
   }
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

int bcg_parts(int n) { return std::max(kBlocks, std::max(1, (int)((n / 2 + kChunk - 1) / kChunk))); }

static void bcg_final(int nparts, int n, const double *partials, const BcgFinal &f, hipStream_t s)
{
   hipLaunchKernelGGL(k_bcg_final, dim3(1), dim3(kFinalThreads), 0, s, nparts, bcg_parts(n), partials, f);
   ECM2_HIP(hipGetLastError());
}

void bcg_dot(int n, const double *a, const double *b, const double *c, double *partials, const BcgFinal &f, hipStream_t s)
{
   const int nb = std::max(1, (int)((n / 2 + kChunk - 1) / kChunk));
   hipLaunchKernelGGL(k_bcg_dot, dim3(nb), dim3(256), 0, s, n, a, b, c, bcg_parts(n), partials, f.ctl);
   ECM2_HIP(hipGetLastError());
   bcg_final(nb, n, partials, f, s);
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
