// k_cheb.hip -- the vector passes of OperatorChebyshevSmoother (linalg/solvers.cpp:619-658), of the power
// method behind its eigenvalue estimate (PowerMethod::EstimateLargestEigenvalue, linalg/operator.cpp:871-928)
// and of the PCG that takes the smoother as its preconditioner (CGSolver::Mult, linalg/solvers.cpp:869-1004),
// for gfx950.  The smoother is y = sum_k c_k (D^-1 A~)^k D^-1 x; per entry the reference's operations in its
// order: t *= dinv, then y += c_k t.  Vector streams (FP64 vectors read or written) per pass:
//   cheb_first        4 (3 for the last term of order 1)   t = dinv .* x, y = c_0 t
//   cheb_accum        5 (4 last term; +1 with the r.y sum) t = dinv .* h, y += c_k t
//   pcg_step_r_prec   6 (5 at order 1)                     r -= alpha (A d), t = dinv .* r, z = c_0 t
//   pcg_update_xd_z   5                                    x += alpha d, d = z + beta d
//   cheb_power_pass   4                                    v1 = dinv .* h, (v0, v1), (v1, v1)
//   cheb_scale        2                                    v *= 1 / sqrt(norm)
// All in k_pcg_step_r's form (k_misc.hip): 16-byte accesses, the last thread takes an odd n's tail entry, a
// grid-stride loop over kBlocks workgroups; the passes that sum park one partial per workgroup in a fixed order
// (park_partial) for kern::dot_final -- no atomics, so two applications are bitwise equal; with a LoopCtl every
// kernel returns at once when the loop has stopped.
#include "dev_common.hpp"

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
   const Sweep w(n);
   const v2d *q2 = as2(dinv), *x2 = as2(x);
   v2d *t2 = as2(t), *y2 = as2(y);
   for (long i = w.t; i < w.n2; i += w.stride)
   {
      const v2d tv = x2[i] * q2[i];
      if (t) { t2[i] = tv; }
      y2[i] = c0 * tv;
   }
   if (w.tail)
   {
      const long i = n - 1;
      const double tv = x[i] * dinv[i];
      if (t) { t[i] = tv; }
      y[i] = c0 * tv;
   }
}

// t = dinv .* h (h = A~ t_prev; stored unless t is null: the last term), y += ck t; with r (the PCG's last
// term): the workgroup's partial of r.y
__global__ void __launch_bounds__(256)
k_cheb_accum(int n, const double *__restrict__ dinv, const double *__restrict__ h, double ck, double *__restrict__ t,
             double *__restrict__ y, const double *__restrict__ r, double *__restrict__ partials, const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }  // (wave-uniform)
   __shared__ double red[4];
   const Sweep w(n);
   const v2d *q2 = as2(dinv), *h2 = as2(h), *r2 = as2(r);
   v2d *t2 = as2(t), *y2 = as2(y);
   double s = 0.0;
   for (long i = w.t; i < w.n2; i += w.stride)
   {
      const v2d tv = h2[i] * q2[i];
      if (t) { t2[i] = tv; }
      const v2d yn = y2[i] + ck * tv;
      y2[i] = yn;
      if (r)
      {
         const v2d rv = r2[i];
         s += rv.x * yn.x;
         s += rv.y * yn.y;
      }
   }
   if (w.tail)
   {
      const long i = n - 1;
      const double tv = h[i] * dinv[i];
      if (t) { t[i] = tv; }
      const double yn = y[i] + ck * tv;
      y[i] = yn;
      if (r) { s += r[i] * yn; }
   }
   if (r) { park_partial(s, partials, red); }
}

// The residual half of CGSolver's update with the smoother's first term fused (solvers.cpp:930-947, :631-656):
// alpha = nom/den (-> *alpha_out); r -= alpha ap (ap holds A d); t = dinv .* r (stored unless null: order 1);
// z = c0 t; with `sum` (order 1: z is complete) the workgroup's partial of r.z.  x += alpha d is deferred to
// k_pcg_update_xd_z (or k_pcg_finish_x after the stop), as in k_pcg_step_r.
__global__ void __launch_bounds__(256)
k_pcg_step_r_prec(int n, const double *__restrict__ nom, const double *__restrict__ den, const double *__restrict__ ap,
                  double *__restrict__ r, const double *__restrict__ dinv, double c0, double *__restrict__ t,
                  double *__restrict__ z, double *__restrict__ partials, double *__restrict__ alpha_out, bool sum,
                  const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }
   __shared__ double red[4];
   const double alpha = *nom / *den;
   if (blockIdx.x == 0 && threadIdx.x == 0) { *alpha_out = alpha; }
   const Sweep w(n);
   const v2d *a2 = as2(ap), *q2 = as2(dinv);
   v2d *r2 = as2(r), *t2 = as2(t), *z2 = as2(z);
   double s = 0.0;
   for (long i = w.t; i < w.n2; i += w.stride)
   {
      const v2d rn = r2[i] + (-alpha) * a2[i];
      r2[i] = rn;
      const v2d tv = rn * q2[i];
      if (t) { t2[i] = tv; }
      const v2d zv = c0 * tv;
      z2[i] = zv;
      if (sum)
      {
         s += rn.x * zv.x;
         s += rn.y * zv.y;
      }
   }
   if (w.tail)
   {
      const long i = n - 1;
      const double rn = r[i] + (-alpha) * ap[i];
      r[i] = rn;
      const double tv = rn * dinv[i];
      if (t) { t[i] = tv; }
      const double zv = c0 * tv;
      z[i] = zv;
      if (sum) { s += rn * zv; }
   }
   if (sum) { park_partial(s, partials, red); }
}

// The direction half (solvers.cpp:930, 985-990) with the stored z = B r: x += alpha d (this iteration's
// alpha = nom/den), d = z + (betanom/nom) d.
__global__ void __launch_bounds__(256)
k_pcg_update_xd_z(int n, const double *__restrict__ nom, const double *__restrict__ den,
                  const double *__restrict__ betanom, double *__restrict__ x, double *__restrict__ d,
                  const double *__restrict__ z, const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }
   const double alpha = *nom / *den, beta = *betanom / *nom;
   const Sweep w(n);
   const v2d *z2 = as2(z);
   v2d *x2 = as2(x), *d2 = as2(d);
   for (long i = w.t; i < w.n2; i += w.stride)
   {
      const v2d dold = d2[i];
      x2[i] = x2[i] + alpha * dold;
      d2[i] = z2[i] + beta * dold;
   }
   if (w.tail)
   {
      const long i = n - 1;
      const double dold = d[i];
      x[i] = x[i] + alpha * dold;
      d[i] = z[i] + beta * dold;
   }
}

// One power step's pass: v1 = dinv .* h (h = A~ v0) with the partials of (v0, v1) at partials[0, kBlocks) and
// of (v1, v1) -- the next step's norm -- at partials[kBlocks, 2 kBlocks)
__global__ void __launch_bounds__(256)
k_cheb_power_pass(int n, const double *__restrict__ dinv, const double *__restrict__ h, const double *__restrict__ v0,
                  double *__restrict__ v1, double *__restrict__ partials)
{
   __shared__ double red0[4], red1[4];
   const Sweep w(n);
   const v2d *q2 = as2(dinv), *h2 = as2(h), *u2 = as2(v0);
   v2d *v2 = as2(v1);
   double s0 = 0.0, s1 = 0.0;
   for (long i = w.t; i < w.n2; i += w.stride)
   {
      const v2d v = h2[i] * q2[i], u = u2[i];
      v2[i] = v;
      s0 += u.x * v.x;
      s0 += u.y * v.y;
      s1 += v.x * v.x;
      s1 += v.y * v.y;
   }
   if (w.tail)
   {
      const long i = n - 1;
      const double v = h[i] * dinv[i];
      v1[i] = v;
      s0 += v0[i] * v;
      s1 += v * v;
   }
   park_partial(s0, partials, red0);
   park_partial(s1, partials + gridDim.x, red1);
}

// v0 /= sqrt(normV0) as Vector::operator/= does it: m = 1 / sqrt(*norm), v *= m
__global__ void __launch_bounds__(256) k_cheb_scale(int n, const double *__restrict__ norm, double *__restrict__ v)
{
   const double m = 1.0 / sqrt(*norm);
   const Sweep w(n);
   v2d *v2 = as2(v);
   for (long i = w.t; i < w.n2; i += w.stride) { v2[i] = v2[i] * m; }
   if (w.tail) { v[n - 1] = v[n - 1] * m; }
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

void pcg_step_r_prec(int n, const double *nom, const double *den, const double *ap, double *r, const double *dinv,
                     double c0, double *t, double *z, double *partials, double *alpha, bool sum, hipStream_t s,
                     const LoopCtl *ctl)
{
   hipLaunchKernelGGL(k_pcg_step_r_prec, dim3(kBlocks), dim3(256), 0, s, n, nom, den, ap, r, dinv, c0, t, z, partials,
                      alpha, sum, ctl);
   ECM2_HIP(hipGetLastError());
}

void pcg_update_xd_z(int n, const double *nom, const double *den, const double *betanom, double *x, double *d,
                     const double *z, hipStream_t s, const LoopCtl *ctl)
{
   hipLaunchKernelGGL(k_pcg_update_xd_z, dim3(kBlocks), dim3(256), 0, s, n, nom, den, betanom, x, d, z, ctl);
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
