// k_mg.hip -- the vector passes of the multigrid cycle (MultigridBase::SmoothingStep and Cycle,
// fem/multigrid.cpp:147-232) and of the PCG that takes the cycle as its preconditioner (CGSolver::Mult,
// linalg/solvers.cpp:869-1004), for gfx950.  Vector streams (FP64 vectors read or written) per pass:
//   mg_residual    3   r = x - h                 (h = A~ y: R = X, then AddMult(Y, R, -1), in one pass)
//   mg_add         3   y += z                    (the smoother's correction, the prolonged coarse correction)
//   mg_pcg_step_r  3   r -= alpha (A d)          (alpha = nom / den -> *alpha_out; x += alpha d is deferred to
//                                                 kern::pcg_update_xd_z / pcg_finish_x as in k_pcg_step_r_prec)
// All in k_cheb.hip's form: 16-byte accesses, the last thread takes an odd n's tail entry, a grid-stride loop over
// kDotPartials workgroups; nothing is summed here, so nothing depends on an order.
#include "dev_common.hpp"

namespace ecm2
{
namespace
{
using namespace dev;
using kern::LoopCtl;

constexpr int kBlocks = kern::kDotPartials;

__global__ void __launch_bounds__(256)
k_mg_residual(int n, const double *__restrict__ x, const double *__restrict__ h, double *__restrict__ r)
{
   const Sweep w(n);
   const v2d *x2 = as2(x), *h2 = as2(h);
   v2d *r2 = as2(r);
   for (long i = w.t; i < w.n2; i += w.stride) { r2[i] = x2[i] - h2[i]; }
   if (w.tail) { r[n - 1] = x[n - 1] - h[n - 1]; }
}

__global__ void __launch_bounds__(256) k_mg_add(int n, const double *__restrict__ z, double *__restrict__ y)
{
   const Sweep w(n);
   const v2d *z2 = as2(z);
   v2d *y2 = as2(y);
   for (long i = w.t; i < w.n2; i += w.stride) { y2[i] = y2[i] + z2[i]; }
   if (w.tail) { y[n - 1] = y[n - 1] + z[n - 1]; }
}

__global__ void __launch_bounds__(256)
k_mg_pcg_step_r(int n, const double *__restrict__ nom, const double *__restrict__ den, const double *__restrict__ ap,
                double *__restrict__ r, double *__restrict__ alpha_out, const LoopCtl *ctl)
{
   if (ctl && ctl->done) { return; }  // (wave-uniform)
   const double alpha = *nom / *den;
   if (blockIdx.x == 0 && threadIdx.x == 0) { *alpha_out = alpha; }
   const Sweep w(n);
   const v2d *a2 = as2(ap);
   v2d *r2 = as2(r);
   for (long i = w.t; i < w.n2; i += w.stride) { r2[i] = r2[i] + (-alpha) * a2[i]; }
   if (w.tail) { r[n - 1] = r[n - 1] + (-alpha) * ap[n - 1]; }
}

} // namespace

namespace kern
{

void mg_residual(int n, const double *x, const double *h, double *r, hipStream_t s)
{
   hipLaunchKernelGGL(k_mg_residual, dim3(kBlocks), dim3(256), 0, s, n, x, h, r);
   ECM2_HIP(hipGetLastError());
}

void mg_add(int n, const double *z, double *y, hipStream_t s)
{
   hipLaunchKernelGGL(k_mg_add, dim3(kBlocks), dim3(256), 0, s, n, z, y);
   ECM2_HIP(hipGetLastError());
}

void mg_pcg_step_r(int n, const double *nom, const double *den, const double *ap, double *r, double *alpha, hipStream_t s,
                   const LoopCtl *ctl)
{
   hipLaunchKernelGGL(k_mg_pcg_step_r, dim3(kBlocks), dim3(256), 0, s, n, nom, den, ap, r, alpha, ctl);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
