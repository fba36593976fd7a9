// k_mg.hip -- the vector passes of the multigrid cycle (MultigridBase::SmoothingStep and Cycle,
// fem/multigrid.cpp:147-232), for gfx950.  Vector streams (FP64 vectors read or written) per pass:
//   mg_residual    3   r = x - h                 (h = A~ y: R = X, then AddMult(Y, R, -1), in one pass)
//   mg_add         3   y += z                    (the smoother's correction, the prolonged coarse correction)
// (The PCG that takes the cycle as its preconditioner: k_pcg.hip, k_pcg_step_r<PCG_STEP_ONLY>.)  Grid-stride sweeps of
// vec_pass.hpp over kDotPartials workgroups: 16-byte accesses, the last thread takes an odd n's tail entry with the
// same body; nothing is summed here, so nothing depends on an order.
#include "vec_pass.hpp"

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kBlocks = kern::kDotPartials;

__global__ void __launch_bounds__(256)
k_mg_residual(int n, const double *__restrict__ x, const double *__restrict__ h, double *__restrict__ r)
{
   each_entry(Sweep(n), n, [&](auto k) { st(r, k, ld(x, k) - ld(h, k)); });
}

__global__ void __launch_bounds__(256) k_mg_add(int n, const double *__restrict__ z, double *__restrict__ y)
{
   each_entry(Sweep(n), n, [&](auto k) { st(y, k, ld(y, k) + ld(z, k)); });
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

} // namespace kern
} // namespace ecm2
