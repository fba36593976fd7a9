// k_ess.hip -- the kernels of the essential-condition elimination (ConstrainedOperator::EliminateRHS,
// linalg/operator.cpp:559-584; Operator::FormLinearSystem, :114-129) for gfx950, beside the Mult and the list
// kernels of k_misc.hip (copy_values: the lift w[ess] = x[ess] and the overwrite b[ess] = x[ess]; gather_idx:
// buf = x[ess]).  Vector streams (FP64 vectors read or written) per pass:
//   ess_sub        3              b -= z          a 16-byte pass (vec_pass.hpp), flat, a pair per thread
//   ess_scatter    n_ess entries  x[ess] = buf    after gather_idx and the memset of x: X.SetSubVectorComplement(ess, 0.0)
// Nothing is summed here, so nothing depends on an order; the list is sorted and unique (no two threads write one
// entry).
#include "vec_pass.hpp"

namespace ecm2
{
namespace
{
using namespace dev;

__global__ void __launch_bounds__(256) k_ess_sub(int n, const double *__restrict__ z, double *__restrict__ b)
{
   const Flat w(n);
   each_entry(w, n, [&](auto k) { st(b, k, ld(b, k) - ld(z, k)); });
}

__global__ void k_ess_scatter(int n, const int *__restrict__ idx, const double *__restrict__ buf, double *__restrict__ x)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { x[idx[i]] = buf[i]; }
}

} // namespace

namespace kern
{

void ess_sub(int n, const double *z, double *b, hipStream_t s)
{
   if (n <= 0) { return; }
   hipLaunchKernelGGL(k_ess_sub, dim3(grid_for(n / 2 + 1, 256)), dim3(256), 0, s, n, z, b);
   ECM2_HIP(hipGetLastError());
}

void ess_scatter(int n, const int *idx, const double *buf, double *x, hipStream_t s)
{
   if (n <= 0) { return; }
   hipLaunchKernelGGL(k_ess_scatter, dim3(grid_for(n, 256)), dim3(256), 0, s, n, idx, buf, x);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
