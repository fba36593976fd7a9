// k_transfer.hip -- the p-refinement transfer operator's two kernels for gfx950 and the device operator around
// them (transfer.hpp).
//
// Reference:
//   TransferKernels::Prolongation3D   fem/transfer.cpp:2338-2423   (sum factorisation x, then y, then z)
//   TransferKernels::Restriction3D    fem/transfer.cpp:2470-2539   (z outer, y, x inner)
//   Mult / MultTranspose              fem/transfer.cpp:2542-2592   (gather, kernel, scatter)
//   ElementRestriction::BooleanMask   fem/restriction.cpp:248-283  (here: owner bits, tested in the kernel)
//
// Both kernels are fused with their gathers and the prolongation with its scatter too: the only E-vector in HBM
// is the restriction's coarse one, summed per coarse dof in ascending order by kern::restriction_mult_transpose
// over the plan's transposed map (no atomics: two calls are bitwise equal).
//
// Work mapping, one form for the six (Dc, Df): a workgroup takes EPB consecutive elements and first stages their
// gathered input dofs in LDS with all its threads -- consecutive threads read consecutive map entries (coalesced;
// the caller's [e][nd] maps as they are, no blocked copy), one gather each, and a fine entry the element does not
// own is not read at all.  Then one thread per (element, output column): for the prolongation the Df^2 columns
// (qx, qy) of an element, each thread forming its column's sol_xy for dz = 0 .. Dc - 1 and adding it into its Df
// outputs along z; for the restriction the Dc^2 columns (dx, dy) likewise.  Per output entry these are the
// reference's sums in its order (the x sum, the y sum, the z sum, each ascending); the x and y stages are
// recomputed per column instead of shared through a second LDS buffer (at most 170 multiply-adds per thread,
// against 125 LDS reads).  The thread's two rows of B are picked from the kernel argument by compare-and-select
// (no runtime index into it), the z stage's entries are constants of the unrolled loop: scalar loads, no scratch.
// The LDS image pads an element's stride to an odd number of doubles, so the elements a wave holds fall on
// distinct banks while the lanes of one element read one address (a broadcast).
#include "dev_common.hpp"
#include "transfer.hpp"

#include <algorithm>

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kXferLdsDoubles = 2048;  // at most 16 KiB of LDS per workgroup

__host__ __device__ constexpr int cube(int d) { return d * d * d; }
// elements per workgroup: columns fill at most 256 threads, the staged input at most kXferLdsDoubles
__host__ __device__ constexpr int xfer_epb(int cols, int nin)
{
   return (256 / cols) < (kXferLdsDoubles / (nin | 1)) ? (256 / cols) : (kXferLdsDoubles / (nin | 1));
}
__host__ __device__ constexpr int xfer_threads(int cols, int nin) { return (xfer_epb(cols, nin) * cols + 63) / 64 * 64; }

template <int Df>
__device__ __forceinline__ bool owns(uint64_t w0, uint64_t w1, int i)
{
   if (cube(Df) <= 64) { return (w0 >> i) & 1; }
   return ((i < 64 ? w0 >> i : w1 >> (i - 64)) & 1) != 0;
}

// rows q = qa and q = qb of B as registers: ra[d] = B[qa + Df d], rb[d] = B[qb + Df d]
template <int Dc, int Df>
__device__ __forceinline__ void pick_rows(const TransferBasis &b, int qa, int qb, double (&ra)[Dc], double (&rb)[Dc])
{
#pragma unroll
   for (int d = 0; d < Dc; d++)
   {
      ra[d] = rb[d] = 0.0;
#pragma unroll
      for (int q = 0; q < Df; q++)
      {
         const double v = b.B[q + Df * d];
         ra[d] = q == qa ? v : ra[d];
         rb[d] = q == qb ? v : rb[d];
      }
   }
}
// columns d = da and d = db of B: ca[q] = B[q + Df da], cb[q] = B[q + Df db]
template <int Dc, int Df>
__device__ __forceinline__ void pick_cols(const TransferBasis &b, int da, int db, double (&ca)[Df], double (&cb)[Df])
{
#pragma unroll
   for (int q = 0; q < Df; q++)
   {
      ca[q] = cb[q] = 0.0;
#pragma unroll
      for (int d = 0; d < Dc; d++)
      {
         const double v = b.B[q + Df * d];
         ca[q] = d == da ? v : ca[q];
         cb[q] = d == db ? v : cb[q];
      }
   }
}

template <int Dc, int Df>
__global__ void __launch_bounds__(xfer_threads(Df *Df, cube(Dc)))
k_transfer_prolong(int ne, const int *__restrict__ gc, const int *__restrict__ gf, const uint64_t *__restrict__ owner,
                   const TransferBasis b, const double *__restrict__ x, double *__restrict__ y)
{
   constexpr int NC = cube(Dc), NF = cube(Df), COLS = Df * Df, LS = NC | 1;
   constexpr int EPB = xfer_epb(COLS, NC);
   __shared__ double sx[EPB * LS];
   const long e0 = (long)blockIdx.x * EPB;
   const int nel = (int)(ne - e0 < EPB ? ne - e0 : EPB);  // (>= 1: the grid covers ne)
   // stage x_c[gc[e][.]] of the workgroup's elements
   for (int k = threadIdx.x; k < nel * NC; k += blockDim.x)
   {
      sx[(k / NC) * LS + k % NC] = x[gc[e0 * NC + k]];
   }
   __syncthreads();
   const int le = threadIdx.x / COLS, col = threadIdx.x % COLS;
   if (le >= nel) { return; }
   const int qx = col % Df, qy = col / Df;
   double bx[Dc], by[Dc], acc[Df];
   pick_rows<Dc, Df>(b, qx, qy, bx, by);
   const double *xe = sx + le * LS;
#pragma unroll
   for (int qz = 0; qz < Df; qz++) { acc[qz] = 0.0; }
#pragma unroll
   for (int dz = 0; dz < Dc; dz++)
   {
      double sxy = 0.0;
#pragma unroll
      for (int dy = 0; dy < Dc; dy++)
      {
         double s1 = 0.0;
#pragma unroll
         for (int dx = 0; dx < Dc; dx++) { s1 += bx[dx] * xe[dx + Dc * (dy + Dc * dz)]; }
         sxy += by[dy] * s1;
      }
#pragma unroll
      for (int qz = 0; qz < Df; qz++) { acc[qz] += b.B[qz + Df * dz] * sxy; }
   }
   // y *= mask and the scatter: the owner element alone writes the dof
   const long e = e0 + le;
   const uint64_t w0 = owner[2 * e], w1 = owner[2 * e + 1];
   const int *ge = gf + e * NF;
#pragma unroll
   for (int qz = 0; qz < Df; qz++)
   {
      const int i = col + COLS * qz;
      if (owns<Df>(w0, w1, i)) { y[ge[i]] = acc[qz]; }
   }
}

template <int Dc, int Df>
__global__ void __launch_bounds__(xfer_threads(Dc *Dc, cube(Df)))
k_transfer_restrict(int ne, const int *__restrict__ gf, const uint64_t *__restrict__ owner, const TransferBasis b,
                    const double *__restrict__ x, double *__restrict__ ye)
{
   constexpr int NC = cube(Dc), NF = cube(Df), COLS = Dc * Dc, LS = NF | 1;
   constexpr int EPB = xfer_epb(COLS, NF);
   __shared__ double sx[EPB * LS];
   const long e0 = (long)blockIdx.x * EPB;
   const int nel = (int)(ne - e0 < EPB ? ne - e0 : EPB);
   // stage mask .* x_f[gf[e][.]]: an entry the element does not own is 0 and is not read
   for (int k = threadIdx.x; k < nel * NF; k += blockDim.x)
   {
      const int le = k / NF, i = k % NF;
      const uint64_t w0 = owner[2 * (e0 + le)], w1 = owner[2 * (e0 + le) + 1];
      sx[le * LS + i] = owns<Df>(w0, w1, i) ? x[gf[e0 * NF + k]] : 0.0;
   }
   __syncthreads();
   const int le = threadIdx.x / COLS, col = threadIdx.x % COLS;
   if (le >= nel) { return; }
   const int dx = col % Dc, dy = col / Dc;
   double btx[Df], bty[Df], acc[Dc];
   pick_cols<Dc, Df>(b, dx, dy, btx, bty);
   const double *xe = sx + le * LS;
#pragma unroll
   for (int dz = 0; dz < Dc; dz++) { acc[dz] = 0.0; }
#pragma unroll
   for (int qz = 0; qz < Df; qz++)
   {
      double sxy = 0.0;
#pragma unroll
      for (int qy = 0; qy < Df; qy++)
      {
         double s1 = 0.0;
#pragma unroll
         for (int qx = 0; qx < Df; qx++) { s1 += btx[qx] * xe[qx + Df * (qy + Df * qz)]; }
         sxy += bty[qy] * s1;
      }
#pragma unroll
      for (int dz = 0; dz < Dc; dz++) { acc[dz] += b.B[qz + Df * dz] * sxy; }
   }
   double *out = ye + (e0 + le) * NC;
#pragma unroll
   for (int dz = 0; dz < Dc; dz++) { out[col + COLS * dz] = acc[dz]; }
}

template <int Dc, int Df>
void launch_prolong(int ne, const int *gc, const int *gf, const uint64_t *owner, const TransferBasis &b, const double *x,
                    double *y, hipStream_t s)
{
   constexpr int EPB = xfer_epb(Df * Df, cube(Dc)), T = xfer_threads(Df * Df, cube(Dc));
   hipLaunchKernelGGL((k_transfer_prolong<Dc, Df>), dim3(grid_for(ne, EPB)), dim3(T), 0, s, ne, gc, gf, owner, b, x, y);
   ECM2_HIP(hipGetLastError());
}

template <int Dc, int Df>
void launch_restrict(int ne, const int *gf, const uint64_t *owner, const TransferBasis &b, const double *x, double *ye,
                     hipStream_t s)
{
   constexpr int EPB = xfer_epb(Dc * Dc, cube(Df)), T = xfer_threads(Dc * Dc, cube(Df));
   hipLaunchKernelGGL((k_transfer_restrict<Dc, Df>), dim3(grid_for(ne, EPB)), dim3(T), 0, s, ne, gf, owner, b, x, ye);
   ECM2_HIP(hipGetLastError());
}

// (Dc, Df) instantiated: the six pairs 1 <= pc < pf <= 4
bool has_transfer(int pc, int pf) { return pc >= 1 && pc < pf && pf <= kTransferMaxOrder; }

} // namespace

namespace kern
{

#define ECM2_XFER_PAIRS(X) X(1, 2) X(1, 3) X(1, 4) X(2, 3) X(2, 4) X(3, 4)

void transfer_prolong(int pc, int pf, int ne, const int *gc, const int *gf, const uint64_t *owner, const TransferBasis &b,
                      const double *x_c, double *y_f, hipStream_t s)
{
   ECM2_VERIFY(has_transfer(pc, pf), ERR_UNSUPPORTED, "no transfer kernel for orders " << pc << " -> " << pf);
   if (ne == 0) { return; }
#define X(PC, PF) \
   if (pc == PC && pf == PF) { return launch_prolong<PC + 1, PF + 1>(ne, gc, gf, owner, b, x_c, y_f, s); }
   ECM2_XFER_PAIRS(X)
#undef X
}

void transfer_restrict(int pc, int pf, int ne, const int *gf, const uint64_t *owner, const TransferBasis &b,
                       const double *x_f, double *ye, hipStream_t s)
{
   ECM2_VERIFY(has_transfer(pc, pf), ERR_UNSUPPORTED, "no transfer kernel for orders " << pc << " -> " << pf);
   if (ne == 0) { return; }
#define X(PC, PF) \
   if (pc == PC && pf == PF) { return launch_restrict<PC + 1, PF + 1>(ne, gf, owner, b, x_f, ye, s); }
   ECM2_XFER_PAIRS(X)
#undef X
}

} // namespace kern

// ---- the device operator ----
PTransfer::PTransfer(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f)
   : ne_(ne), pc_(pc), pf_(pf), nc_(nc), nf_(nf)
{
   // (validated and planned on the host before anything is allocated on the device)
   const TransferPlan p = build_transfer_plan(ne, pc, nc, gather_c, pf, nf, gather_f);
   require_device();
   basis_ = p.basis;
   const size_t ndc = (size_t)(pc + 1) * (pc + 1) * (pc + 1), ndf = (size_t)(pf + 1) * (pf + 1) * (pf + 1);
   gc_.upload(gather_c, ne * ndc);
   gf_.upload(gather_f, ne * ndf);
   owner_.upload(p.owner);
   c_off_.upload(p.c_off);
   c_idx_.upload(p.c_idx);
   ye_.resize(std::max<size_t>(ne * ndc, 1));
   ECM2_HIP(hipStreamSynchronize(nullptr));  // (the uploads read the plan's host vectors)
}

size_t PTransfer::plan_bytes() const
{
   return gc_.bytes() + gf_.bytes() + owner_.bytes() + c_off_.bytes() + c_idx_.bytes();
}

void PTransfer::mult(const double *x_c, double *y_f, hipStream_t s) const
{
   kern::transfer_prolong(pc_, pf_, ne_, gc_.data(), gf_.data(), owner_.data(), basis_, x_c, y_f, s);
}

void PTransfer::mult_transpose(const double *x_f, double *y_c, hipStream_t s) const
{
   kern::transfer_restrict(pc_, pf_, ne_, gf_.data(), owner_.data(), basis_, x_f, ye_.data(), s);
   kern::restriction_mult_transpose(nc_, (pc_ + 1) * (pc_ + 1) * (pc_ + 1), c_off_.data(), c_idx_.data(), ye_.data(),
                                    y_c, s);
}

} // namespace ecm2
