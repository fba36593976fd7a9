// k_htransfer.hip -- the h-refinement transfer operator's two kernels for gfx950 and the device operator around
// them (htransfer.hpp).
//
// Reference:
//   RefinementOperator::Mult            fem/fespace.cpp:1942-2019  (per fine element: lP of its embedding times the
//                                                                   parent's dofs, SetSubVector)
//   RefinementOperator::MultTranspose   fem/fespace.cpp:2021-2120  (`processed` marks, lP^T, AddElementVector)
//   GetLocalRefinementMatrices          fem/fespace.cpp:1786-1807  (here: B_oz (x) B_oy (x) B_ox, never formed)
//
// Both kernels are fused with their gathers and the prolongation with its scatter too: the only E-vector in HBM
// is the restriction's coarse one [ne_c][D^3] -- a parent's eight children are summed inside the workgroup, so it
// is 8x smaller than one row per fine element -- which kern::restriction_mult_transpose sums per coarse dof in
// ascending order over the plan's transposed map (no atomics: two calls are bitwise equal).
//
// Work mapping, k_transfer.hip's with the parent as the unit: a workgroup takes PPB consecutive parents, so a
// parent's D^3 coarse values are gathered once into LDS and serve its eight children (prolongation), and its
// children's 8 D^3 fine values are staged once (restriction); consecutive threads read consecutive map entries.
// Then one thread per (parent, octant, output column): the D^2 columns (qx, qy) of a child for the prolongation,
// (dx, dy) for the restriction, each thread forming its column's x and y sums per z plane and adding them into its
// D outputs along z -- per output entry the sums run x, then y, then z, each ascending.  The thread's rows of B_ox
// and B_oy are picked from the kernel argument by compare-and-select (no runtime index into it), the z table's
// entries are constants of the unrolled loop selected by oz: scalar loads, no scratch.  The restriction's per-child
// results go through a second LDS buffer and are added per coarse entry in ascending octant order.  LDS rows are
// padded to an odd number of doubles.
#include "dev_common.hpp"
#include "htransfer.hpp"

#include <algorithm>

namespace ecm2
{
namespace
{
using namespace dev;

__host__ __device__ constexpr int hx_cube(int d) { return d * d * d; }
// parents per workgroup: 8 D^2 threads per parent, at most 256 threads
__host__ __device__ constexpr int hx_ppb(int D) { return 256 / (8 * D * D) > 1 ? 256 / (8 * D * D) : 1; }
__host__ __device__ constexpr int hx_threads(int D) { return (hx_ppb(D) * 8 * D * D + 63) / 64 * 64; }

template <int D>
__device__ __forceinline__ bool hx_owns(uint64_t w0, uint64_t w1, int i)
{
   if (hx_cube(D) <= 64) { return (w0 >> i) & 1; }
   return ((i < 64 ? w0 >> i : w1 >> (i - 64)) & 1) != 0;
}

// rows of the octant's tables as registers: ra[d] = B[oa][qa + D d], rb[d] = B[ob][qb + D d]
template <int D>
__device__ __forceinline__ void hx_pick_rows(const HTransferBasis &b, int oa, int qa, int ob, int qb, double (&ra)[D],
                                             double (&rb)[D])
{
#pragma unroll
   for (int d = 0; d < D; d++)
   {
      ra[d] = rb[d] = 0.0;
#pragma unroll
      for (int o = 0; o < 2; o++)
      {
#pragma unroll
         for (int q = 0; q < D; q++)
         {
            const double v = b.B[o][q + D * d];
            ra[d] = (o == oa && q == qa) ? v : ra[d];
            rb[d] = (o == ob && q == qb) ? v : rb[d];
         }
      }
   }
}
// columns: ca[q] = B[oa][q + D da], cb[q] = B[ob][q + D db]
template <int D>
__device__ __forceinline__ void hx_pick_cols(const HTransferBasis &b, int oa, int da, int ob, int db, double (&ca)[D],
                                             double (&cb)[D])
{
#pragma unroll
   for (int q = 0; q < D; q++)
   {
      ca[q] = cb[q] = 0.0;
#pragma unroll
      for (int o = 0; o < 2; o++)
      {
#pragma unroll
         for (int d = 0; d < D; d++)
         {
            const double v = b.B[o][q + D * d];
            ca[q] = (o == oa && d == da) ? v : ca[q];
            cb[q] = (o == ob && d == db) ? v : cb[q];
         }
      }
   }
}

template <int D>
__global__ void __launch_bounds__(hx_threads(D))
k_htransfer_prolong(int ne_c, const int *__restrict__ gc, const int *__restrict__ gf, const int *__restrict__ children,
                    const uint64_t *__restrict__ owner, const HTransferBasis b, const double *__restrict__ x,
                    double *__restrict__ y)
{
   constexpr int ND = hx_cube(D), COLS = D * D, TPP = 8 * COLS, LS = ND | 1, PPB = hx_ppb(D);
   __shared__ double sx[PPB * LS];
   const long p0 = (long)blockIdx.x * PPB;
   const int npar = (int)(ne_c - p0 < PPB ? ne_c - p0 : PPB);  // (>= 1: the grid covers ne_c)
   // stage x_c[gc[parent][.]] of the workgroup's parents, once for their eight children
   for (int k = threadIdx.x; k < npar * ND; k += blockDim.x)
   {
      sx[(k / ND) * LS + k % ND] = x[gc[p0 * ND + k]];
   }
   __syncthreads();
   const int lp = threadIdx.x / TPP, r = threadIdx.x % TPP;
   if (lp >= npar) { return; }
   const int oct = r / COLS, col = r % COLS;
   const int ox = oct & 1, oy = (oct >> 1) & 1, oz = oct >> 2;
   const int qx = col % D, qy = col / D;
   double bx[D], by[D], acc[D];
   hx_pick_rows<D>(b, ox, qx, oy, qy, bx, by);
   const double *xe = sx + lp * LS;
#pragma unroll
   for (int qz = 0; qz < D; qz++) { acc[qz] = 0.0; }
#pragma unroll
   for (int dz = 0; dz < D; dz++)
   {
      double sxy = 0.0;
#pragma unroll
      for (int dy = 0; dy < D; dy++)
      {
         double s1 = 0.0;
#pragma unroll
         for (int dx = 0; dx < D; dx++) { s1 += bx[dx] * xe[dx + D * (dy + D * dz)]; }
         sxy += by[dy] * s1;
      }
#pragma unroll
      for (int qz = 0; qz < D; qz++) { acc[qz] += (oz ? b.B[1][qz + D * dz] : b.B[0][qz + D * dz]) * sxy; }
   }
   // y *= mask and the scatter: the owner element alone writes the dof
   const long f = children[(p0 + lp) * 8 + oct];
   const uint64_t w0 = owner[2 * f], w1 = owner[2 * f + 1];
   const int *ge = gf + f * ND;
#pragma unroll
   for (int qz = 0; qz < D; qz++)
   {
      const int i = col + COLS * qz;
      if (hx_owns<D>(w0, w1, i)) { y[ge[i]] = acc[qz]; }
   }
}

template <int D>
__global__ void __launch_bounds__(hx_threads(D))
k_htransfer_restrict(int ne_c, const int *__restrict__ gf, const int *__restrict__ children,
                     const uint64_t *__restrict__ owner, const HTransferBasis b, const double *__restrict__ x,
                     double *__restrict__ ye)
{
   constexpr int ND = hx_cube(D), COLS = D * D, TPP = 8 * COLS, LS = ND | 1, PPB = hx_ppb(D);
   __shared__ double sx[PPB * 8 * LS];  // mask .* x_f of the parents' children
   __shared__ double sp[PPB * 8 * LS];  // every child's contribution to its parent's D^3 entries
   const long p0 = (long)blockIdx.x * PPB;
   const int npar = (int)(ne_c - p0 < PPB ? ne_c - p0 : PPB);
   // stage mask .* x_f[gf[child][.]]: an entry the child does not own is 0 and is not read
   for (int k = threadIdx.x; k < npar * 8 * ND; k += blockDim.x)
   {
      const int lc = k / ND, i = k % ND;  // lc = 8 lp + octant
      const long f = children[p0 * 8 + lc];
      const uint64_t w0 = owner[2 * f], w1 = owner[2 * f + 1];
      sx[lc * LS + i] = hx_owns<D>(w0, w1, i) ? x[gf[f * ND + i]] : 0.0;
   }
   __syncthreads();
   const int lp = threadIdx.x / TPP, r = threadIdx.x % TPP;
   if (lp < npar)
   {
      const int oct = r / COLS, col = r % COLS;
      const int ox = oct & 1, oy = (oct >> 1) & 1, oz = oct >> 2;
      const int dx = col % D, dy = col / D;
      double btx[D], bty[D], acc[D];
      hx_pick_cols<D>(b, ox, dx, oy, dy, btx, bty);
      const double *xe = sx + (lp * 8 + oct) * LS;
#pragma unroll
      for (int dz = 0; dz < D; dz++) { acc[dz] = 0.0; }
#pragma unroll
      for (int qz = 0; qz < D; qz++)
      {
         double sxy = 0.0;
#pragma unroll
         for (int qy = 0; qy < D; qy++)
         {
            double s1 = 0.0;
#pragma unroll
            for (int qx = 0; qx < D; qx++) { s1 += btx[qx] * xe[qx + D * (qy + D * qz)]; }
            sxy += bty[qy] * s1;
         }
#pragma unroll
         for (int dz = 0; dz < D; dz++) { acc[dz] += (oz ? b.B[1][qz + D * dz] : b.B[0][qz + D * dz]) * sxy; }
      }
      double *out = sp + (lp * 8 + oct) * LS;
#pragma unroll
      for (int dz = 0; dz < D; dz++) { out[col + COLS * dz] = acc[dz]; }
   }
   __syncthreads();
   // the parent's entry: its eight children in ascending octant order
   for (int k = threadIdx.x; k < npar * ND; k += blockDim.x)
   {
      const int kp = k / ND, a = k % ND;
      double v = sp[(kp * 8) * LS + a];
#pragma unroll
      for (int o = 1; o < 8; o++) { v += sp[(kp * 8 + o) * LS + a]; }
      ye[p0 * ND + k] = v;
   }
}

template <int D>
void launch_hprolong(int ne_c, const int *gc, const int *gf, const int *children, const uint64_t *owner,
                     const HTransferBasis &b, const double *x, double *y, hipStream_t s)
{
   hipLaunchKernelGGL((k_htransfer_prolong<D>), dim3(grid_for(ne_c, hx_ppb(D))), dim3(hx_threads(D)), 0, s, ne_c, gc, gf,
                      children, owner, b, x, y);
   ECM2_HIP(hipGetLastError());
}

template <int D>
void launch_hrestrict(int ne_c, const int *gf, const int *children, const uint64_t *owner, const HTransferBasis &b,
                      const double *x, double *ye, hipStream_t s)
{
   hipLaunchKernelGGL((k_htransfer_restrict<D>), dim3(grid_for(ne_c, hx_ppb(D))), dim3(hx_threads(D)), 0, s, ne_c, gf,
                      children, owner, b, x, ye);
   ECM2_HIP(hipGetLastError());
}

} // namespace

namespace kern
{

#define ECM2_HXFER_ORDERS(X) X(1) X(2) X(3) X(4)

void htransfer_prolong(int p, int ne_c, const int *gc, const int *gf, const int *children, const uint64_t *owner,
                       const HTransferBasis &b, const double *x_c, double *y_f, hipStream_t s)
{
   ECM2_VERIFY(p >= 1 && p <= kTransferMaxOrder, ERR_UNSUPPORTED, "no h-transfer kernel for order " << p);
   if (ne_c == 0) { return; }
#define X(P) \
   if (p == P) { return launch_hprolong<P + 1>(ne_c, gc, gf, children, owner, b, x_c, y_f, s); }
   ECM2_HXFER_ORDERS(X)
#undef X
}

void htransfer_restrict(int p, int ne_c, const int *gf, const int *children, const uint64_t *owner,
                        const HTransferBasis &b, const double *x_f, double *ye, hipStream_t s)
{
   ECM2_VERIFY(p >= 1 && p <= kTransferMaxOrder, ERR_UNSUPPORTED, "no h-transfer kernel for order " << p);
   if (ne_c == 0) { return; }
#define X(P) \
   if (p == P) { return launch_hrestrict<P + 1>(ne_c, gf, children, owner, b, x_f, ye, s); }
   ECM2_HXFER_ORDERS(X)
#undef X
}

} // namespace kern

// ---- the device operator ----
HTransfer::HTransfer(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                     const int *parent, const int *octant)
   : p_(p), ne_c_(ne_c), ne_f_(ne_f), nc_(nc), nf_(nf)
{
   // (validated and planned on the host before anything is allocated on the device)
   const HTransferPlan pl = build_htransfer_plan(p, ne_c, nc, gather_c, ne_f, nf, gather_f, parent, octant);
   require_device();
   basis_ = pl.basis;
   const size_t nd = (size_t)(p + 1) * (p + 1) * (p + 1);
   gc_.upload(gather_c, ne_c * nd);
   gf_.upload(gather_f, ne_f * nd);
   children_.upload(pl.children);
   owner_.upload(pl.owner);
   c_off_.upload(pl.c_off);
   c_idx_.upload(pl.c_idx);
   ye_.resize(std::max<size_t>(ne_c * nd, 1));
   ECM2_HIP(hipStreamSynchronize(nullptr));  // (the uploads read the plan's host vectors)
}

size_t HTransfer::plan_bytes() const
{
   return gc_.bytes() + gf_.bytes() + children_.bytes() + owner_.bytes() + c_off_.bytes() + c_idx_.bytes();
}

void HTransfer::mult(const double *x_c, double *y_f, hipStream_t s) const
{
   kern::htransfer_prolong(p_, ne_c_, gc_.data(), gf_.data(), children_.data(), owner_.data(), basis_, x_c, y_f, s);
}

void HTransfer::mult_transpose(const double *x_f, double *y_c, hipStream_t s) const
{
   kern::htransfer_restrict(p_, ne_c_, gf_.data(), children_.data(), owner_.data(), basis_, x_f, ye_.data(), s);
   const int D = p_ + 1;
   kern::restriction_mult_transpose(nc_, D * D * D, c_off_.data(), c_idx_.data(), ye_.data(), y_c, s);
}

} // namespace ecm2
