// k_transfer.hip -- the transfer operator's two kernels for gfx950, for both kinds (p- and h-refinement), and the
// device operator around them (transfer.hpp).
//
// Reference:
//   TransferKernels::Prolongation3D     fem/transfer.cpp:2338-2423   (sum factorisation x, then y, then z)
//   TransferKernels::Restriction3D      fem/transfer.cpp:2470-2539   (z outer, y, x inner)
//   Mult / MultTranspose                fem/transfer.cpp:2542-2592   (gather, kernel, scatter)
//   ElementRestriction::BooleanMask     fem/restriction.cpp:248-283  (here: owner bits, tested in the kernel)
//   RefinementOperator::Mult            fem/fespace.cpp:1942-2019    (per fine element: lP of its embedding times the
//                                                                     parent's dofs, SetSubVector)
//   RefinementOperator::MultTranspose   fem/fespace.cpp:2021-2120    (`processed` marks, lP^T, AddElementVector)
//   GetLocalRefinementMatrices          fem/fespace.cpp:1786-1807    (here: B_oz (x) B_oy (x) B_ox, never formed)
//
// Both kernels are fused with their gathers and the prolongation with its scatter too: the only E-vector in HBM
// is the restriction's coarse one [units][Dc^3] -- a parent's eight children are summed inside the workgroup, so
// for the h kind it is 8x smaller than one row per fine element -- which kern::restriction_mult_transpose sums
// per coarse dof in ascending order over the plan's transposed map (no atomics: two calls are bitwise equal).
//
// Work mapping, one form for the ten (kind, orders): the unit of work is an element with itself as its one child
// (p kind, NCH = 1) or a parent with its eight children (h kind, NCH = 8).  A workgroup takes UPB consecutive
// units and first stages their gathered input dofs in LDS with all its threads -- consecutive threads read
// consecutive map entries (coalesced; the caller's [e][nd] maps as they are, no blocked copy), one gather each, and
// a fine entry its element does not own is not read at all.  A parent's Dc^3 coarse values are so gathered once
// and serve its eight children (prolongation), and its children's 8 Df^3 fine values are staged once
// (restriction).  Then one thread per (unit, child, output column): for the prolongation the Df^2 columns
// (qx, qy) of a child, each thread forming its column's sol_xy for dz = 0 .. Dc - 1 and adding it into its Df
// outputs along z; for the restriction the Dc^2 columns (dx, dy) likewise.  Per output entry these are the
// reference's sums in its order (the x sum, the y sum, the z sum, each ascending from 0.0); the x and y stages
// are recomputed per column instead of shared through a second LDS buffer (at most 170 multiply-adds per thread,
// against 125 LDS reads).  The thread's rows of B_ox and B_oy are picked from the kernel argument by
// compare-and-select (no runtime index into it), the z table's entries are constants of the unrolled loop
// selected by oz: scalar loads, no scratch.  With one child the octant is the constant 0, so the table selects
// fold away and the children table is not read.  The h restriction's per-child results go through a second LDS
// buffer and are added per coarse entry in ascending octant order; with one child the thread writes the coarse
// E-vector itself.  An LDS row's stride is padded to an odd number of doubles, so the rows a wave holds fall on
// distinct banks while the lanes of one row read one address (a broadcast).
#include "dev_common.hpp"
#include "transfer.hpp"

#include <algorithm>

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kXferLdsDoubles = 2048;  // at most 16 KiB of staged input per workgroup

__host__ __device__ constexpr int cube(int d) { return d * d * d; }
__host__ __device__ constexpr int odd(int n) { return n | 1; }  // an LDS row's stride
// units per workgroup: the columns of a unit's children fill at most 256 threads, the staged input (doubles per
// unit) at most kXferLdsDoubles; at least one unit
__host__ __device__ constexpr int xfer_upb(int nch, int cols, int staged)
{
   const int by_threads = 256 / (nch * cols), by_lds = kXferLdsDoubles / staged;
   const int u = by_threads < by_lds ? by_threads : by_lds;
   return u > 1 ? u : 1;
}
__host__ __device__ constexpr int xfer_threads(int nch, int cols, int staged)
{
   return (xfer_upb(nch, cols, staged) * nch * cols + 63) / 64 * 64;
}
__host__ __device__ constexpr int prolong_upb(int Dc, int Df, int nch) { return xfer_upb(nch, Df * Df, odd(cube(Dc))); }
__host__ __device__ constexpr int restrict_upb(int Dc, int Df, int nch) { return xfer_upb(nch, Dc * Dc, nch * odd(cube(Df))); }
// (the launch geometry every instantiation had when the two kinds were separate kernels)
static_assert(prolong_upb(2, 3, 1) == 28 && prolong_upb(2, 4, 1) == 16 && prolong_upb(2, 5, 1) == 10 &&
              prolong_upb(3, 4, 1) == 16 && prolong_upb(3, 5, 1) == 10 && prolong_upb(4, 5, 1) == 10, "p prolongation");
static_assert(restrict_upb(2, 3, 1) == 64 && restrict_upb(2, 4, 1) == 31 && restrict_upb(2, 5, 1) == 16 &&
              restrict_upb(3, 4, 1) == 28 && restrict_upb(3, 5, 1) == 16 && restrict_upb(4, 5, 1) == 16, "p restriction");
static_assert(prolong_upb(2, 2, 8) == 8 && prolong_upb(3, 3, 8) == 3 && prolong_upb(4, 4, 8) == 2 &&
              prolong_upb(5, 5, 8) == 1, "h prolongation");
static_assert(restrict_upb(2, 2, 8) == 8 && restrict_upb(3, 3, 8) == 3 && restrict_upb(4, 4, 8) == 2 &&
              restrict_upb(5, 5, 8) == 1, "h restriction");

// owner bit i of a fine element with N local dofs
template <int N>
__device__ __forceinline__ bool owns(uint64_t w0, uint64_t w1, int i)
{
   if (N <= 64) { return (w0 >> i) & 1; }
   return ((i < 64 ? w0 >> i : w1 >> (i - 64)) & 1) != 0;
}

// B[o][k] with k a constant of an unrolled loop; with one table there is nothing to select
template <int NT>
__device__ __forceinline__ double table_entry(const TransferBasis &b, int o, int k)
{
   if (NT == 1) { return b.B[0][k]; }
   return o ? b.B[1][k] : b.B[0][k];
}

// rows of the tables as registers: ra[d] = B[oa][qa + Df d], rb[d] = B[ob][qb + Df d]
template <int Dc, int Df, int NT>
__device__ __forceinline__ void pick_rows(const TransferBasis &b, int oa, int qa, int ob, int qb, double (&ra)[Dc],
                                          double (&rb)[Dc])
{
#pragma unroll
   for (int d = 0; d < Dc; d++)
   {
      ra[d] = rb[d] = 0.0;
#pragma unroll
      for (int o = 0; o < NT; o++)
      {
#pragma unroll
         for (int q = 0; q < Df; q++)
         {
            const double v = b.B[o][q + Df * d];
            ra[d] = (o == oa && q == qa) ? v : ra[d];
            rb[d] = (o == ob && q == qb) ? v : rb[d];
         }
      }
   }
}
// columns: ca[q] = B[oa][q + Df da], cb[q] = B[ob][q + Df db]
template <int Dc, int Df, int NT>
__device__ __forceinline__ void pick_cols(const TransferBasis &b, int oa, int da, int ob, int db, double (&ca)[Df],
                                          double (&cb)[Df])
{
#pragma unroll
   for (int q = 0; q < Df; q++)
   {
      ca[q] = cb[q] = 0.0;
#pragma unroll
      for (int o = 0; o < NT; o++)
      {
#pragma unroll
         for (int d = 0; d < Dc; d++)
         {
            const double v = b.B[o][q + Df * d];
            ca[q] = (o == oa && d == da) ? v : ca[q];
            cb[q] = (o == ob && d == db) ? v : cb[q];
         }
      }
   }
}

// Stages `rows` rows of N gathered values x[g[elem][.]] at stride LS.  CPR rows per unit: row r is element u0 + r
// (CPR == 1) or child r of the workgroup's units, children[8 u0 + r] (CPR == 8).  MASKED: an entry its element does
// not own is 0 and is not read.
template <int N, int LS, int CPR, bool MASKED>
__device__ __forceinline__ void stage(double *sx, long u0, int rows, const int *__restrict__ children,
                                      const int *__restrict__ g, const uint64_t *__restrict__ owner,
                                      const double *__restrict__ x)
{
   for (int k = threadIdx.x; k < rows * N; k += blockDim.x)
   {
      const int r = k / N, i = k % N;
      const long e = CPR == 1 ? u0 + r : children[u0 * CPR + r];
      const long at = CPR == 1 ? u0 * N + k : e * N + i;  // (= e N + i either way)
      bool read = true;
      if (MASKED) { read = owns<N>(owner[2 * e], owner[2 * e + 1], i); }
      sx[r * LS + i] = read ? x[g[at]] : 0.0;
   }
}

// One output column of the sum-factorised product: the input xe[ix + NI (iy + NI iz)], the x sum with bx, the y
// sum with by, and per input plane iz the z entry bz(o, iz) added into the column's NO outputs, which the caller
// has set to 0.0.  (Zeroing them here instead changes nothing in the arithmetic but the compiler's schedule: the
// h prolongations at p = 3, 4 then take 42 and 55 VGPRs instead of 70 and 120, and the p = 4 one is slower for it:
// DESIGN.md section 4g, profiles/transfer_unify_ab.txt.)
template <int NI, int NO, class BZ>
__device__ __forceinline__ void column(const double *xe, const double (&bx)[NI], const double (&by)[NI], BZ bz,
                                       double (&acc)[NO])
{
#pragma unroll
   for (int iz = 0; iz < NI; iz++)
   {
      double sxy = 0.0;
#pragma unroll
      for (int iy = 0; iy < NI; iy++)
      {
         double s1 = 0.0;
#pragma unroll
         for (int ix = 0; ix < NI; ix++) { s1 += bx[ix] * xe[ix + NI * (iy + NI * iz)]; }
         sxy += by[iy] * s1;
      }
#pragma unroll
      for (int o = 0; o < NO; o++) { acc[o] += bz(o, iz) * sxy; }
   }
}

// y_f[gf[f][i]] = (B_oz (x) B_oy (x) B_ox x_c[gc[unit]])_i where fine element f, child o of the unit, owns dof i
template <int Dc, int Df, int NCH>
__global__ void __launch_bounds__(xfer_threads(NCH, Df *Df, odd(cube(Dc))))
k_prolong(int nu, const int *__restrict__ gc, const int *__restrict__ gf, const int *__restrict__ children,
          const uint64_t *__restrict__ owner, const TransferBasis b, const double *__restrict__ x, double *__restrict__ y)
{
   constexpr int NC = cube(Dc), NF = cube(Df), COLS = Df * Df, TPU = NCH * COLS, LS = odd(NC), NT = NCH == 1 ? 1 : 2;
   constexpr int UPB = prolong_upb(Dc, Df, NCH);
   __shared__ double sx[UPB * LS];
   const long u0 = (long)blockIdx.x * UPB;
   const int nun = (int)(nu - u0 < UPB ? nu - u0 : UPB);  // (>= 1: the grid covers nu)
   // x_c[gc[unit][.]] of the workgroup's units, once for all their children
   stage<NC, LS, 1, false>(sx, u0, nun, nullptr, gc, nullptr, x);
   __syncthreads();
   const int lu = threadIdx.x / TPU, r = threadIdx.x % TPU;
   if (lu >= nun) { return; }
   const int oct = NCH == 1 ? 0 : r / COLS, col = r % COLS;
   const int ox = oct & 1, oy = (oct >> 1) & 1, oz = oct >> 2;
   const int qx = col % Df, qy = col / Df;
   double bx[Dc], by[Dc], acc[Df];
   pick_rows<Dc, Df, NT>(b, ox, qx, oy, qy, bx, by);
#pragma unroll
   for (int qz = 0; qz < Df; qz++) { acc[qz] = 0.0; }
   column<Dc, Df>(sx + lu * LS, bx, by, [&](int qz, int dz) { return table_entry<NT>(b, oz, qz + Df * dz); }, acc);
   // y *= mask and the scatter: the owner element alone writes the dof
   const long f = NCH == 1 ? u0 + lu : children[(u0 + lu) * NCH + oct];
   const uint64_t w0 = owner[2 * f], w1 = owner[2 * f + 1];
   const int *ge = gf + f * NF;
#pragma unroll
   for (int qz = 0; qz < Df; qz++)
   {
      const int i = col + COLS * qz;
      if (owns<NF>(w0, w1, i)) { y[ge[i]] = acc[qz]; }
   }
}

// ye[unit][a] = sum_o (B_oz^T (x) B_oy^T (x) B_ox^T (mask_f .* x_f[gf[f]]))_a, f child o of the unit, o ascending
template <int Dc, int Df, int NCH>
__global__ void __launch_bounds__(xfer_threads(NCH, Dc *Dc, NCH *odd(cube(Df))))
k_restrict(int nu, const int *__restrict__ gf, const int *__restrict__ children, const uint64_t *__restrict__ owner,
           const TransferBasis b, const double *__restrict__ x, double *__restrict__ ye)
{
   constexpr int NC = cube(Dc), NF = cube(Df), COLS = Dc * Dc, TPU = NCH * COLS, LS = odd(NF), LP = odd(NC);
   constexpr int NT = NCH == 1 ? 1 : 2, UPB = restrict_upb(Dc, Df, NCH);
   // sx: mask .* x_f of the units' children; sp (NCH > 1 only): every child's contribution to its unit's Dc^3 entries
   constexpr int SX = UPB * NCH * LS, SP = NCH == 1 ? 0 : UPB * NCH * LP;
   __shared__ double lds[SX + SP];
   double *sx = lds, *sp = lds + SX;
   const long u0 = (long)blockIdx.x * UPB;
   const int nun = (int)(nu - u0 < UPB ? nu - u0 : UPB);
   stage<NF, LS, NCH, true>(sx, u0, nun * NCH, children, gf, owner, x);
   __syncthreads();
   const int lu = threadIdx.x / TPU, r = threadIdx.x % TPU;
   if (lu < nun)
   {
      const int oct = NCH == 1 ? 0 : r / COLS, col = r % COLS;
      const int ox = oct & 1, oy = (oct >> 1) & 1, oz = oct >> 2;
      const int dx = col % Dc, dy = col / Dc;
      double btx[Df], bty[Df], acc[Dc];
      pick_cols<Dc, Df, NT>(b, ox, dx, oy, dy, btx, bty);
#pragma unroll
      for (int dz = 0; dz < Dc; dz++) { acc[dz] = 0.0; }
      column<Df, Dc>(sx + (lu * NCH + oct) * LS, btx, bty,
                     [&](int dz, int qz) { return table_entry<NT>(b, oz, qz + Df * dz); }, acc);
      double *out = NCH == 1 ? ye + (u0 + lu) * NC : sp + (lu * NCH + oct) * LP;
#pragma unroll
      for (int dz = 0; dz < Dc; dz++) { out[col + COLS * dz] = acc[dz]; }
   }
   if (NCH == 1) { return; }
   __syncthreads();
   // the unit's entry: its children in ascending octant order
   for (int k = threadIdx.x; k < nun * NC; k += blockDim.x)
   {
      const int ku = k / NC, a = k % NC;
      double v = sp[(ku * NCH) * LP + a];
#pragma unroll
      for (int o = 1; o < NCH; o++) { v += sp[(ku * NCH + o) * LP + a]; }
      ye[u0 * NC + k] = v;
   }
}

template <int Dc, int Df, int NCH>
void launch_prolong(int nu, const int *gc, const int *gf, const int *children, const uint64_t *owner,
                    const TransferBasis &b, const double *x, double *y, hipStream_t s)
{
   constexpr int UPB = prolong_upb(Dc, Df, NCH), T = xfer_threads(NCH, Df * Df, odd(cube(Dc)));
   hipLaunchKernelGGL((k_prolong<Dc, Df, NCH>), dim3(grid_for(nu, UPB)), dim3(T), 0, s, nu, gc, gf, children, owner, b, x, y);
   ECM2_HIP(hipGetLastError());
}

template <int Dc, int Df, int NCH>
void launch_restrict(int nu, const int *gf, const int *children, const uint64_t *owner, const TransferBasis &b,
                     const double *x, double *ye, hipStream_t s)
{
   constexpr int UPB = restrict_upb(Dc, Df, NCH), T = xfer_threads(NCH, Dc * Dc, NCH * odd(cube(Df)));
   hipLaunchKernelGGL((k_restrict<Dc, Df, NCH>), dim3(grid_for(nu, UPB)), dim3(T), 0, s, nu, gf, children, owner, b, x, ye);
   ECM2_HIP(hipGetLastError());
}

// The launchers of one (kind, pc, pf): the six pairs 1 <= pc < pf <= 4 of the p kind, the four orders of the h kind
struct Launchers
{
   decltype(&launch_prolong<2, 3, 1>) prolong;
   decltype(&launch_restrict<2, 3, 1>) restriction;
};

Launchers launchers_for(TransferKind kind, int pc, int pf)
{
#define X(KIND, PC, PF, NCH) \
   if (kind == KIND && pc == PC && pf == PF) { return {launch_prolong<PC + 1, PF + 1, NCH>, launch_restrict<PC + 1, PF + 1, NCH>}; }
   X(TRANSFER_P, 1, 2, 1) X(TRANSFER_P, 1, 3, 1) X(TRANSFER_P, 1, 4, 1) X(TRANSFER_P, 2, 3, 1) X(TRANSFER_P, 2, 4, 1)
   X(TRANSFER_P, 3, 4, 1) X(TRANSFER_H, 1, 1, 8) X(TRANSFER_H, 2, 2, 8) X(TRANSFER_H, 3, 3, 8) X(TRANSFER_H, 4, 4, 8)
#undef X
   ECM2_VERIFY(false, ERR_UNSUPPORTED,
               "no " << (kind == TRANSFER_H ? "h-" : "") << "transfer kernel for orders " << pc << " -> " << pf);
   return {};
}

} // namespace

// ---- the device operator ----
Transfer::Transfer(const TransferPlan &p, const int *gather_c, const int *gather_f)
   : kind_(p.kind), ne_c_(p.ne_c), ne_f_(p.ne_f), pc_(p.pc), pf_(p.pf), nc_(p.nc), nf_(p.nf), basis_(p.basis)
{
   require_device();
   const size_t ndc = cube(pc_ + 1), ndf = cube(pf_ + 1);
   gc_.upload(gather_c, ne_c_ * ndc);
   gf_.upload(gather_f, ne_f_ * ndf);
   children_.upload(p.children);
   owner_.upload(p.owner);
   c_off_.upload(p.c_off);
   c_idx_.upload(p.c_idx);
   ye_.resize(std::max<size_t>(ne_c_ * ndc, 1));
   ECM2_HIP(hipStreamSynchronize(nullptr));  // (the uploads read the plan's host vectors)
}

// (validated and planned on the host before anything is allocated on the device)
Transfer Transfer::p_refinement(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f)
{
   return Transfer(build_transfer_plan(ne, pc, nc, gather_c, pf, nf, gather_f), gather_c, gather_f);
}

Transfer Transfer::h_refinement(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                                const int *parent, const int *octant)
{
   return Transfer(build_htransfer_plan(p, ne_c, nc, gather_c, ne_f, nf, gather_f, parent, octant), gather_c, gather_f);
}

size_t Transfer::plan_bytes() const
{
   return gc_.bytes() + gf_.bytes() + children_.bytes() + owner_.bytes() + c_off_.bytes() + c_idx_.bytes();
}

void Transfer::mult(const double *x_c, double *y_f, hipStream_t s) const
{
   if (ne_c_ == 0) { return; }
   launchers_for(kind_, pc_, pf_).prolong(ne_c_, gc_.data(), gf_.data(), children_.data(), owner_.data(), basis_, x_c, y_f, s);
}

void Transfer::mult_transpose(const double *x_f, double *y_c, hipStream_t s) const
{
   if (ne_c_ != 0)
   {
      launchers_for(kind_, pc_, pf_).restriction(ne_c_, gf_.data(), children_.data(), owner_.data(), basis_, x_f, ye_.data(), s);
   }
   kern::restriction_mult_transpose(nc_, cube(pc_ + 1), c_off_.data(), c_idx_.data(), ye_.data(), y_c, s);
}

} // namespace ecm2
