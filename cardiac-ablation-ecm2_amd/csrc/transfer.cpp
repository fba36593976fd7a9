// transfer.cpp -- host construction of the transfer operator's plan (transfer.hpp), both kinds from shared pieces:
// the 1D tables (p: TensorProductPRefinementTransferOperator's constructor, fem/transfer.cpp:2223-2287; h:
// GetLocalRefinementMatrices, fem/fespace.cpp:1786-1807, in tensor form, with NodalLocalInterpolation's 1e-12
// threshold, fem/fe/fe_base.cpp:884-893), the owner bits (ElementRestriction::BooleanMask,
// fem/restriction.cpp:248-283; RefinementOperator::MultTranspose's `processed` marks, fem/fespace.cpp:2030-2085),
// the h kind's children table (CoarseFineTransformations::embeddings inverted) and the coarse space's transposed
// map.  Plain C++: also compiled into tests/cpp/transfer_plan_check.cpp's CPU program.
#include "transfer.hpp"

#include "fe.hpp"

#include <cmath>

namespace ecm2
{
namespace
{

// The pieces both builders are made of.  `pre` is the kind's message prefix ("transfer" or "h-transfer").

// (the transposed map indexes the coarse E-vector with ints, the kernels' staging loops the fine one)
void check_evector_size(const char *pre, int ne, int nd)
{
   ECM2_VERIFY((long)ne * nd <= 0x7fffffffL, ERR_UNSUPPORTED,
               pre << ": an E-vector of " << ne << " elements exceeds 2^31 entries");
}

// A map entry outside 0..ndofs - 1: the message and the code, out of line so that the loops over the maps' tens of
// millions of entries keep one compare per entry
[[noreturn]] void refuse_entry(const char *pre, const char *space, int g, int ndofs)
{
   ECM2_VERIFY(g >= 0, ERR_UNSUPPORTED, pre << ": signed entry " << g << " in the " << space << " map (H1 has none)");
   ECM2_VERIFY(false, ERR_ARG, pre << ": " << space << " map entry " << g << " >= ndofs " << ndofs);
   throw Error(ERR_INTERNAL, "unreachable");
}

inline void check_entry(const char *pre, const char *space, int g, int ndofs)
{
   if ((unsigned)g >= (unsigned)ndofs) { refuse_entry(pre, space, g, ndofs); }  // (negative, or >= ndofs >= 0)
}

void check_coarse_map(const char *pre, long n, const int *gather_c, int nc)
{
   for (long k = 0; k < n; k++) { check_entry(pre, "coarse", gather_c[k], nc); }
}

// The fine map's entries, and the owner of every fine dof: the lowest fine element that holds it (its first
// occurrence in the E-vector, BooleanMask's "first element" rule; the first to mark it `processed`)
std::vector<uint64_t> owner_bits(const char *pre, int ne, int nd, const int *gather_f, int nf)
{
   std::vector<char> seen((size_t)nf, 0);
   std::vector<uint64_t> owner((size_t)ne * 2, 0);
   long owned = 0;
   for (int e = 0; e < ne; e++)
   {
      for (int i = 0; i < nd; i++)
      {
         const int g = gather_f[(long)e * nd + i];
         check_entry(pre, "fine", g, nf);
         if (!seen[g])
         {
            seen[g] = 1;
            owned++;
            owner[(size_t)e * 2 + (i >> 6)] |= uint64_t(1) << (i & 63);
         }
      }
   }
   ECM2_VERIFY(owned == nf, ERR_ARG, pre << ": " << nf - owned << " fine dofs are held by no element");
   return owner;
}

// The coarse transposed map (counting sort: ascending E-vector entries within a row)
void transposed_map(long n, const int *gather_c, int nc, std::vector<int> &c_off, std::vector<int> &c_idx)
{
   c_off.assign((size_t)nc + 1, 0);
   for (long k = 0; k < n; k++) { c_off[gather_c[k] + 1]++; }
   for (int c = 0; c < nc; c++) { c_off[c + 1] += c_off[c]; }
   c_idx.resize((size_t)n);
   std::vector<int> fill(c_off.begin(), c_off.end() - 1);
   for (long k = 0; k < n; k++) { c_idx[fill[gather_c[k]]++] = (int)k; }
}

} // namespace

TransferBasis htransfer_basis(int p)
{
   ECM2_VERIFY(p >= 1 && p <= kTransferMaxOrder, ERR_UNSUPPORTED,
               "h-transfer: order " << p << " (kernels exist for 1 <= p <= " << kTransferMaxOrder << ")");
   TransferBasis b = {};
   const int D = p + 1;
   double xi[MAX_D1D], w[MAX_D1D], u[MAX_D1D], du[MAX_D1D];
   gauss_lobatto(D, xi, w);
   for (int o = 0; o < 2; o++)
   {
      for (int q = 0; q < D; q++)
      {
         basis_eval(p, xi, 0.5 * (o + xi[q]), u, du);
         for (int d = 0; d < D; d++) { b.B[o][q + D * d] = std::fabs(u[d]) < kHTransferZero ? 0.0 : u[d]; }
      }
   }
   return b;
}

TransferPlan build_transfer_plan(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f)
{
   const char *pre = "transfer";
   ECM2_VERIFY(pc < pf, ERR_ARG, "transfer: the coarse order " << pc << " must be below the fine order " << pf);
   ECM2_VERIFY(pc >= 1 && pf <= kTransferMaxOrder, ERR_UNSUPPORTED,
               "transfer: orders " << pc << " -> " << pf << " (kernels exist for 1 <= pc < pf <= " << kTransferMaxOrder << ")");
   ECM2_VERIFY(ne >= 0 && nc >= 0 && nf >= 0, ERR_ARG, "transfer: negative size");
   ECM2_VERIFY(ne == 0 || (gather_c && gather_f), ERR_ARG, "transfer: null gather map");
   const int Dc = pc + 1, Df = pf + 1, ndc = Dc * Dc * Dc, ndf = Df * Df * Df;
   check_evector_size(pre, ne, ndc);
   check_evector_size(pre, ne, ndf);
   TransferPlan p;
   p.kind = TRANSFER_P;
   p.ne_c = p.ne_f = ne; p.pc = pc; p.pf = pf; p.nc = nc; p.nf = nf;
   // B[0][q + Df d]: coarse basis function d at fine node q
   double xc[MAX_D1D], xf[MAX_D1D], w[MAX_D1D], u[MAX_D1D], du[MAX_D1D];
   gauss_lobatto(Dc, xc, w);
   gauss_lobatto(Df, xf, w);
   for (int q = 0; q < Df; q++)
   {
      basis_eval(pc, xc, xf[q], u, du);
      for (int d = 0; d < Dc; d++) { p.basis.B[0][q + Df * d] = u[d]; }
   }
   check_coarse_map(pre, (long)ne * ndc, gather_c, nc);
   p.owner = owner_bits(pre, ne, ndf, gather_f, nf);
   transposed_map((long)ne * ndc, gather_c, nc, p.c_off, p.c_idx);
   return p;
}

TransferPlan build_htransfer_plan(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                                  const int *parent, const int *octant)
{
   const char *pre = "h-transfer";
   TransferPlan pl;
   pl.basis = htransfer_basis(p);  // (refuses the order)
   ECM2_VERIFY(ne_c >= 0 && ne_f >= 0 && nc >= 0 && nf >= 0, ERR_ARG, "h-transfer: negative size");
   ECM2_VERIFY(ne_c == 0 || gather_c, ERR_ARG, "h-transfer: null coarse gather map");
   ECM2_VERIFY(ne_f == 0 || (gather_f && parent && octant), ERR_ARG, "h-transfer: null fine gather map or embedding");
   const int D = p + 1, nd = D * D * D;
   check_evector_size(pre, ne_f, nd);
   pl.kind = TRANSFER_H;
   pl.ne_c = ne_c; pl.ne_f = ne_f; pl.pc = pl.pf = p; pl.nc = nc; pl.nf = nf;
   check_coarse_map(pre, (long)ne_c * nd, gather_c, nc);
   pl.owner = owner_bits(pre, ne_f, nd, gather_f, nf);
   // the embedding inverted: one child per octant of every parent
   pl.children.assign((size_t)ne_c * 8, -1);
   for (int f = 0; f < ne_f; f++)
   {
      ECM2_VERIFY(parent[f] >= 0 && parent[f] < ne_c, ERR_ARG,
                  "h-transfer: fine element " << f << " has parent " << parent[f] << " of " << ne_c);
      ECM2_VERIFY(octant[f] >= 0 && octant[f] < 8, ERR_ARG, "h-transfer: fine element " << f << " has octant " << octant[f]);
      int &slot = pl.children[(size_t)parent[f] * 8 + octant[f]];
      ECM2_VERIFY(slot < 0, ERR_UNSUPPORTED,
                  "h-transfer: parent " << parent[f] << " has two children at octant " << octant[f] << " (" << slot << ", " << f << ")");
      slot = f;
   }
   for (long k = 0; k < (long)ne_c * 8; k++)
   {
      ECM2_VERIFY(pl.children[k] >= 0, ERR_UNSUPPORTED,
                  "h-transfer: parent " << k / 8 << " has no child at octant " << k % 8
                                        << " (non-conforming and partial refinements are not supported)");
   }
   transposed_map((long)ne_c * nd, gather_c, nc, pl.c_off, pl.c_idx);
   return pl;
}

} // namespace ecm2
