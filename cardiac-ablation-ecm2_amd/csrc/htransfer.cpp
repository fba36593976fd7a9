// htransfer.cpp -- host construction of the h-refinement transfer operator's plan (htransfer.hpp): the two 1D
// tables (GetLocalRefinementMatrices, fem/fespace.cpp:1786-1807, in tensor form, with NodalLocalInterpolation's
// 1e-12 threshold, fem/fe/fe_base.cpp:884-893), the owner bits (RefinementOperator::MultTranspose's `processed`
// marks, fem/fespace.cpp:2030-2085), the children table (CoarseFineTransformations::embeddings inverted) and the
// coarse space's transposed map.  Plain C++: also compiled into tests/cpp/htransfer_plan_check.cpp's CPU program.
#include "htransfer.hpp"

#include "fe.hpp"

#include <cmath>

namespace ecm2
{

HTransferBasis htransfer_basis(int p)
{
   ECM2_VERIFY(p >= 1 && p <= kTransferMaxOrder, ERR_UNSUPPORTED,
               "h-transfer: order " << p << " (kernels exist for 1 <= p <= " << kTransferMaxOrder << ")");
   HTransferBasis b = {};
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

HTransferPlan build_htransfer_plan(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                                   const int *parent, const int *octant)
{
   HTransferPlan pl;
   pl.basis = htransfer_basis(p);  // (refuses the order)
   ECM2_VERIFY(ne_c >= 0 && ne_f >= 0 && nc >= 0 && nf >= 0, ERR_ARG, "h-transfer: negative size");
   ECM2_VERIFY(ne_c == 0 || gather_c, ERR_ARG, "h-transfer: null coarse gather map");
   ECM2_VERIFY(ne_f == 0 || (gather_f && parent && octant), ERR_ARG, "h-transfer: null fine gather map or embedding");
   const int D = p + 1, nd = D * D * D;
   ECM2_VERIFY((long)ne_f * nd <= 0x7fffffffL, ERR_UNSUPPORTED,
               "h-transfer: an E-vector of " << ne_f << " elements exceeds 2^31 entries");
   pl.p = p; pl.ne_c = ne_c; pl.ne_f = ne_f; pl.nc = nc; pl.nf = nf;
   for (long k = 0; k < (long)ne_c * nd; k++)
   {
      ECM2_VERIFY(gather_c[k] >= 0, ERR_UNSUPPORTED, "h-transfer: signed entry " << gather_c[k] << " in the coarse map (H1 has none)");
      ECM2_VERIFY(gather_c[k] < nc, ERR_ARG, "h-transfer: coarse map entry " << gather_c[k] << " >= ndofs " << nc);
   }
   // the owner of a fine dof is the lowest fine element that holds it (the first to mark it `processed`)
   std::vector<char> seen((size_t)nf, 0);
   pl.owner.assign((size_t)ne_f * 2, 0);
   long owned = 0;
   for (int e = 0; e < ne_f; e++)
   {
      for (int i = 0; i < nd; i++)
      {
         const int g = gather_f[(long)e * nd + i];
         ECM2_VERIFY(g >= 0, ERR_UNSUPPORTED, "h-transfer: signed entry " << g << " in the fine map (H1 has none)");
         ECM2_VERIFY(g < nf, ERR_ARG, "h-transfer: fine map entry " << g << " >= ndofs " << nf);
         if (!seen[g])
         {
            seen[g] = 1;
            owned++;
            pl.owner[(size_t)e * 2 + (i >> 6)] |= uint64_t(1) << (i & 63);
         }
      }
   }
   ECM2_VERIFY(owned == nf, ERR_ARG, "h-transfer: " << nf - owned << " fine dofs are held by no element");
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
   // the coarse transposed map (counting sort: ascending E-vector entries within a row)
   pl.c_off.assign((size_t)nc + 1, 0);
   for (long k = 0; k < (long)ne_c * nd; k++) { pl.c_off[gather_c[k] + 1]++; }
   for (int c = 0; c < nc; c++) { pl.c_off[c + 1] += pl.c_off[c]; }
   pl.c_idx.resize((size_t)ne_c * nd);
   std::vector<int> fill(pl.c_off.begin(), pl.c_off.end() - 1);
   for (long k = 0; k < (long)ne_c * nd; k++) { pl.c_idx[fill[gather_c[k]]++] = (int)k; }
   return pl;
}

} // namespace ecm2
