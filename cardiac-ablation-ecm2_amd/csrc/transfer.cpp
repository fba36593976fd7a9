// transfer.cpp -- host construction of the p-refinement transfer operator's plan (transfer.hpp): the 1D table
// (TensorProductPRefinementTransferOperator's constructor, fem/transfer.cpp:2223-2287), the owner bits
// (ElementRestriction::BooleanMask, fem/restriction.cpp:248-283) and the coarse space's transposed map.
// Plain C++: also compiled into tests/cpp/transfer_plan_check.cpp's CPU program.
#include "transfer.hpp"

#include "fe.hpp"

namespace ecm2
{

TransferPlan build_transfer_plan(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f)
{
   ECM2_VERIFY(pc < pf, ERR_ARG, "transfer: the coarse order " << pc << " must be below the fine order " << pf);
   ECM2_VERIFY(pc >= 1 && pf <= kTransferMaxOrder, ERR_UNSUPPORTED,
               "transfer: orders " << pc << " -> " << pf << " (kernels exist for 1 <= pc < pf <= " << kTransferMaxOrder << ")");
   ECM2_VERIFY(ne >= 0 && nc >= 0 && nf >= 0, ERR_ARG, "transfer: negative size");
   ECM2_VERIFY(ne == 0 || (gather_c && gather_f), ERR_ARG, "transfer: null gather map");
   const int Dc = pc + 1, Df = pf + 1, ndc = Dc * Dc * Dc, ndf = Df * Df * Df;
   // (the transposed map indexes the coarse E-vector with ints, the kernels' staging loops the fine one)
   ECM2_VERIFY((long)ne * ndc <= 0x7fffffffL && (long)ne * ndf <= 0x7fffffffL, ERR_UNSUPPORTED,
               "transfer: an E-vector of " << ne << " elements exceeds 2^31 entries");
   TransferPlan p;
   p.ne = ne; p.pc = pc; p.pf = pf; p.nc = nc; p.nf = nf;
   // B[q + Df d]: coarse basis function d at fine node q
   double xc[MAX_D1D], xf[MAX_D1D], w[MAX_D1D], u[MAX_D1D], du[MAX_D1D];
   gauss_lobatto(Dc, xc, w);
   gauss_lobatto(Df, xf, w);
   for (int q = 0; q < Df; q++)
   {
      basis_eval(pc, xc, xf[q], u, du);
      for (int d = 0; d < Dc; d++) { p.basis.B[q + Df * d] = u[d]; }
   }
   // the maps' entries; the owner of a fine dof is the lowest element that holds it (its first occurrence in
   // the E-vector, BooleanMask's "first element" rule)
   for (long k = 0; k < (long)ne * ndc; k++)
   {
      ECM2_VERIFY(gather_c[k] >= 0, ERR_UNSUPPORTED, "transfer: signed entry " << gather_c[k] << " in the coarse map (H1 has none)");
      ECM2_VERIFY(gather_c[k] < nc, ERR_ARG, "transfer: coarse map entry " << gather_c[k] << " >= ndofs " << nc);
   }
   std::vector<char> seen((size_t)nf, 0);
   p.owner.assign((size_t)ne * 2, 0);
   long owned = 0;
   for (int e = 0; e < ne; e++)
   {
      for (int i = 0; i < ndf; i++)
      {
         const int g = gather_f[(long)e * ndf + i];
         ECM2_VERIFY(g >= 0, ERR_UNSUPPORTED, "transfer: signed entry " << g << " in the fine map (H1 has none)");
         ECM2_VERIFY(g < nf, ERR_ARG, "transfer: fine map entry " << g << " >= ndofs " << nf);
         if (!seen[g])
         {
            seen[g] = 1;
            owned++;
            p.owner[(size_t)e * 2 + (i >> 6)] |= uint64_t(1) << (i & 63);
         }
      }
   }
   ECM2_VERIFY(owned == nf, ERR_ARG, "transfer: " << nf - owned << " fine dofs are held by no element");
   // the coarse transposed map (counting sort: ascending E-vector entries within a row)
   p.c_off.assign((size_t)nc + 1, 0);
   for (long k = 0; k < (long)ne * ndc; k++) { p.c_off[gather_c[k] + 1]++; }
   for (int c = 0; c < nc; c++) { p.c_off[c + 1] += p.c_off[c]; }
   p.c_idx.resize((size_t)ne * ndc);
   std::vector<int> fill(p.c_off.begin(), p.c_off.end() - 1);
   for (long k = 0; k < (long)ne * ndc; k++) { p.c_idx[fill[gather_c[k]]++] = (int)k; }
   return p;
}

} // namespace ecm2
