// transfer_plan_check.cpp -- CPU check of the transfer operator's host construction (csrc/transfer.cpp), built
// under ASan + UBSan by the library Makefile's transfer_plan_check target and run by tests/test_transfer_host.py.
// Reads cases from stdin:
//    case <ne> <pc> <nc> <pf> <nf>, the coarse map (ne (pc+1)^3 ints), the fine map, x_c (nc hex doubles), x_f (nf)
// and for each: checks the owner bits (every fine dof has exactly one owner, the lowest element holding it) and
// the coarse transposed map (every (element, local) pair exactly once, in its dof's row, ascending), then replays
// Mult and MultTranspose from the plan in the reference's order (fem/transfer.cpp:2338-2423, :2470-2539) and
// prints the results as hex doubles for the caller to compare with tests/mg_ref.py.  Then the refusals.
#include "transfer.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

using namespace ecm2;

namespace
{
int fails = 0;
#define CHECK(c, msg)                                                       \
   do {                                                                     \
      if (!(c)) { std::cerr << "FAIL: " << msg << " [" << #c << "]\n"; fails++; } \
   } while (0)

bool owns(const TransferPlan &p, int e, int i) { return (p.owner[(size_t)e * 2 + (i >> 6)] >> (i & 63)) & 1; }

void check_plan(const TransferPlan &p, const std::vector<int> &gc, const std::vector<int> &gf)
{
   const int Dc = p.pc + 1, Df = p.pf + 1, ndc = Dc * Dc * Dc, ndf = Df * Df * Df;
   std::vector<int> owners(p.nf, 0), lowest(p.nf, -1);
   for (int e = 0; e < p.ne; e++)
   {
      for (int i = 0; i < ndf; i++)
      {
         const int g = gf[(size_t)e * ndf + i];
         if (lowest[g] < 0) { lowest[g] = e; }
         if (owns(p, e, i))
         {
            owners[g]++;
            CHECK(lowest[g] == e, "fine dof " << g << " owned by element " << e << ", lowest holder " << lowest[g]);
         }
      }
      for (int i = ndf; i < 128; i++) { CHECK(!owns(p, e, i), "owner bit " << i << " beyond the element's dofs"); }
   }
   for (int g = 0; g < p.nf; g++) { CHECK(owners[g] == 1, "fine dof " << g << " has " << owners[g] << " owners"); }
   CHECK((int)p.c_off.size() == p.nc + 1 && p.c_off[0] == 0 && p.c_off[p.nc] == p.ne * ndc, "transposed map offsets");
   std::vector<char> seen((size_t)p.ne * ndc, 0);
   for (int c = 0; c < p.nc; c++)
   {
      for (int k = p.c_off[c]; k < p.c_off[c + 1]; k++)
      {
         const int idx = p.c_idx[k];
         CHECK(idx >= 0 && idx < p.ne * ndc, "transposed map entry " << idx);
         CHECK(gc[idx] == c, "E-vector entry " << idx << " listed in row " << c << ", its dof is " << gc[idx]);
         CHECK(!seen[idx], "E-vector entry " << idx << " listed twice");
         seen[idx] = 1;
         CHECK(k == p.c_off[c] || p.c_idx[k - 1] < idx, "row " << c << " not ascending");
      }
   }
   for (size_t k = 0; k < seen.size(); k++) { CHECK(seen[k], "E-vector entry " << k << " not listed"); }
}

void replay(const TransferPlan &p, const std::vector<int> &gc, const std::vector<int> &gf, const std::vector<double> &xc,
            const std::vector<double> &xf, std::vector<double> &yf, std::vector<double> &yc)
{
   const int Dc = p.pc + 1, Df = p.pf + 1, ndc = Dc * Dc * Dc, ndf = Df * Df * Df;
   const double *B = p.basis.B;
   yf.assign(p.nf, std::nan(""));
   for (int e = 0; e < p.ne; e++)
   {
      for (int qz = 0; qz < Df; qz++)
      for (int qy = 0; qy < Df; qy++)
      for (int qx = 0; qx < Df; qx++)
      {
         const int i = qx + Df * (qy + Df * qz);
         if (!owns(p, e, i)) { continue; }
         double v = 0.0;
         for (int dz = 0; dz < Dc; dz++)
         {
            double sxy = 0.0;
            for (int dy = 0; dy < Dc; dy++)
            {
               double sx = 0.0;
               for (int dx = 0; dx < Dc; dx++) { sx += B[qx + Df * dx] * xc[gc[(size_t)e * ndc + dx + Dc * (dy + Dc * dz)]]; }
               sxy += B[qy + Df * dy] * sx;
            }
            v += B[qz + Df * dz] * sxy;
         }
         yf[gf[(size_t)e * ndf + i]] = v;
      }
   }
   std::vector<double> ye((size_t)p.ne * ndc);
   for (int e = 0; e < p.ne; e++)
   {
      for (int dz = 0; dz < Dc; dz++)
      for (int dy = 0; dy < Dc; dy++)
      for (int dx = 0; dx < Dc; dx++)
      {
         double v = 0.0;
         for (int qz = 0; qz < Df; qz++)
         {
            double sxy = 0.0;
            for (int qy = 0; qy < Df; qy++)
            {
               double sx = 0.0;
               for (int qx = 0; qx < Df; qx++)
               {
                  const int i = qx + Df * (qy + Df * qz);
                  sx += B[qx + Df * dx] * (owns(p, e, i) ? xf[gf[(size_t)e * ndf + i]] : 0.0);
               }
               sxy += B[qy + Df * dy] * sx;
            }
            v += B[qz + Df * dz] * sxy;
         }
         ye[(size_t)e * ndc + dx + Dc * (dy + Dc * dz)] = v;
      }
   }
   yc.assign(p.nc, 0.0);
   for (int c = 0; c < p.nc; c++)
   {
      double v = 0.0;
      for (int k = p.c_off[c]; k < p.c_off[c + 1]; k++) { v += ye[p.c_idx[k]]; }
      yc[c] = v;
   }
}

int code_of(int ne, int pc, int nc, const int *gc, int pf, int nf, const int *gf)
{
   try { (void)build_transfer_plan(ne, pc, nc, gc, pf, nf, gf); }
   catch (const Error &e) { return e.code; }
   return OK;
}

void check_refusals()
{
   // one element, p 1 -> 2
   std::vector<int> gc(8), gf(27);
   for (int i = 0; i < 8; i++) { gc[i] = i; }
   for (int i = 0; i < 27; i++) { gf[i] = i; }
   CHECK(code_of(1, 1, 8, gc.data(), 2, 27, gf.data()) == OK, "a valid pair");
   CHECK(code_of(1, 2, 27, gf.data(), 2, 27, gf.data()) == ERR_ARG, "pc == pf");
   CHECK(code_of(1, 2, 27, gf.data(), 1, 8, gc.data()) == ERR_ARG, "pc > pf");
   CHECK(code_of(1, 0, 1, gc.data(), 2, 27, gf.data()) == ERR_UNSUPPORTED, "pc = 0");
   std::vector<int> g5(216, 0);
   CHECK(code_of(1, 1, 8, gc.data(), 5, 216, g5.data()) == ERR_UNSUPPORTED, "pf = 5");
   std::vector<int> bad = gf;
   bad[13] = -1 - 13;
   CHECK(code_of(1, 1, 8, gc.data(), 2, 27, bad.data()) == ERR_UNSUPPORTED, "a signed fine entry");
   bad = gf;
   bad[13] = 27;
   CHECK(code_of(1, 1, 8, gc.data(), 2, 27, bad.data()) == ERR_ARG, "a fine entry out of range");
   bad = gf;
   bad[13] = 12;
   CHECK(code_of(1, 1, 8, gc.data(), 2, 27, bad.data()) == ERR_ARG, "a fine dof held by no element");
   std::vector<int> badc = gc;
   badc[3] = 8;
   CHECK(code_of(1, 1, 8, badc.data(), 2, 27, gf.data()) == ERR_ARG, "a coarse entry out of range");
   badc[3] = -4;
   CHECK(code_of(1, 1, 8, badc.data(), 2, 27, gf.data()) == ERR_UNSUPPORTED, "a signed coarse entry");
   CHECK(code_of(1, 1, 8, nullptr, 2, 27, gf.data()) == ERR_ARG, "a null map");
}

double read_hex()
{
   std::string t;
   std::cin >> t;
   return std::strtod(t.c_str(), nullptr);
}
} // namespace

int main()
{
   std::string word;
   int ncases = 0;
   while (std::cin >> word && word == "case")
   {
      int ne, pc, nc, pf, nf;
      std::cin >> ne >> pc >> nc >> pf >> nf;
      const size_t ndc = (size_t)(pc + 1) * (pc + 1) * (pc + 1), ndf = (size_t)(pf + 1) * (pf + 1) * (pf + 1);
      std::vector<int> gc(ne * ndc), gf(ne * ndf);
      for (int &v : gc) { std::cin >> v; }
      for (int &v : gf) { std::cin >> v; }
      std::vector<double> xc(nc), xf(nf), yf, yc;
      for (double &v : xc) { v = read_hex(); }
      for (double &v : xf) { v = read_hex(); }
      try
      {
         const TransferPlan p = build_transfer_plan(ne, pc, nc, gc.data(), pf, nf, gf.data());
         check_plan(p, gc, gf);
         replay(p, gc, gf, xc, xf, yf, yc);
      }
      catch (const Error &e)
      {
         std::cerr << "FAIL: case " << ncases << ": " << e.what() << "\n";
         return 1;
      }
      std::printf("mult");
      for (double v : yf) { std::printf(" %a", v); }
      std::printf("\nmultT");
      for (double v : yc) { std::printf(" %a", v); }
      std::printf("\n");
      ncases++;
   }
   check_refusals();
   std::printf("cases %d\n", ncases);
   if (fails) { return 1; }
   std::printf("PASS\n");
   return 0;
}
