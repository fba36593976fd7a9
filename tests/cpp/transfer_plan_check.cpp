// transfer_plan_check.cpp -- CPU check of the transfer operator's host construction (csrc/transfer.cpp), both kinds,
// built under ASan + UBSan by the library Makefile's transfer_plan_check target and run by
// tests/test_transfer_host.py and tests/test_htransfer_host.py.  Reads cases from stdin:
//    pcase <ne> <pc> <nc> <pf> <nf>, the coarse map (ne (pc+1)^3 ints), the fine map, x_c (nc hex doubles), x_f (nf)
//    hcase <p> <ne_c> <nc> <ne_f> <nf>, the coarse map (ne_c (p+1)^3 ints), the fine map, parent (ne_f ints), octant,
//          x_c, x_f
// and for each: checks the owner bits (every fine dof has exactly one owner, the lowest fine element holding it),
// the children table (h: the embedding inverted; p: empty), the h tables and the coarse transposed map (every
// (element, local) pair exactly once, in its dof's row, ascending), then replays Mult and MultTranspose from the plan
// in the device's order -- the reference's (fem/transfer.cpp:2338-2423, :2470-2539): x, y, z sums ascending; then
// children in ascending octant order; the coarse E-vector summed through the transposed map -- and prints the
// results as hex doubles for the caller to compare with tests/mg_ref.py or tests/hmg_ref.py.  Then the refusals of
// both builders, the h ones on a one-parent mesh refined by HexMesh::refine_uniform.
#include "mesh.hpp"
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

int cube(int d) { return d * d * d; }
bool owns(const TransferPlan &p, int e, int i) { return (p.owner[(size_t)e * 2 + (i >> 6)] >> (i & 63)) & 1; }

// (parent, octant: the h kind's embedding; empty for the p kind)
void check_plan(const TransferPlan &p, const std::vector<int> &gc, const std::vector<int> &gf,
                const std::vector<int> &parent, const std::vector<int> &octant)
{
   const int Df = p.pf + 1, ndc = cube(p.pc + 1), ndf = cube(Df);
   std::vector<int> owners(p.nf, 0), lowest(p.nf, -1);
   for (int e = 0; e < p.ne_f; e++)
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
   CHECK((int)p.c_off.size() == p.nc + 1 && p.c_off[0] == 0 && p.c_off[p.nc] == p.ne_c * ndc, "transposed map offsets");
   std::vector<char> seen((size_t)p.ne_c * ndc, 0);
   for (int c = 0; c < p.nc; c++)
   {
      for (int k = p.c_off[c]; k < p.c_off[c + 1]; k++)
      {
         const int idx = p.c_idx[k];
         CHECK(idx >= 0 && idx < p.ne_c * ndc, "transposed map entry " << idx);
         CHECK(gc[idx] == c, "E-vector entry " << idx << " listed in row " << c << ", its dof is " << gc[idx]);
         CHECK(!seen[idx], "E-vector entry " << idx << " listed twice");
         seen[idx] = 1;
         CHECK(k == p.c_off[c] || p.c_idx[k - 1] < idx, "row " << c << " not ascending");
      }
   }
   for (size_t k = 0; k < seen.size(); k++) { CHECK(seen[k], "E-vector entry " << k << " not listed"); }
   if (p.kind == TRANSFER_P)
   {
      CHECK(p.children.empty() && p.ne_c == p.ne_f && p.pc < p.pf, "a p plan: no children table, one mesh, two orders");
      return;
   }
   CHECK(p.pc == p.pf, "an h plan: one order");
   CHECK((int)p.children.size() == 8 * p.ne_c && p.ne_f == 8 * p.ne_c, "children table size");
   std::vector<char> listed(p.ne_f, 0);
   for (int i = 0; i < p.ne_c; i++)
   {
      for (int o = 0; o < 8; o++)
      {
         const int f = p.children[(size_t)i * 8 + o];
         CHECK(f >= 0 && f < p.ne_f, "child " << f << " of parent " << i);
         if (f < 0 || f >= p.ne_f) { continue; }
         CHECK(parent[f] == i && octant[f] == o, "child " << f << " listed at (" << i << ", " << o << "), embedded at ("
                                                          << parent[f] << ", " << octant[f] << ")");
         CHECK(!listed[f], "child " << f << " listed twice");
         listed[f] = 1;
      }
   }
   // the tables: rows sum to 1, entries below the threshold are exact zeros
   for (int o = 0; o < 2; o++)
   {
      for (int q = 0; q < Df; q++)
      {
         double sum = 0.0;
         for (int d = 0; d < Df; d++)
         {
            const double v = p.basis.B[o][q + Df * d];
            CHECK(v == 0.0 || std::fabs(v) >= kHTransferZero, "table entry " << v << " below the threshold");
            sum += v;
         }
         CHECK(std::fabs(sum - 1.0) <= 1e-14, "row " << q << " of table " << o << " sums to " << sum);
      }
   }
}

// Parameterised like the kernels: a unit (element; parent) with nch children (itself; its eight fine elements)
void replay(const TransferPlan &p, const std::vector<int> &gc, const std::vector<int> &gf, const std::vector<double> &xc,
            const std::vector<double> &xf, std::vector<double> &yf, std::vector<double> &yc)
{
   const int Dc = p.pc + 1, Df = p.pf + 1, ndc = cube(Dc), ndf = cube(Df), nch = p.kind == TRANSFER_H ? 8 : 1;
   yf.assign(p.nf, std::nan(""));
   std::vector<double> ye((size_t)p.ne_c * ndc);
   for (int u = 0; u < p.ne_c; u++)
   {
      std::vector<double> part((size_t)nch * ndc);
      for (int o = 0; o < nch; o++)
      {
         const int f = nch == 1 ? u : p.children[(size_t)u * 8 + o];
         const double *Bx = p.basis.B[o & 1], *By = p.basis.B[(o >> 1) & 1], *Bz = p.basis.B[o >> 2];
         for (int qz = 0; qz < Df; qz++)
         for (int qy = 0; qy < Df; qy++)
         for (int qx = 0; qx < Df; qx++)
         {
            const int l = qx + Df * (qy + Df * qz);
            if (!owns(p, f, l)) { continue; }
            double v = 0.0;
            for (int dz = 0; dz < Dc; dz++)
            {
               double sxy = 0.0;
               for (int dy = 0; dy < Dc; dy++)
               {
                  double sx = 0.0;
                  for (int dx = 0; dx < Dc; dx++) { sx += Bx[qx + Df * dx] * xc[gc[(size_t)u * ndc + dx + Dc * (dy + Dc * dz)]]; }
                  sxy += By[qy + Df * dy] * sx;
               }
               v += Bz[qz + Df * dz] * sxy;
            }
            yf[gf[(size_t)f * ndf + l]] = v;
         }
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
                     const int l = qx + Df * (qy + Df * qz);
                     sx += Bx[qx + Df * dx] * (owns(p, f, l) ? xf[gf[(size_t)f * ndf + l]] : 0.0);
                  }
                  sxy += By[qy + Df * dy] * sx;
               }
               v += Bz[qz + Df * dz] * sxy;
            }
            part[(size_t)o * ndc + dx + Dc * (dy + Dc * dz)] = v;
         }
      }
      for (int a = 0; a < ndc; a++)
      {
         double v = part[a];
         for (int o = 1; o < nch; o++) { v += part[(size_t)o * ndc + a]; }
         ye[(size_t)u * ndc + a] = v;
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

void check_p_refusals()
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

struct Maps
{
   int p, ne_c, nc, ne_f, nf;
   std::vector<int> gc, gf, parent, octant;
   int code() const
   {
      try
      {
         (void)build_htransfer_plan(p, ne_c, nc, gc.empty() ? nullptr : gc.data(), ne_f, nf, gf.empty() ? nullptr : gf.data(),
                                    parent.empty() ? nullptr : parent.data(), octant.empty() ? nullptr : octant.data());
      }
      catch (const Error &e) { return e.code; }
      return OK;
   }
};

// one hex and its eight children at order p, through the mesh's own refinement and numbering
Maps one_parent(int p)
{
   HexMesh m = HexMesh::cartesian(1, 1, 1, 1.0, 1.0, 1.0);
   const H1Space lo = H1Space::build(m, p, NUMBERING_ENTITY);
   m.refine_uniform();
   const H1Space hi = H1Space::build(m, p, NUMBERING_ENTITY);
   Maps r{p, lo.ne, lo.ndofs, hi.ne, hi.ndofs, lo.gather_map, hi.gather_map, {}, {}};
   int native_to_lex[8];
   for (int a = 0; a < 8; a++) { native_to_lex[kLexToNative[a]] = a; }
   for (int f = 0; f < 8; f++) { r.parent.push_back(0); r.octant.push_back(native_to_lex[f]); }
   return r;
}

void check_h_refusals()
{
   const Maps ok = one_parent(2);
   CHECK(ok.code() == OK, "a valid pair");
   Maps m = ok;
   m.p = 0;
   CHECK(m.code() == ERR_UNSUPPORTED, "p = 0");
   m.p = 5;
   CHECK(m.code() == ERR_UNSUPPORTED, "p = 5");
   m = ok; m.gc.clear();
   CHECK(m.code() == ERR_ARG, "a null coarse map");
   m = ok; m.gf.clear();
   CHECK(m.code() == ERR_ARG, "a null fine map");
   m = ok; m.parent.clear();
   CHECK(m.code() == ERR_ARG, "a null embedding");
   m = ok; m.ne_f = -1;
   CHECK(m.code() == ERR_ARG, "ne < 0");
   m = ok; m.gf[13] = m.nf;
   CHECK(m.code() == ERR_ARG, "a fine entry out of range");
   m = ok; m.gc[3] = m.nc;
   CHECK(m.code() == ERR_ARG, "a coarse entry out of range");
   m = ok; m.gf[13] = -1 - m.gf[13];
   CHECK(m.code() == ERR_UNSUPPORTED, "a signed fine entry");
   m = ok; m.gc[3] = -1 - m.gc[3];
   CHECK(m.code() == ERR_UNSUPPORTED, "a signed coarse entry");
   m = ok; m.nf += 1;
   CHECK(m.code() == ERR_ARG, "a fine dof held by no element");
   m = ok; m.parent[5] = 1;
   CHECK(m.code() == ERR_ARG, "a parent out of range");
   m = ok; m.parent[5] = -1;
   CHECK(m.code() == ERR_ARG, "a negative parent");
   m = ok; m.octant[5] = 8;
   CHECK(m.code() == ERR_ARG, "an octant out of range");
   m = ok; m.octant[5] = m.octant[4];
   CHECK(m.code() == ERR_UNSUPPORTED, "two children at one octant (and none at another)");
   // seven children: a parent with a missing octant
   m = ok; m.ne_f = 7; m.parent.pop_back(); m.octant.pop_back();
   m.gf.resize((size_t)7 * 27);
   {
      std::vector<char> held(m.nf, 0);
      for (int g : m.gf) { held[g] = 1; }
      bool all = true;
      for (char h : held) { all = all && h; }
      // (the eighth child's interior dofs are held by no one else: the map is refused before the embedding is)
      CHECK(!all && m.code() == ERR_ARG, "seven children whose maps leave fine dofs unheld");
   }
   // two parents declared, all eight children given to the first: the second has none
   m = ok; m.ne_c = 2;
   m.gc.insert(m.gc.end(), ok.gc.begin(), ok.gc.end());
   CHECK(m.code() == ERR_UNSUPPORTED, "a parent without children");
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
   while (std::cin >> word && (word == "pcase" || word == "hcase"))
   {
      const bool h = word == "hcase";
      int ne_c, ne_f, pc, pf, nc, nf;
      if (h) { std::cin >> pc >> ne_c >> nc >> ne_f >> nf; pf = pc; }
      else { std::cin >> ne_c >> pc >> nc >> pf >> nf; ne_f = ne_c; }
      std::vector<int> gc((size_t)ne_c * cube(pc + 1)), gf((size_t)ne_f * cube(pf + 1)), parent(h ? ne_f : 0), octant(h ? ne_f : 0);
      for (int &v : gc) { std::cin >> v; }
      for (int &v : gf) { std::cin >> v; }
      for (int &v : parent) { std::cin >> v; }
      for (int &v : octant) { std::cin >> v; }
      std::vector<double> xc(nc), xf(nf), yf, yc;
      for (double &v : xc) { v = read_hex(); }
      for (double &v : xf) { v = read_hex(); }
      try
      {
         const TransferPlan p = h ? build_htransfer_plan(pc, ne_c, nc, gc.data(), ne_f, nf, gf.data(), parent.data(), octant.data())
                                  : build_transfer_plan(ne_c, pc, nc, gc.data(), pf, nf, gf.data());
         CHECK(p.kind == (h ? TRANSFER_H : TRANSFER_P) && p.ne_c == ne_c && p.ne_f == ne_f && p.pc == pc && p.pf == pf &&
                  p.nc == nc && p.nf == nf, "the plan's kind and sizes");
         check_plan(p, gc, gf, parent, octant);
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
   check_p_refusals();
   check_h_refusals();
   std::printf("cases %d\n", ncases);
   if (fails) { return 1; }
   std::printf("PASS\n");
   return 0;
}
