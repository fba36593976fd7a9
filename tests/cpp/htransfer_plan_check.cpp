// htransfer_plan_check.cpp -- CPU check of the h-refinement transfer operator's host construction
// (csrc/htransfer.cpp), built under ASan + UBSan by the library Makefile's htransfer_plan_check target and run by
// tests/test_htransfer_host.py.  Reads cases from stdin:
//    case <p> <ne_c> <nc> <ne_f> <nf>, the coarse map (ne_c (p+1)^3 ints), the fine map, parent (ne_f ints), octant,
//    x_c (nc hex doubles), x_f (nf)
// and for each: checks the owner bits (every fine dof has exactly one owner, the lowest fine element holding it),
// the children table (the embedding inverted) and the coarse transposed map, then replays Mult and MultTranspose
// from the plan in the device's order (x, y, z sums ascending; children in ascending octant order; the coarse
// E-vector summed through the transposed map) and prints the results as hex doubles for the caller to compare with
// tests/hmg_ref.py.  Then the refusals, on a one-parent mesh refined by HexMesh::refine_uniform.
#include "htransfer.hpp"
#include "mesh.hpp"

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

bool owns(const HTransferPlan &p, int e, int i) { return (p.owner[(size_t)e * 2 + (i >> 6)] >> (i & 63)) & 1; }

void check_plan(const HTransferPlan &p, const std::vector<int> &gc, const std::vector<int> &gf,
                const std::vector<int> &parent, const std::vector<int> &octant)
{
   const int D = p.p + 1, nd = D * D * D;
   std::vector<int> owners(p.nf, 0), lowest(p.nf, -1);
   for (int e = 0; e < p.ne_f; e++)
   {
      for (int i = 0; i < nd; i++)
      {
         const int g = gf[(size_t)e * nd + i];
         if (lowest[g] < 0) { lowest[g] = e; }
         if (owns(p, e, i))
         {
            owners[g]++;
            CHECK(lowest[g] == e, "fine dof " << g << " owned by element " << e << ", lowest holder " << lowest[g]);
         }
      }
      for (int i = nd; i < 128; i++) { CHECK(!owns(p, e, i), "owner bit " << i << " beyond the element's dofs"); }
   }
   for (int g = 0; g < p.nf; g++) { CHECK(owners[g] == 1, "fine dof " << g << " has " << owners[g] << " owners"); }
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
   CHECK((int)p.c_off.size() == p.nc + 1 && p.c_off[0] == 0 && p.c_off[p.nc] == p.ne_c * nd, "transposed map offsets");
   std::vector<char> seen((size_t)p.ne_c * nd, 0);
   for (int c = 0; c < p.nc; c++)
   {
      for (int k = p.c_off[c]; k < p.c_off[c + 1]; k++)
      {
         const int idx = p.c_idx[k];
         CHECK(idx >= 0 && idx < p.ne_c * nd, "transposed map entry " << idx);
         CHECK(gc[idx] == c, "E-vector entry " << idx << " listed in row " << c << ", its dof is " << gc[idx]);
         CHECK(!seen[idx], "E-vector entry " << idx << " listed twice");
         seen[idx] = 1;
         CHECK(k == p.c_off[c] || p.c_idx[k - 1] < idx, "row " << c << " not ascending");
      }
   }
   for (size_t k = 0; k < seen.size(); k++) { CHECK(seen[k], "E-vector entry " << k << " not listed"); }
   // the tables: rows sum to 1, entries below the threshold are exact zeros
   for (int o = 0; o < 2; o++)
   {
      for (int q = 0; q < D; q++)
      {
         double sum = 0.0;
         for (int d = 0; d < D; d++)
         {
            const double v = p.basis.B[o][q + D * d];
            CHECK(v == 0.0 || std::fabs(v) >= kHTransferZero, "table entry " << v << " below the threshold");
            sum += v;
         }
         CHECK(std::fabs(sum - 1.0) <= 1e-14, "row " << q << " of table " << o << " sums to " << sum);
      }
   }
}

void replay(const HTransferPlan &p, const std::vector<int> &gc, const std::vector<int> &gf, const std::vector<double> &xc,
            const std::vector<double> &xf, std::vector<double> &yf, std::vector<double> &yc)
{
   const int D = p.p + 1, nd = D * D * D;
   yf.assign(p.nf, std::nan(""));
   std::vector<double> ye((size_t)p.ne_c * nd);
   for (int i = 0; i < p.ne_c; i++)
   {
      std::vector<double> part((size_t)8 * nd);
      for (int o = 0; o < 8; o++)
      {
         const int f = p.children[(size_t)i * 8 + o];
         const double *Bx = p.basis.B[o & 1], *By = p.basis.B[(o >> 1) & 1], *Bz = p.basis.B[o >> 2];
         for (int qz = 0; qz < D; qz++)
         for (int qy = 0; qy < D; qy++)
         for (int qx = 0; qx < D; qx++)
         {
            const int l = qx + D * (qy + D * qz);
            if (!owns(p, f, l)) { continue; }
            double v = 0.0;
            for (int dz = 0; dz < D; dz++)
            {
               double sxy = 0.0;
               for (int dy = 0; dy < D; dy++)
               {
                  double sx = 0.0;
                  for (int dx = 0; dx < D; dx++) { sx += Bx[qx + D * dx] * xc[gc[(size_t)i * nd + dx + D * (dy + D * dz)]]; }
                  sxy += By[qy + D * dy] * sx;
               }
               v += Bz[qz + D * dz] * sxy;
            }
            yf[gf[(size_t)f * nd + l]] = v;
         }
         for (int dz = 0; dz < D; dz++)
         for (int dy = 0; dy < D; dy++)
         for (int dx = 0; dx < D; dx++)
         {
            double v = 0.0;
            for (int qz = 0; qz < D; qz++)
            {
               double sxy = 0.0;
               for (int qy = 0; qy < D; qy++)
               {
                  double sx = 0.0;
                  for (int qx = 0; qx < D; qx++)
                  {
                     const int l = qx + D * (qy + D * qz);
                     sx += Bx[qx + D * dx] * (owns(p, f, l) ? xf[gf[(size_t)f * nd + l]] : 0.0);
                  }
                  sxy += By[qy + D * dy] * sx;
               }
               v += Bz[qz + D * dz] * sxy;
            }
            part[(size_t)o * nd + dx + D * (dy + D * dz)] = v;
         }
      }
      for (int a = 0; a < nd; a++)
      {
         double v = part[a];
         for (int o = 1; o < 8; o++) { v += part[(size_t)o * nd + a]; }
         ye[(size_t)i * nd + a] = v;
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

void check_refusals()
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
   while (std::cin >> word && word == "case")
   {
      int p, ne_c, nc, ne_f, nf;
      std::cin >> p >> ne_c >> nc >> ne_f >> nf;
      const size_t nd = (size_t)(p + 1) * (p + 1) * (p + 1);
      std::vector<int> gc(ne_c * nd), gf(ne_f * nd), parent(ne_f), octant(ne_f);
      for (int &v : gc) { std::cin >> v; }
      for (int &v : gf) { std::cin >> v; }
      for (int &v : parent) { std::cin >> v; }
      for (int &v : octant) { std::cin >> v; }
      std::vector<double> xc(nc), xf(nf), yf, yc;
      for (double &v : xc) { v = read_hex(); }
      for (double &v : xf) { v = read_hex(); }
      try
      {
         const HTransferPlan pl = build_htransfer_plan(p, ne_c, nc, gc.data(), ne_f, nf, gf.data(), parent.data(), octant.data());
         check_plan(pl, gc, gf, parent, octant);
         replay(pl, gc, gf, xc, xf, yf, yc);
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
