// conv_plan_check.cpp -- CPU check of the convection term's plan (csrc/conv_plan.hpp).
//
// For each case (mesh, order, marker, layout): build the H1 gather map with the project's mesh and space
// code, build the plan, and check it the way the kernels use it:
//   * every E-vector entry of an active element appears in exactly one CSR row, and that row is the
//     entry's dof; no entry of an inactive element (and no padding slot) appears;
//   * each row's entries ascend in (element, local index) order, its dofs ascend and are unique;
//   * orientation signs survive (some map entries are flipped to -1 - g on purpose);
//   * the map in the kernel's layout reproduces the gather rows, padding lanes repeat in-bounds entries;
//   * all indices are in bounds;
//   * summing ones over the rows reproduces each dof's signed count of active holders.
// Links conv_plan.cpp, mesh.cpp and fe.cpp only; meant to run under ASan + UBSan
// (tests/test_conv_plan_host.py).  usage: conv_plan_check <tests/golden directory>
#include "common.hpp"
#include "conv_plan.hpp"
#include "mesh.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace ecm2;

static std::string g_case;
#define CHECK(cond, ...)                                                  \
   do {                                                                   \
      if (!(cond)) {                                                      \
         std::printf("FAIL [%s] %s:%d: %s: ", g_case.c_str(), __FILE__, __LINE__, #cond); \
         std::printf(__VA_ARGS__);                                        \
         std::printf("\n");                                               \
         std::exit(1);                                                    \
      }                                                                   \
   } while (0)

struct Space
{
   int ne, nd, ndofs;
   std::vector<int> gmap;
   std::vector<double> zc;  // element centroid z (the slab marker)
};

static Space make_space(const HexMesh &m, int p, int numbering)
{
   const H1Space h = H1Space::build(m, p, numbering);
   Space s{h.ne, h.nd, h.ndofs, h.gather_map, {}};
   std::vector<double> en;
   m.element_nodes(en);  // [ne][3][8]
   s.zc.resize(h.ne);
   for (int e = 0; e < h.ne; e++)
   {
      double z = 0.0;
      for (int a = 0; a < 8; a++) { z += en[((size_t)e * 3 + 2) * 8 + a]; }
      s.zc[e] = z / 8.0;
   }
   return s;
}

static void check(const Space &S, const std::vector<unsigned char> &keep, bool blocked, bool flip)
{
   std::vector<int> gmap = S.gmap;
   if (flip)
   {
      for (size_t i = 0; i < gmap.size(); i += 5) { gmap[i] = -1 - gmap[i]; }
   }
   const int nd = S.nd;
   const ConvPlan p = build_conv_plan(gmap, S.ne, nd, S.ndofs, keep, blocked);
   int n_keep = 0;
   for (unsigned char k : keep) { n_keep += k != 0; }
   CHECK(p.n_act == n_keep && (int)p.act.size() == n_keep, "active count %d of %d", p.n_act, n_keep);
   for (int k = 0; k < p.n_act; k++)
   {
      CHECK(p.act[k] >= 0 && p.act[k] < S.ne && keep[p.act[k]], "active element %d", p.act[k]);
      CHECK(k == 0 || p.act[k] > p.act[k - 1], "active list not ascending at %d", k);
   }
   const int nblk = (p.n_act + kConvBlock - 1) / kConvBlock;
   const size_t ev = blocked ? (size_t)nblk * nd * kConvBlock : (size_t)p.n_act * nd;
   CHECK(p.ev_size == ev && p.map.size() == ev, "E-vector size %zu, expected %zu", p.ev_size, ev);
   CHECK((int)p.csr_dof.size() == p.n_rows && (int)p.csr_off.size() == p.n_rows + 1, "row arrays");
   CHECK(p.csr_off[0] == 0 && p.csr_off[p.n_rows] == (int)p.csr_idx.size(), "row offsets");
   CHECK(p.csr_idx.size() == (size_t)p.n_act * nd, "%zu entries", p.csr_idx.size());
   // the map in the kernel's layout; where a real entry lives
   std::vector<int> owner(ev, -1);  // E-vector position -> k nd + i of the active entry, -1 padding
   for (int k = 0; k < p.n_act; k++)
      for (int i = 0; i < nd; i++)
      {
         const size_t pos = conv_ev_index(blocked, nd, k, i);
         CHECK(pos < ev && owner[pos] < 0, "position %zu", pos);
         owner[pos] = k * nd + i;
         CHECK(p.map[pos] == gmap[(size_t)p.act[k] * nd + i], "map row of active element %d", k);
      }
   for (size_t pos = 0; pos < ev; pos++)
   {
      const int g = p.map[pos], d = g >= 0 ? g : -1 - g;
      CHECK(d >= 0 && d < S.ndofs, "map entry %d at %zu", g, pos);  // (padding lanes too: in-bounds loads)
   }
   // the rows
   std::vector<int> seen(ev, 0);
   std::vector<long> y(S.ndofs, 0), want(S.ndofs, 0);
   for (int r = 0; r < p.n_rows; r++)
   {
      const int d = p.csr_dof[r];
      CHECK(d >= 0 && d < S.ndofs, "row dof %d", d);
      CHECK(r == 0 || d > p.csr_dof[r - 1], "row dofs not ascending at %d", r);
      CHECK(p.csr_off[r + 1] > p.csr_off[r], "empty row %d", r);
      int last = -1;
      for (int j = p.csr_off[r]; j < p.csr_off[r + 1]; j++)
      {
         const int enc = p.csr_idx[j];
         const long pos = enc >= 0 ? enc : -1 - (long)enc;
         CHECK(pos >= 0 && (size_t)pos < ev, "entry %d of row %d", enc, r);
         CHECK(owner[pos] >= 0, "row %d lists the padding slot %ld", r, pos);
         CHECK(!seen[pos], "position %ld listed twice", pos);
         seen[pos] = 1;
         CHECK(owner[pos] > last, "row %d: entries not in ascending element order", r);
         last = owner[pos];
         const int g = gmap[(size_t)p.act[owner[pos] / nd] * nd + owner[pos] % nd];
         CHECK((g >= 0 ? g : -1 - g) == d, "row %d lists an entry of dof %d", r, g);
         CHECK((g < 0) == (enc < 0), "sign of entry %ld", pos);
         y[d] += enc >= 0 ? 1 : -1;  // the add pass over an E-vector of ones
      }
   }
   for (size_t pos = 0; pos < ev; pos++) { CHECK(seen[pos] == (owner[pos] >= 0), "position %zu listed %d times", pos, seen[pos]); }
   for (int e = 0; e < S.ne; e++)
   {
      if (!keep[e]) { continue; }
      for (int i = 0; i < nd; i++)
      {
         const int g = gmap[(size_t)e * nd + i];
         want[g >= 0 ? g : -1 - g] += g >= 0 ? 1 : -1;
      }
   }
   for (int d = 0; d < S.ndofs; d++) { CHECK(y[d] == want[d], "dof %d: %ld of %ld holders", d, y[d], want[d]); }
}

static void run(const std::string &name, const Space &S)
{
   double zmin = 1e300, zmax = -1e300;
   for (double z : S.zc) { zmin = z < zmin ? z : zmin; zmax = z > zmax ? z : zmax; }
   std::vector<unsigned char> none(S.ne, 0), all(S.ne, 1), slab(S.ne, 0), stripes(S.ne, 0);
   for (int e = 0; e < S.ne; e++)
   {
      slab[e] = S.zc[e] > zmin + 0.3 * (zmax - zmin) && S.zc[e] < zmin + 0.8 * (zmax - zmin);
      stripes[e] = e % 3 != 0;
   }
   const struct { const char *n; const std::vector<unsigned char> *k; } markers[] = {
      {"none", &none}, {"all", &all}, {"z-slab", &slab}, {"stripes", &stripes}};
   for (const auto &mk : markers)
      for (int blocked = 0; blocked < 2; blocked++)
         for (int flip = 0; flip < 2; flip++)
         {
            g_case = name + " " + mk.n + (blocked ? " blocked" : " rows") + (flip ? " signs" : "");
            check(S, *mk.k, blocked != 0, flip != 0);
         }
   std::printf("ok %s: %d elements, %d dofs\n", name.c_str(), S.ne, S.ndofs);
}

int main(int argc, char **argv)
{
   if (argc < 2)
   {
      std::printf("usage: conv_plan_check <tests/golden directory>\n");
      return 2;
   }
   const std::string golden = argv[1];
   for (int p = 1; p <= 4; p++)
   {
      // (the plan depends on the topology only: the perturbed 5 x 4 x 3 mesh of the tests is this one)
      run("cartesian 5x4x3 p=" + std::to_string(p), make_space(HexMesh::cartesian(5, 4, 3, 1.0, 0.8, 0.6), p, NUMBERING_ENTITY));
      HexMesh m = HexMesh::read(golden + "/fichera.mesh");
      m.refine_uniform();
      run("fichera refined p=" + std::to_string(p), make_space(m, p, NUMBERING_ENTITY));
   }
   run("cartesian 2x1x1 p=2", make_space(HexMesh::cartesian(2, 1, 1, 2.0, 1.0, 1.0), 2, NUMBERING_ENTITY));
   run("cartesian 8x8x8 p=2 structured", make_space(HexMesh::cartesian(8, 8, 8, 1.0, 0.7, 1.3), 2, NUMBERING_STRUCTURED));
   // a map entry out of range is refused, not planned
   {
      Space S = make_space(HexMesh::cartesian(2, 1, 1, 2.0, 1.0, 1.0), 1, NUMBERING_ENTITY);
      S.gmap[3] = S.ndofs;
      bool threw = false;
      try { (void)build_conv_plan(S.gmap, S.ne, S.nd, S.ndofs, std::vector<unsigned char>(S.ne, 1), true); }
      catch (const Error &) { threw = true; }
      g_case = "out-of-range entry";
      CHECK(threw, "not refused");
   }
   std::printf("PASS\n");
   return 0;
}
