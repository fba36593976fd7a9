// plan_check.cpp -- CPU check of the fused kernels' scatter plans (csrc/scatter_plan.hpp).
//
// For each case: build the H1 gather map with the project's mesh and space code, build the plan,
// and replay the scatter on the host in integers, the way the kernels execute it: every element
// entry carries a small integer weight; the thread-per-element replay applies the in-wave and
// cross-wave face merges the lane flags name (tpe_assemble_store, k_tpe.hip) and stores the held
// entries to y or to their partial slots; the line replay sums each brick's lattice points and
// stores them or the leftover elements' entries; then the summation plan runs thread by thread
// as k_sum_partials does.  y must equal the direct per-dof sum of the weights, every slot must be
// in bounds, written once and read once, and the lattice units must reproduce the map.
// Links scatter_plan.cpp, bricks.cpp, mesh.cpp and fe.cpp only; meant to run under ASan + UBSan
// (tests/test_plan_host.py).  usage: plan_check <tests/golden directory>
#include "kernels.hpp"
#include "mesh.hpp"
#include "scatter_plan.hpp"

#include <algorithm>
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
   int ne, D, ND, ndofs;
   std::vector<int> gmap;
};
static Space make_space(const HexMesh &m, int p, int numbering)
{
   const H1Space h = H1Space::build(m, p, numbering);
   return {h.ne, p + 1, h.nd, h.ndofs, h.gather_map};
}
static Space cartesian(int nx, int ny, int nz, int p, int numbering)
{
   return make_space(HexMesh::cartesian(nx, ny, nz, 1.0, 1.0, 1.0), p, numbering);
}
static Space fichera(const std::string &golden, int refinements, int p)
{
   HexMesh m = HexMesh::read(golden + "/fichera.mesh");
   for (int r = 0; r < refinements; r++) { m.refine_uniform(); }
   return make_space(m, p, NUMBERING_ENTITY);
}

static int dofv(int g) { return g >= 0 ? g : -1 - g; }
static int edof(int enc) { return enc & 0x3fffffff; }
static bool eshared(int enc) { return ((unsigned)enc >> 30) & 1; }
static bool eneg(int enc) { return (unsigned)enc >> 31; }
static long weight(const Space &S, int e, int a) { return 1 + ((long)e * S.ND + a) % 7; }

// what a replay writes: y and the partial slots, with write / read counts
struct Scatter
{
   std::vector<long> y, part;
   std::vector<int> ywrites, pwrites, preads;
   Scatter(int ndofs, size_t nslots) : y(ndofs, 0), part(nslots, 0), ywrites(ndofs, 0), pwrites(nslots, 0), preads(nslots, 0) {}
   void store(int d, bool shared, long slot, long v)
   {
      CHECK(d >= 0 && d < (int)y.size(), "dof %d", d);
      if (!shared)
      {
         y[d] = v;
         ywrites[d]++;
         return;
      }
      CHECK(slot >= 0 && slot < (long)part.size(), "slot %ld of %zu", slot, part.size());
      CHECK(!pwrites[slot], "slot %ld written twice", slot);
      part[slot] = v;
      pwrites[slot] = 1;
   }
   long read(long slot)
   {
      CHECK(slot >= 0 && slot < (long)part.size(), "read of slot %ld of %zu", slot, part.size());
      CHECK(pwrites[slot], "slot %ld read but never written", slot);
      preads[slot]++;
      return part[slot];
   }
};

// kern::sum_partials, thread by thread (k_sum_partials: 256 threads per plan block)
static void replay_sum(const SharedPlan &P, int n_owned, Scatter &sc)
{
   CHECK((int)P.blocks.size() == 4 * P.nblk && (long)P.runs.size() == 12 * (P.n_runs + 1), "plan sizes");
   CHECK((int)P.pdof.size() == P.n_sh && P.nblk_owned <= P.nblk && P.n_sh_owned <= P.n_sh, "plan counts");
   int next_run = 0, next_entry = 0;
   long explicit_runs = 0;
   for (int blk = 0; blk < P.nblk; blk++)
   {
      const int r0 = P.blocks[4 * blk], nr = P.blocks[4 * blk + 1] - r0, e0 = P.blocks[4 * blk + 2], bn = P.blocks[4 * blk + 3];
      const int n = bn & 0xffff;
      CHECK(r0 == next_run && nr > 0 && r0 + nr <= P.n_runs && e0 == next_entry && n >= 1 && n <= 256, "block %d", blk);
      CHECK(P.runs[(size_t)(r0 + nr) * 12 + 6] == e0 + n, "block %d: the row after its runs starts at entry %d", blk, e0 + n);
      const int *sd = &P.runs[(size_t)r0 * 12];
      for (int t = 0; t < n; t++)
      {
         const int i = e0 + t;
         int lo = 0, hi = nr - 1;
         while (lo < hi)
         {
            const int mid = (lo + hi + 1) >> 1;
            if (sd[mid * 12 + 6] <= i) { lo = mid; }
            else { hi = mid - 1; }
         }
         const int *R = sd + lo * 12;
         const int shape = R[0], n1 = shape & 255, n2 = (shape >> 8) & 255, cnt = (shape >> 16) & 255;
         const int off = i - R[6], pa = off % n1, pb = off / n1;
         CHECK(off >= 0 && pb < n2, "entry %d outside its run", i);
         const bool ex = shape >> 24;
         CHECK(!ex || ((bn >> 30) & 1), "block %d: explicit run without the block's flag", blk);
         const int d = ex ? P.pdof[i] : R[1] + pa * R[2] + pb * R[3];
         CHECK(d == P.pdof[i], "entry %d: dof %d, entry list %d", i, d, P.pdof[i]);
         CHECK((blk < P.nblk_owned) == (d < n_owned) && (i < P.n_sh_owned) == (d < n_owned), "entry %d: dof %d on the wrong side of the owned | ghost boundary", i, d);
         const int ds = pa * R[4] + pb * R[5];
         long acc = 0;
         for (int k = 0; k < cnt; k++)
         {
            CHECK(R[7] + k < (int)P.rslots.size(), "run slot list");
            const int s = P.rslots[R[7] + k];  // (the slot list holds every holder, the row the first four)
            CHECK(k >= 4 || s == R[8 + k], "run row slot %d", k);
            acc += sc.read((long)s + ds);
         }
         sc.store(d, false, 0, acc);
      }
      for (int r = r0; r < r0 + nr; r++) { explicit_runs += P.runs[(size_t)r * 12] >> 24; }
      next_run = r0 + nr;
      next_entry = e0 + n;
   }
   CHECK(next_run == P.n_runs && next_entry == P.n_sh && explicit_runs == P.n_explicit_runs, "plan blocks do not cover the plan");
   CHECK(P.runs[(size_t)P.n_runs * 12 + 6] == P.n_sh, "sentinel");
}

static void check_result(const Space &S, const Scatter &sc, long n_slots)
{
   std::vector<long> want(S.ndofs, 0);
   for (int e = 0; e < S.ne; e++)
      for (int a = 0; a < S.ND; a++)
      {
         const int g = S.gmap[(size_t)e * S.ND + a];
         want[dofv(g)] += g < 0 ? -weight(S, e, a) : weight(S, e, a);
      }
   for (int d = 0; d < S.ndofs; d++)
   {
      CHECK(sc.ywrites[d] == 1, "dof %d stored %d times", d, sc.ywrites[d]);
      CHECK(sc.y[d] == want[d], "y[%d] = %ld, direct sum %ld", d, sc.y[d], want[d]);
   }
   long written = 0;
   for (size_t s = 0; s < sc.part.size(); s++)
   {
      CHECK(sc.preads[s] == sc.pwrites[s], "slot %zu written %d, read %d times", s, sc.pwrites[s], sc.preads[s]);
      written += sc.pwrites[s];
   }
   CHECK(written == n_slots, "%ld slots written, plan says %ld", written, n_slots);
}

static bool same(const SharedPlan &a, const SharedPlan &b)
{
   return a.runs == b.runs && a.rslots == b.rslots && a.blocks == b.blocks && a.pdof == b.pdof && a.n_sh == b.n_sh &&
          a.n_sh_owned == b.n_sh_owned && a.nblk_owned == b.nblk_owned && a.nblk == b.nblk && a.n_slots == b.n_slots &&
          a.n_runs == b.n_runs && a.n_explicit_runs == b.n_explicit_runs;
}
static bool same(const TpePlan &a, const TpePlan &b)
{
   return a.perm == b.perm && a.perm_derived == b.perm_derived && a.pos == b.pos && a.gmap_blk == b.gmap_blk &&
          a.lane_flags == b.lane_flags && a.treg == b.treg && a.lmap == b.lmap && a.n_treg == b.n_treg && a.n_tlat == b.n_tlat &&
          a.part_stride == b.part_stride && a.treg_all == b.treg_all && a.tlat_all == b.tlat_all && same(a.shared, b.shared);
}
static bool same(const LinePlan &a, const LinePlan &b)
{
   return a.gmap_line == b.gmap_line && a.lelem == b.lelem && a.lelem_off == b.lelem_off && a.belem == b.belem &&
          a.bmap == b.bmap && a.brick_off == b.brick_off && a.breg == b.breg && a.n_bricks == b.n_bricks &&
          a.brick_bz == b.brick_bz && a.brick_np == b.brick_np && a.n_left == b.n_left &&
          a.part_line_off == b.part_line_off && same(a.shared, b.shared);
}

// ---- thread-per-element replay ----
static TpePlan check_tpe(const char *name, const Space &S, int n_owned, const std::vector<int> &splits, int latency_from,
                         const PlanOptions &opt = {})
{
   g_case = name;
   const int D = S.D, ND = S.ND, ne = S.ne, nblk = (ne + 63) / 64;
   const TpePlan P = build_tpe_plan(ne, D, S.ndofs, n_owned, S.gmap, {}, splits, latency_from, true, opt);
   CHECK(same(P, build_tpe_plan(ne, D, S.ndofs, n_owned, S.gmap, {}, splits, latency_from, true, opt)), "second build differs");
   CHECK(P.perm_derived && (int)P.perm.size() == ne && (int)P.pos.size() == ne, "order");
   CHECK(P.gmap_blk.size() == (size_t)nblk * ND * 64 && P.lane_flags.size() == (size_t)nblk * 64, "map sizes");
   CHECK(P.treg.empty() || P.treg.size() == (size_t)nblk * 8, "block table size");
   const int NL = tpe_lattice_points(D), L = 4 * (D - 1);
   CHECK(P.lmap.empty() ? P.n_tlat == 0 : P.lmap.size() == (size_t)nblk * NL, "lattice map size");
   Scatter sc(S.ndofs, (size_t)nblk * P.part_stride);  // (PAForm: part_.resize(nblk * part_stride))
   auto ent = [&](int b, int l, int a) { return P.gmap_blk[((size_t)b * ND + a) * 64 + l]; };
   // the lanes' outputs, with the map's orientation signs
   std::vector<long> Y((size_t)nblk * 64 * ND, 0);
   auto Yo = [&](std::vector<long> &v, int b, int l, int a) -> long & { return v[((size_t)b * 64 + l) * ND + a]; };
   for (int i = 0; i < ne; i++)
   {
      const int e = P.perm[i], b = i / 64, l = i % 64;
      CHECK(e >= 0 && e < ne && P.pos[e] == i, "perm / pos at %d", i);
      for (int a = 0; a < ND; a++)
      {
         const int g = S.gmap[(size_t)e * ND + a];
         CHECK(edof(ent(b, l, a)) == dofv(g) && eneg(ent(b, l, a)) == (g < 0), "blocked map entry (%d, %d, %d)", b, l, a);
         Yo(Y, b, l, a) = g < 0 ? -weight(S, e, a) : weight(S, e, a);
      }
   }
   // workgroups: 4 blocks from each apply segment's first block
   std::vector<int> seg{0, nblk};
   for (int sp : splits) { seg.push_back(std::max(0, std::min(nblk, sp))); }
   std::sort(seg.begin(), seg.end());
   auto group_of = [&](int b, int &g0, int &g1) {
      int s0 = 0, s1 = nblk;
      for (int c : seg) { if (c <= b) { s0 = std::max(s0, c); } else { s1 = std::min(s1, c); } }
      g0 = s0 + (b - s0) / 4 * 4;
      g1 = std::min(g0 + 4, s1);
   };
   auto face = [D](int dir, int s, int i, int j) {
      return dir == 0 ? (j * D + i) * D + s : dir == 1 ? (j * D + s) * D + i : (s * D + j) * D + i;
   };
   for (int dir = 0; dir < 3; dir++)
   {
      const int delta = 1 << (2 * dir), recv = 1 << (2 * dir), sent = 2 << (2 * dir);
      std::vector<long> Y0 = Y;  // what the shuffles and the LDS staging read
      for (int b = 0; b < nblk; b++)
         for (int l = 0; l < 64; l++)
         {
            const int fl = P.lane_flags[(size_t)b * 64 + l];
            CHECK(!(fl & recv) || l + delta < 64, "lane %d receives from beyond the wave", l);
            int g0 = 0, g1 = 0, bs = -1;
            if (fl & (64 << dir))
            {
               group_of(b, g0, g1);
               bs = g0 + ((fl >> (9 + 3 * dir)) & 7);
               const int m = l - 3 * delta;
               CHECK(bs < g1 && bs != b && m >= 0 && ((m / delta) & 3) == 0, "cross-wave link of block %d lane %d", b, l);
               CHECK(P.lane_flags[(size_t)bs * 64 + m] & sent, "cross-wave sender %d lane %d did not send", bs, m);
               CHECK(latency_from < 0 || b < latency_from, "cross-wave link in a latency block");
            }
            for (int j = 0; j < D; j++)
               for (int i = 0; i < D; i++)
               {
                  const int lo = face(dir, 0, i, j), hi = face(dir, D - 1, i, j);
                  if (fl & recv) { Yo(Y, b, l, hi) += Yo(Y0, b, l + delta, lo); }
                  if (fl & sent) { Yo(Y, b, l, lo) = 0; }
                  if (bs >= 0) { Yo(Y, b, l, hi) += Yo(Y0, bs, l - 3 * delta, lo); }
               }
         }
   }
   // the store
   for (int i = 0; i < ne; i++)
   {
      const int b = i / 64, l = i % 64, fl = P.lane_flags[(size_t)b * 64 + l];
      const int *rg = P.treg.empty() ? nullptr : &P.treg[(size_t)b * 8];
      const int regf = rg ? rg[7] : 0;
      CHECK(regf >= 0 && regf <= 2, "block flag %d", regf);
      for (int a = 0; a < ND; a++)
      {
         const LatticeXYZ p = block_lattice_xyz(D, l, a);
         const bool held = !((a % D == 0 && (fl & 2)) || ((a / D) % D == 0 && (fl & 8)) || (a / (D * D) == 0 && (fl & 32)));
         int d = edof(ent(b, l, a));
         bool shared = eshared(ent(b, l, a));
         if (regf == 1)  // the five integers reproduce the map
         {
            const int faces = (p.X == 0) | (p.X == L) << 1 | (p.Y == 0) << 2 | (p.Y == L) << 3 | (p.Z == 0) << 4 | (p.Z == L) << 5;
            CHECK(d == rg[0] + p.X * rg[1] + p.Y * rg[2] + p.Z * rg[3] && !eneg(ent(b, l, a)), "regular block %d: dof of (%d, %d)", b, l, a);
            CHECK(!held || shared == ((faces & rg[4]) != 0), "regular block %d: shared flag of (%d, %d)", b, l, a);
         }
         if (regf == 2)  // the lattice map reproduces the entries
         {
            const int g = P.lmap[(size_t)b * NL + tpe_lattice_slot(D, p.X, p.Y, p.Z)];
            CHECK(g == ent(b, l, a), "lattice-slot block %d: entry (%d, %d)", b, l, a);
         }
         if (!held) { continue; }
         const int si = tpe_surface_index(D, p.X, p.Y, p.Z);
         CHECK(!shared || !regf || si >= 0, "block %d: shared interior point", b);
         sc.store(d, shared, (long)b * P.part_stride + (regf ? si : a * 64 + l), Yo(Y, b, l, a));
      }
   }
   replay_sum(P.shared, n_owned, sc);
   check_result(S, sc, P.shared.n_slots);
   std::printf("ok  %-40s ne %d blocks %d regular %d lattice-slot %d stride %d shared %d (owned %d) slots %ld runs %ld\n", name, ne,
               nblk, P.n_treg, P.n_tlat, P.part_stride, P.shared.n_sh, P.shared.n_sh_owned, P.shared.n_slots, P.shared.n_runs);
   return P;
}

// ---- line / brick replay ----
static LinePlan check_line(const char *name, const Space &S, int bz, const std::vector<int> &splits = {})
{
   g_case = name;
   const int D = S.D, ND = S.ND, ne = S.ne, nblk = (ne + 63) / 64;
   const LinePlan P = build_line_plan(ne, D, S.ndofs, S.ndofs, S.gmap, splits, bz, {});
   CHECK(same(P, build_line_plan(ne, D, S.ndofs, S.ndofs, S.gmap, splits, bz, {})), "second build differs");
   const int nbe = 4 * (P.brick_bz ? P.brick_bz : 1), np = P.brick_np;
   const int LX = 2 * D - 1, LY = LX, LZ = P.brick_bz * (D - 1) + 1;
   const int nsurf = P.brick_bz ? brick_surface_points(D, P.brick_bz) : 0;
   CHECK(P.belem.size() == (size_t)P.n_bricks * nbe && P.bmap.size() == (size_t)P.n_bricks * np, "brick sizes");
   CHECK(!P.n_bricks || np == LX * LY * LZ, "brick lattice points");
   CHECK(P.part_line_off == (long)P.n_bricks * nsurf && (int)P.lelem.size() == P.n_left, "slot offsets");
   CHECK(P.gmap_line.size() == S.gmap.size() && P.breg.size() == (P.breg.empty() ? 0 : (size_t)P.n_bricks * 8), "map sizes");
   CHECK((int)P.lelem_off.size() == nblk + 1 && (int)P.brick_off.size() == nblk + 1 && P.lelem_off[nblk] == P.n_left &&
            P.brick_off[nblk] == P.n_bricks, "per-block lists");
   // (PAForm: part_.resize(max(1, part_line_off + (n_left ? ne * ND : 0))))
   Scatter sc(S.ndofs, std::max<size_t>(1, (size_t)P.part_line_off + (P.n_left ? (size_t)ne * ND : 0)));
   std::vector<int> seen(ne, 0);
   for (int k = 0; k < P.n_bricks; k++)
   {
      std::vector<long> acc(np, 0);
      for (int elt = 0; elt < nbe; elt++)
      {
         const int e = P.belem[(size_t)k * nbe + elt], ex = elt & 1, ey = (elt >> 1) & 1, ez = elt >> 2;
         CHECK(e >= 0 && e < ne && !seen[e]++, "brick %d member %d", k, elt);
         for (int a = 0; a < ND; a++)
         {
            const int p = ((ez * (D - 1) + a / (D * D)) * LY + ey * (D - 1) + (a / D) % D) * LX + ex * (D - 1) + a % D;
            const int g = S.gmap[(size_t)e * ND + a];
            CHECK(g >= 0 && edof(P.bmap[(size_t)k * np + p]) == g, "brick %d: lattice point %d", k, p);
            acc[p] += weight(S, e, a);
         }
      }
      const int *rg = P.breg.empty() ? nullptr : &P.breg[(size_t)k * 8];
      for (int p = 0; p < np; p++)
      {
         const int X = p % LX, Y = (p / LX) % LY, Z = p / (LX * LY), enc = P.bmap[(size_t)k * np + p];
         if (rg)  // the five integers reproduce the lattice map
         {
            const int faces = (X == 0) | (X == LX - 1) << 1 | (Y == 0) << 2 | (Y == LY - 1) << 3 | (Z == 0) << 4 | (Z == LZ - 1) << 5;
            CHECK(edof(enc) == rg[0] + X * rg[1] + Y * rg[2] + Z * rg[3], "regular brick %d: dof of point %d", k, p);
            CHECK(eshared(enc) == ((faces & rg[4]) != 0), "regular brick %d: shared flag of point %d", k, p);
         }
         const int si = brick_surface_index(D, P.brick_bz, X, Y, Z);
         CHECK(!eshared(enc) || si >= 0, "brick %d: shared interior point %d", k, p);
         sc.store(edof(enc), eshared(enc), (long)k * nsurf + si, acc[p]);
      }
   }
   for (int b = 0; b < nblk; b++)
   {
      for (int k = P.brick_off[b]; k < P.brick_off[b + 1]; k++) { CHECK(P.belem[(size_t)k * nbe] / 64 == b, "brick %d not in block %d", k, b); }
      for (int i = P.lelem_off[b]; i < P.lelem_off[b + 1]; i++)
      {
         const int e = P.lelem[i];
         CHECK(e >= 0 && e < ne && e / 64 == b && !seen[e]++, "leftover element %d of block %d", e, b);
         for (int a = 0; a < ND; a++)
         {
            const int g = S.gmap[(size_t)e * ND + a], enc = P.gmap_line[(size_t)e * ND + a];
            sc.store(edof(enc), eshared(enc), P.part_line_off + (long)e * ND + a, g < 0 ? -weight(S, e, a) : weight(S, e, a));
         }
      }
   }
   for (size_t i = 0; i < S.gmap.size(); i++)
   {
      CHECK(seen[i / ND] == 1, "element %zu in %d units", i / ND, seen[i / ND]);
      CHECK(edof(P.gmap_line[i]) == dofv(S.gmap[i]) && eneg(P.gmap_line[i]) == (S.gmap[i] < 0), "encoded map entry %zu", i);
   }
   replay_sum(P.shared, S.ndofs, sc);
   check_result(S, sc, P.shared.n_slots);
   std::printf("ok  %-40s ne %d bricks %d (2x2x%d, regular %d) left %d shared %d slots %ld runs %ld\n", name, ne, P.n_bricks,
               P.brick_bz, (int)!P.breg.empty(), P.n_left, P.shared.n_sh, P.shared.n_slots, P.shared.n_runs);
   return P;
}

int main(int argc, char **argv)
{
   CHECK(argc == 2, "usage: plan_check <golden directory>");
   const std::string golden = argv[1];
   try
   {
      const Space c844 = cartesian(8, 4, 4, 2, NUMBERING_STRUCTURED);
      {
         const TpePlan P = check_tpe("p2 structured 8x4x4", c844, c844.ndofs, {}, -1);
         CHECK(P.treg_all && P.n_treg == 2 && P.part_stride == tpe_surface_points(3), "two regular blocks, surface stride");
      }
      {
         const TpePlan P = check_tpe("p2 structured 8x4x4 split 1 latency 1", c844, c844.ndofs, {1}, 1);
         CHECK(!P.treg_all && (P.treg.empty() || P.treg[8 + 7] == 0) && P.part_stride == 27 * 64, "block 1 is a lattice unit");
         for (int l = 0; l < 64; l++) { CHECK(!(P.lane_flags[64 + l] >> 6), "block 1 lane %d is cross-wave linked", l); }
      }
      {
         const Space c543 = cartesian(5, 4, 3, 1, NUMBERING_ENTITY);
         const TpePlan P = check_tpe("p1 entity 5x4x3", c543, c543.ndofs, {}, -1);
         CHECK(P.n_treg + P.n_tlat == 0 && P.part_stride == 8 * 64, "a partial block stores [a][lane] slots");
      }
      const Space f2 = fichera(golden, 2, 2);
      {
         const TpePlan P = check_tpe("p2 entity fichera x2", f2, f2.ndofs, {}, -1);
         CHECK(f2.ne == 448 && P.n_tlat + P.n_treg > 0 && !P.lmap.empty(), "fichera: %d elements, %d + %d lattice units", f2.ne, P.n_treg, P.n_tlat);
      }
      {
         // (one workgroup: the two blocks' common face is assembled across the waves, nothing is
         // shared; blocks with ghost dofs are not regular)
         const TpePlan P = check_tpe("p2 structured 8x4x4 owned ndofs-40", c844, c844.ndofs - 40, {}, -1);
         CHECK(P.n_treg == 0, "blocks with ghost dofs are regular");
         // a workgroup per block, each block half of the mesh's z-layers (no 4x4x4 brick): dofs
         // stay shared, ghosts among them, and the plan has both ranges
         const TpePlan Q = check_tpe("p2 structured 8x4x4 owned ndofs-40 split 1", c844, c844.ndofs - 40, {1}, -1);
         CHECK(Q.shared.n_sh_owned > 0 && Q.shared.n_sh > Q.shared.n_sh_owned && Q.shared.nblk_owned > 0 && Q.shared.nblk > Q.shared.nblk_owned,
               "owned and ghost ranges: %d shared, %d owned", Q.shared.n_sh, Q.shared.n_sh_owned);
      }
      // every run order, without shared dofs (one workgroup) and with them (latency block)
      const char *orders[3] = {"slot", "dof", "chain"};
      for (int o = 0; o < 3; o++)
      {
         PlanOptions opt;
         opt.run_order = o;
         const std::string by = std::string(" run order ") + orders[o];
         check_tpe(("p2 structured 8x4x4" + by).c_str(), c844, c844.ndofs, {}, -1, opt);
         check_tpe(("p2 8x4x4 split 1 latency 1" + by).c_str(), c844, c844.ndofs, {1}, 1, opt);
         check_tpe(("p2 entity fichera x2" + by).c_str(), f2, f2.ndofs, {}, -1, opt);
      }
      const Space c442 = cartesian(4, 4, 2, 3, NUMBERING_STRUCTURED);
      {
         const LinePlan P = check_line("p3 bz1 4x4x2", c442, 1);
         CHECK(P.n_bricks == c442.ne / 4 && !P.breg.empty() && P.n_left == 0, "every element in a regular 2x2x1 brick");
      }
      {
         const LinePlan P = check_line("p3 bz1 5x3x2", cartesian(5, 3, 2, 3, NUMBERING_STRUCTURED), 1);
         CHECK(P.n_bricks > 0 && P.n_left > 0, "bricks and leftover elements");
      }
      {
         const LinePlan P = check_line("p3 bz2 4x4x2", c442, 2);
         CHECK(P.n_bricks == c442.ne / 8 && P.brick_bz == 2 && P.n_left == 0, "every element in a 2x2x2 brick");
      }
      {
         const LinePlan P = check_line("p4 bz1 entity fichera x1", fichera(golden, 1, 4), 1);
         CHECK(P.n_bricks > 0 && P.breg.empty(), "entity-numbered bricks are not regular");
      }
      check_line("p3 no bricks 5x3x2", cartesian(5, 3, 2, 3, NUMBERING_STRUCTURED), 0);
   }
   catch (const Error &e)
   {
      std::printf("FAIL [%s] ecm2 error %d: %s\n", g_case.c_str(), e.code, e.what());
      return 1;
   }
   std::printf("PASS\n");
   return 0;
}
