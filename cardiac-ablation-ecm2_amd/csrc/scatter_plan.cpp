// scatter_plan.cpp -- see scatter_plan.hpp.
#include "scatter_plan.hpp"
#include "bricks.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <array>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <tuple>

namespace ecm2
{

PlanOptions plan_options_from_env()
{
   PlanOptions o;
   const char *ro = std::getenv("ECM2_RUN_ORDER");
   const std::string r = ro ? ro : "";
   o.run_order = r == "slot" ? 0 : r == "dof" ? 1 : r == "chain" ? 2 : -1;
   o.dump = std::getenv("ECM2_PLAN_DUMP") != nullptr;
   return o;
}

namespace
{
int dofv(int g) { return g >= 0 ? g : -1 - g; }

void check_dof_bits(int ndofs) { ECM2_VERIFY(ndofs < (1 << 30), ERR_UNSUPPORTED, "fused kernel supports < 2^30 dofs"); }

// map entry: dof | shared << 30 | sign << 31
int encode_entry(int d, bool shared, bool neg)
{
   return (int)((unsigned)d | ((shared ? 1u : 0u) << 30) | ((neg ? 1u : 0u) << 31));
}

// faces of an LX x LY x LZ lattice a point lies on: bits X lo | X hi | Y lo | Y hi | Z lo | Z hi
int lattice_faces(int LX, int LY, int LZ, int X, int Y, int Z)
{
   return (X == 0) | (X == LX - 1) << 1 | (Y == 0) << 2 | (Y == LY - 1) << 3 | (Z == 0) << 4 | (Z == LZ - 1) << 5;
}

// the plan wants each dof's holders in ascending slot order (slots are distinct: the order is unique)
void sort_holders_by_slot(std::vector<int> &hdof, std::vector<int> &hslot)
{
   std::vector<size_t> ord(hslot.size());
   for (size_t i = 0; i < ord.size(); i++) { ord[i] = i; }
   std::sort(ord.begin(), ord.end(), [&](size_t p, size_t q) { return hslot[p] < hslot[q]; });
   std::vector<int> hd(ord.size()), hs(ord.size());
   for (size_t i = 0; i < ord.size(); i++) { hd[i] = hdof[ord[i]]; hs[i] = hslot[ord[i]]; }
   hdof.swap(hd);
   hslot.swap(hs);
}

// ---- the summation plan ----

// d1 == kExplicitDofs: the run's slots are affine but its dofs are not (a numbering that is not a
// lattice, e.g. the reference's entity numbering): the pass reads each entry's dof from the
// plan's entry list instead (4 coalesced bytes per entry)
constexpr int kExplicitDofs = INT32_MIN;
struct Run1 { int i0, n, c, d1, t1; };
struct Run { int n1, n2, c, dof0, d1, d2, t1, t2, first; std::vector<int> s0; };

// the shared holders by dof: dof d's slots, ascending, are slots[start[d] .. start[d + 1])
struct Holders
{
   const std::vector<int> &hcount;
   std::vector<int> start, slots;
   int cnt(int d) const { return hcount[d] > 1 ? start[d + 1] - start[d] : 0; }
   int slot(int d, int h) const { return slots[start[d] + h]; }
};

// the runs of one range ([owned | ghost]) of the entry order `dofs`
struct RangeRuns
{
   const Holders &H;
   const std::vector<int> &dofs;
   std::vector<Run1> r1s;
   std::vector<Run> out;                   // 2D runs
   std::vector<std::vector<int>> members;  // 1D runs of each 2D run
   template <typename F> void each_dof(size_t g, F f) const
   {
      for (int k : members[g])
         for (int j = 0; j < r1s[k].n; j++) { f(dofs[r1s[k].i0 + j]); }
   }
   // the 128-B lines entry d touches: its y line and its partial-slot lines
   void push_lines(int d, std::vector<long> &ids) const
   {
      ids.push_back((long)d >> 4);
      for (int h = 0; h < H.cnt(d); h++) { ids.push_back((1l << 40) + (H.slot(d, h) >> 4)); }
   }
};

// Step 1, entry order: every dof not held exactly once (dofs held by nobody get an empty list:
// y = 0), the owned dofs first, then the ghosts (split form); within each range by first slot, so
// neighbouring threads of k_sum_partials read neighbouring slots.
std::vector<int> entry_order(const Holders &H, int ndofs, int n_owned)
{
   std::vector<int> dofs;
   for (int d = 0; d < ndofs; d++) { if (H.hcount[d] != 1) { dofs.push_back(d); } }
   auto key = [&](int d) -> long {
      const long first = H.hcount[d] > 1 ? H.slots[H.start[d]] : -1;
      return (d < n_owned ? 0 : (1l << 40)) + first;
   };
   std::stable_sort(dofs.begin(), dofs.end(), [&](int p, int q) { return key(p) < key(q); });
   return dofs;
}

// Step 2, 1D runs of entries [r0, r1): consecutive entries with equal holder counts whose dof and
// every holder's slot advance by the same steps.
std::vector<Run1> runs_1d(const Holders &H, const std::vector<int> &dofs, int r0, int r1)
{
   std::vector<Run1> r1s;
   // longest run from entry i: slots affine with a common step, dofs too unless explicit
   auto extend = [&](int i, bool explicit_dofs, int &d1, int &t1) {
      const int c = H.cnt(dofs[i]);
      int n = 1;
      d1 = 0;
      t1 = 0;
      while (i + n < r1 && n < 64 && c <= 8)
      {
         const int dj = dofs[i + n], dp = dofs[i + n - 1];
         if (H.cnt(dj) != c) { break; }
         const int dd = dj - dp, tt = c ? H.slot(dj, 0) - H.slot(dp, 0) : 0;
         bool ok = n == 1 || ((explicit_dofs || dd == d1) && tt == t1);
         for (int h = 1; h < c && ok; h++) { ok = H.slot(dj, h) - H.slot(dp, h) == tt; }
         if (!ok) { break; }
         if (n == 1) { d1 = dd; t1 = tt; }
         n++;
      }
      return n;
   };
   for (int i = r0; i < r1;)
   {
      const int c = H.cnt(dofs[i]);
      int d1, t1, e1, et1;
      int n = extend(i, false, d1, t1);
      const int n_ex = c ? extend(i, true, e1, et1) : 0;  // explicit-dof run length
      if (n_ex > n && (n < 4 || n_ex >= 2 * n))  // a short affine run costs more descriptor bytes per entry
      {
         n = n_ex;
         d1 = kExplicitDofs;
         t1 = et1;
      }
      r1s.push_back({i, n, c, d1, t1});
      i += n;
   }
   return r1s;
}

// Step 3, the 2D join: 1D runs of one shape whose first entries advance by common steps again (a
// face interior, a 4 x 4 lane patch).  One open run per (count, length, steps) class; a 1D run
// joins its class's open run when its first entry continues that run's lattice, else it opens a
// new one.  A run whose slots continue the lattice but whose dofs do not (the reference's
// numbering: the 3- and 4-holder entries of a brick edge are 1D runs of one entry each) joins the
// last open run of its (count, length, slot step) class instead, which becomes explicit-dof if it
// is not yet (only while small: an explicit entry costs 4 plan bytes, a run descriptor 48).
void join_2d(RangeRuns &R)
{
   const Holders &H = R.H;
   std::map<std::tuple<int, int, int, int>, int> open_aff;
   std::map<std::tuple<int, int, int>, int> open_any;
   auto try_join = [&](int gi, const Run1 &q, int d0, int k, bool convert) {
      Run &g = R.out[gi];
      if ((g.n2 + 1) * g.n1 > 64 || q.c > 8) { return false; }
      const int tt = q.c ? H.slot(d0, 0) - g.s0[0] : 0;
      bool ok = g.n2 == 1 || tt == g.n2 * g.t2;
      for (int h = 1; h < q.c && ok; h++) { ok = H.slot(d0, h) - g.s0[h] == tt; }
      if (!ok) { return false; }
      const bool gex = g.d1 == kExplicitDofs, qex = q.d1 == kExplicitDofs;
      const int dd = d0 - g.dof0;
      const bool dofs_ok = !gex && !qex && q.d1 == g.d1 && (g.n2 == 1 || dd == g.n2 * g.d2);
      if (!gex && !dofs_ok)
      {
         if (!convert || g.n1 * g.n2 > 12) { return false; }
         g.d1 = kExplicitDofs;  // the run's dofs come from the entry list from now on
         g.d2 = 0;
      }
      if (g.n2 == 1) { g.t2 = tt; g.d2 = g.d1 == kExplicitDofs ? 0 : dd; }
      g.n2++;
      R.members[gi].push_back(k);
      return true;
   };
   for (size_t k = 0; k < R.r1s.size(); k++)
   {
      const Run1 &q = R.r1s[k];
      const int d0 = R.dofs[q.i0];
      const auto ka = std::make_tuple(q.c, q.n, q.d1, q.t1);
      const auto kb = std::make_tuple(q.c, q.n, q.t1);
      int gi = -1;
      auto ia = open_aff.find(ka);
      if (ia != open_aff.end() && try_join(ia->second, q, d0, (int)k, false)) { gi = ia->second; }
      if (gi < 0)
      {
         auto ib = open_any.find(kb);
         if (ib != open_any.end() && try_join(ib->second, q, d0, (int)k, true)) { gi = ib->second; }
      }
      if (gi < 0)
      {
         Run g{q.n, 1, q.c, d0, q.d1, 0, q.t1, 0, q.i0, {}};
         for (int h = 0; h < q.c; h++) { g.s0.push_back(H.slot(d0, h)); }
         gi = (int)R.out.size();
         open_aff[ka] = gi;
         R.out.push_back(g);
         R.members.push_back({(int)k});
      }
      open_any[kb] = gi;
   }
}

// 128-B lines (y lines written + partial-slot lines read) that windows of 256 consecutive entries
// touch when the runs go in order `go`
long lines_touched(const RangeRuns &R, const std::vector<size_t> &go)
{
   long total = 0;
   int in_window = 0;
   std::vector<long> ids;
   auto flush = [&] {
      std::sort(ids.begin(), ids.end());
      total += std::unique(ids.begin(), ids.end()) - ids.begin();
      ids.clear();
      in_window = 0;
   };
   for (size_t g : go)
   {
      R.each_dof(g, [&](int d) {
         R.push_lines(d, ids);
         if (++in_window == 256) { flush(); }
      });
   }
   flush();
   return total;
}

// chain order: greedy, each next run the unplaced one sharing the most 128-B lines with the
// run placed last (ties and dead ends: the next unplaced run in slot order), so a face's edge
// runs follow its interior run and reuse its partial lines while they are in L2
std::vector<size_t> chain_order(const RangeRuns &R)
{
   const size_t nr = R.out.size();
   std::vector<std::vector<long>> rl(nr);
   std::vector<long> all;
   for (size_t g = 0; g < nr; g++)
   {
      R.each_dof(g, [&](int d) { R.push_lines(d, rl[g]); });
      std::sort(rl[g].begin(), rl[g].end());
      rl[g].erase(std::unique(rl[g].begin(), rl[g].end()), rl[g].end());
      all.insert(all.end(), rl[g].begin(), rl[g].end());
   }
   std::sort(all.begin(), all.end());
   all.erase(std::unique(all.begin(), all.end()), all.end());
   // line -> runs (CSR)
   std::vector<int> loff(all.size() + 1, 0), lrun;
   auto lid = [&](long v) { return (size_t)(std::lower_bound(all.begin(), all.end(), v) - all.begin()); };
   std::vector<std::vector<int>> rli(nr);
   for (size_t g = 0; g < nr; g++)
      for (long v : rl[g])
      {
         const size_t i = lid(v);
         rli[g].push_back((int)i);
         loff[i + 1]++;
      }
   for (size_t i = 0; i < all.size(); i++) { loff[i + 1] += loff[i]; }
   lrun.resize(loff.back());
   {
      std::vector<int> fill(loff.begin(), loff.end() - 1);
      for (size_t g = 0; g < nr; g++)
         for (int i : rli[g]) { lrun[fill[i]++] = (int)g; }
   }
   std::vector<char> placed(nr, 0);
   std::vector<int> shared(nr, 0), touched;
   std::vector<size_t> go;
   go.reserve(nr);
   size_t next_free = 0, cur = 0;
   while (go.size() < nr)
   {
      if (go.empty() || placed[cur])
      {
         while (placed[next_free]) { next_free++; }
         cur = next_free;
      }
      placed[cur] = 1;
      go.push_back(cur);
      size_t best = nr;
      int bs = 0;
      for (int i : rli[cur])
         for (int q = loff[i]; q < loff[i + 1]; q++)
         {
            const int g = lrun[q];
            if (placed[g]) { continue; }
            if (!shared[g]) { touched.push_back(g); }
            shared[g]++;
         }
      for (int g : touched)
      {
         if (shared[g] > bs || (shared[g] == bs && (size_t)g < best)) { bs = shared[g]; best = g; }
         shared[g] = 0;
      }
      touched.clear();
      cur = best < nr ? best : cur;  // cur placed: the next free run in slot order
   }
   return go;
}

// Step 4, run order: by first partial slot (the slot locality of the entry order) or by
// smallest dof (neighbouring workgroups of the pass then store neighbouring y lines: C5
// pass -10%, profiles/r3_ab_runorder.txt) or the chain order.  Which one is decided by
// lines_touched, the smallest total wins; PlanOptions::run_order forces one.
std::vector<size_t> run_order(const RangeRuns &R, const PlanOptions &opt, int range)
{
   std::vector<size_t> by_slot(R.out.size()), by_dof, by_chain;
   for (size_t g = 0; g < by_slot.size(); g++) { by_slot[g] = g; }
   {
      std::vector<long> kmin(R.out.size(), LONG_MAX);
      for (size_t g = 0; g < R.out.size(); g++) { R.each_dof(g, [&](int d) { kmin[g] = std::min<long>(kmin[g], d); }); }
      by_dof = by_slot;
      std::stable_sort(by_dof.begin(), by_dof.end(), [&](size_t a, size_t b) { return kmin[a] < kmin[b]; });
   }
   int pick = opt.run_order;  // 0 slot, 1 dof, 2 chain
   if (pick == 2 || pick < 0) { by_chain = chain_order(R); }
   if (pick < 0)
   {
      const long ls = lines_touched(R, by_slot), ld = lines_touched(R, by_dof), lc = lines_touched(R, by_chain);
      pick = ld < ls ? 1 : 0;
      if (lc < std::min(ls, ld)) { pick = 2; }
      if (opt.dump)
      {
         std::fprintf(stderr, "plan range %d: lines touched by slot order %ld, dof order %ld, chain order %ld -> %s\n",
                      range, ls, ld, lc, pick == 2 ? "chain" : pick ? "dof" : "slot");
      }
   }
   return pick == 2 ? by_chain : pick ? by_dof : by_slot;
}

// (diagnostic) run classes of the summation plan
void dump_run_classes(const std::vector<Run> &runs, int n_sh)
{
   std::map<std::tuple<int, int, int, int>, std::pair<long, long>> h;
   for (const Run &g : runs)
   {
      auto &v = h[std::make_tuple(g.d1 == kExplicitDofs, g.c, g.n1, g.n2)];
      v.first++;
      v.second += (long)g.n1 * g.n2;
   }
   std::vector<std::pair<long, std::tuple<int, int, int, int>>> top;
   for (auto &kv : h) { top.push_back({kv.second.first, kv.first}); }
   std::sort(top.rbegin(), top.rend());
   std::fprintf(stderr, "plan: %zu runs, %d entries\n", runs.size(), n_sh);
   for (size_t i = 0; i < top.size() && i < 30; i++)
   {
      const auto &k = top[i].second;
      std::fprintf(stderr, "  explicit %d holders %d shape %dx%d: %ld runs, %ld entries\n", std::get<0>(k),
                   std::get<1>(k), std::get<2>(k), std::get<3>(k), top[i].first, h[k].second);
   }
}

// Step 5: run descriptors (every entry checked against what its descriptor computes), the slot
// list and the blocks: whole runs, <= 256 entries each, never across the owned / ghost boundary.
void emit_plan(const Holders &H, const std::vector<Run> &runs, SharedPlan &P)
{
   P.runs.reserve((runs.size() + 1) * 12);
   for (const Run &g : runs)
   {
      for (int j = 0; j < g.n1 * g.n2; j++)
      {
         const int a = j % g.n1, b = j / g.n1, d = P.pdof[g.first + j];
         bool ok = (g.d1 == kExplicitDofs || d == g.dof0 + a * g.d1 + b * g.d2) && H.cnt(d) == g.c;
         for (int h = 0; h < g.c && ok; h++) { ok = H.slot(d, h) == g.s0[h] + a * g.t1 + b * g.t2; }
         ECM2_VERIFY(ok, ERR_INTERNAL, "run plan entry " << g.first + j << " does not match its run");
      }
      const bool ex = g.d1 == kExplicitDofs;  // shape bit 24: dofs from the entry list
      ECM2_VERIFY(g.c < 256, ERR_UNSUPPORTED, "a dof with " << g.c << " holders");
      int row[12] = {g.n1 | g.n2 << 8 | g.c << 16 | (ex ? 1 << 24 : 0), g.dof0, ex ? 0 : g.d1, ex ? 0 : g.d2,
                     g.t1, g.t2, g.first, (int)P.rslots.size(), 0, 0, 0, 0};
      for (int h = 0; h < g.c; h++)
      {
         if (h < 4) { row[8 + h] = g.s0[h]; }
         P.rslots.push_back(g.s0[h]);
      }
      P.runs.insert(P.runs.end(), row, row + 12);
      P.n_explicit_runs += ex;
   }
   const int sentinel[12] = {1, 0, 0, 0, 0, 0, P.n_sh, 0, 0, 0, 0, 0};
   P.runs.insert(P.runs.end(), sentinel, sentinel + 12);
   for (size_t r = 0; r < runs.size();)
   {
      const bool ghost = runs[r].first >= P.n_sh_owned;
      size_t e = r;
      int n = 0;
      while (e < runs.size() && (runs[e].first >= P.n_sh_owned) == ghost && n + runs[e].n1 * runs[e].n2 <= 256)
      {
         n += runs[e].n1 * runs[e].n2;
         e++;
      }
      bool ex = false;
      for (size_t g = r; g < e; g++) { ex = ex || runs[g].d1 == kExplicitDofs; }
      const int row[4] = {(int)r, (int)e, runs[r].first, n | (ex ? 1 << 30 : 0)};
      P.blocks.insert(P.blocks.end(), row, row + 4);
      if (!ghost) { P.nblk_owned++; }
      r = e;
   }
   P.nblk = (int)P.blocks.size() / 4;
   P.n_runs = (long)runs.size();
}
} // namespace

SharedPlan build_shared_plan(int ndofs, int n_owned, const std::vector<int> &hcount, const std::vector<int> &hdof,
                             const std::vector<int> &hslot, const PlanOptions &opt)
{
   Holders H{hcount, std::vector<int>(ndofs + 1, 0), std::vector<int>(hdof.size())};
   for (int d = 0; d < ndofs; d++) { H.start[d + 1] = H.start[d] + (hcount[d] > 1 ? hcount[d] : 0); }
   ECM2_VERIFY((size_t)H.start[ndofs] == hdof.size(), ERR_INTERNAL, "shared holder count mismatch");
   {
      std::vector<int> fill(H.start.begin(), H.start.end() - 1);
      for (size_t i = 0; i < hdof.size(); i++) { H.slots[fill[hdof[i]]++] = hslot[i]; }
   }
   const std::vector<int> dofs = entry_order(H, ndofs, n_owned);
   ECM2_VERIFY(H.slots.size() < (1ull << 31), ERR_UNSUPPORTED, "too many partial slots");
   SharedPlan P;
   P.n_sh = (int)dofs.size();
   while (P.n_sh_owned < P.n_sh && dofs[P.n_sh_owned] < n_owned) { P.n_sh_owned++; }
   P.n_slots = (long)H.slots.size();

   // Run compression, per range ([owned | ghost]: finish_shared runs each on its own).  Entries
   // are re-emitted run by run; each dof keeps its holders in ascending slot order.
   std::vector<Run> runs;
   for (int range = 0; range < 2; range++)
   {
      const int r0 = range ? P.n_sh_owned : 0, r1 = range ? P.n_sh : P.n_sh_owned;
      RangeRuns R{H, dofs, runs_1d(H, dofs, r0, r1), {}, {}};
      join_2d(R);
      for (size_t g : run_order(R, opt, range))
      {
         R.out[g].first = (int)P.pdof.size();
         R.each_dof(g, [&](int d) { P.pdof.push_back(d); });
         runs.push_back(std::move(R.out[g]));
      }
      ECM2_VERIFY((int)P.pdof.size() == r1, ERR_INTERNAL, "run plan lost entries");
   }
   if (opt.dump) { dump_run_classes(runs, P.n_sh); }
   emit_plan(H, runs, P);
   return P;
}

// ---- thread-per-element kernel ----
namespace
{
// In-wave face assembly plan of the blocked layout (see tpe_assemble_store): per 64-lane
// block and direction x, y, z, lane l receives lane l + off's (off = 1, 4, 16) low face (index 0
// along the direction) into its high face (index D-1) when all face dofs coincide and no nonzero
// value could land in an entry that no longer holds its dof; the partner then zeroes that face.
// Then (xwave) across the waves of a workgroup group: a wave whose 16 high-face lanes all coincide
// with another wave's 16 low-face lanes receives those through LDS.  groups: [first block, end
// block, link allowed] of every workgroup (<= 4 blocks, in the launch's grouping: from each apply
// segment's first block).  Lane flags: bits 1|4|16 receive x|y|z in-wave, 2|8|32 low face sent
// (in-wave or across waves), 64|128|256 receive x|y|z across waves, bits 9-11 | 12-14 | 15-17 the
// sending wave (within the group) for x | y | z.  After the three passes the "holding" entries
// (holds[(b*64+l)*ND+a]) carry each dof's in-wave sum, and hcount[d] counts the holders of dof d
// in the whole mesh: a dof held once is plain-stored, otherwise it is "shared" (partial slot or
// atomic add).
void build_merge_plan(int ne, int D, const std::vector<int> &gmap_int, int ndofs,
                      std::vector<char> &holds, std::vector<int> &hcount, std::vector<int> &flags,
                      const std::vector<std::array<int, 3>> &groups)
{
   const int ND = D * D * D, nblk = (ne + 63) / 64;
   flags.assign((size_t)nblk * 64, 0);
   holds.assign((size_t)nblk * 64 * ND, 0);
   hcount.assign(ndofs, 0);
   auto dofv = [](int g) { return g >= 0 ? g : -1 - g; };
   auto face = [D](int dir, int s, int i, int j) {
      if (dir == 0) { return (j * D + i) * D + s; }
      if (dir == 1) { return (j * D + s) * D + i; }
      return (s * D + j) * D + i;
   };
   const int off[3] = {1, 4, 16}, recv[3] = {1, 4, 16}, sent[3] = {2, 8, 32};
   auto act = [&](int b, int l) { return b * 64 + l < ne; };
   auto dof = [&](int b, int l, int a) { return dofv(gmap_int[((size_t)b * 64 + l) * ND + a]); };
   auto H = [&](int b, int l, int a) -> char & { return holds[((size_t)b * 64 + l) * ND + a]; };
   auto F = [&](int b, int l) -> int & { return flags[(size_t)b * 64 + l]; };
   for (int b = 0; b < nblk; b++)
      for (int l = 0; l < 64; l++)
         for (int a = 0; a < ND; a++) { H(b, l, a) = act(b, l); }
   for (const auto &grp : groups)
   {
      const int g0 = grp[0], g1 = grp[1];
      const bool xw = grp[2] != 0;
      for (int dir = 0; dir < 3; dir++)
      {
         for (int b = g0; b < g1; b++)
         {
            for (int l = 0; l + off[dir] < 64; l++)
            {
               const int m = l + off[dir];
               if (!act(b, l) || !act(b, m)) { continue; }
               bool ok = true;
               for (int j = 0; j < D && ok; j++)
                  for (int i = 0; i < D && ok; i++)
                  {
                     const int ar = face(dir, D - 1, i, j), as = face(dir, 0, i, j);
                     ok = dof(b, l, ar) == dof(b, m, as) && (H(b, l, ar) || !H(b, m, as));
                  }
               if (!ok) { continue; }
               F(b, l) |= recv[dir];
               F(b, m) |= sent[dir];
            }
            for (int m = 0; m < 64; m++)
            {
               if (!(F(b, m) & sent[dir])) { continue; }
               for (int j = 0; j < D; j++)
                  for (int i = 0; i < D; i++) { H(b, m, face(dir, 0, i, j)) = 0; }
            }
         }
         if (!xw) { continue; }
         // across the group's waves: wave br's 16 high-face lanes <- wave bs's low-face lanes
         for (int br = g0; br < g1; br++)
         {
            for (int bs = g0; bs < g1; bs++)
            {
               if (bs == br) { continue; }
               bool ok = true;
               for (int l = 0; l < 64 && ok; l++)
               {
                  if ((l / off[dir]) % 4 != 3) { continue; }
                  const int m = l - 3 * off[dir];
                  ok = act(br, l) && act(bs, m) && !(F(bs, m) & sent[dir]);
                  for (int j = 0; j < D && ok; j++)
                     for (int i = 0; i < D && ok; i++)
                     {
                        const int ar = face(dir, D - 1, i, j), as = face(dir, 0, i, j);
                        ok = dof(br, l, ar) == dof(bs, m, as) && H(br, l, ar) && H(bs, m, as);
                     }
               }
               if (!ok) { continue; }
               for (int l = 0; l < 64; l++)
               {
                  if ((l / off[dir]) % 4 != 3) { continue; }
                  const int m = l - 3 * off[dir];
                  F(br, l) |= (64 << dir) | ((bs - g0) << (9 + 3 * dir));
                  F(bs, m) |= sent[dir];
                  for (int j = 0; j < D; j++)
                     for (int i = 0; i < D; i++) { H(bs, m, face(dir, 0, i, j)) = 0; }
               }
               break;  // one sender per receiving wave and direction
            }
         }
      }
   }
   for (int b = 0; b < nblk; b++)
      for (int l = 0; l < 64; l++)
         for (int a = 0; a < ND; a++) { if (H(b, l, a)) { hcount[dof(b, l, a)]++; } }
}

// no caller order: 4x4x4 face-linked bricks first (one per wave), per apply segment
std::vector<int> derive_element_order(int ne, int D, const std::vector<int> &gmap_host, const std::vector<int> &splits)
{
   const int ND = D * D * D;
   std::vector<int> perm, cuts{0};
   for (int sp : splits) { cuts.push_back(std::min(ne, sp * kElemBlock)); }
   cuts.push_back(ne);
   std::sort(cuts.begin(), cuts.end());
   for (size_t k = 0; k + 1 < cuts.size(); k++)
   {
      const int e0 = cuts[k], n = cuts[k + 1] - cuts[k];
      if (n <= 0) { continue; }
      std::vector<int> sub(gmap_host.begin() + (size_t)e0 * ND, gmap_host.begin() + (size_t)(e0 + n) * ND);
      for (int e : face_brick_order(n, D, sub)) { perm.push_back(e0 + e); }
   }
   return perm;
}

// workgroups as the launches group them (4 blocks from each apply segment's start); waves of a
// workgroup may assemble shared faces through LDS (xwave), except in segments launched with the
// one-block-per-workgroup latency kernel
std::vector<std::array<int, 3>> workgroup_groups(int nblk, const std::vector<int> &splits, int latency_from, bool xwave)
{
   std::vector<std::array<int, 3>> groups;
   std::vector<int> seg{0, nblk};
   for (int sp : splits) { seg.push_back(std::max(0, std::min(nblk, sp))); }
   std::sort(seg.begin(), seg.end());
   seg.erase(std::unique(seg.begin(), seg.end()), seg.end());
   for (size_t k = 0; k + 1 < seg.size(); k++)
   {
      const bool lat = latency_from >= 0 && seg[k] >= latency_from;
      for (int b = seg[k]; b < seg[k + 1]; b += 4) { groups.push_back({b, std::min(b + 4, seg[k + 1]), (xwave && !lat) ? 1 : 0}); }
   }
   return groups;
}

// what the block classification reads: the blocked map and the merge plan's holders
struct BlockView
{
   int D, ND, n_owned;
   const std::vector<int> &blk;
   const std::vector<char> &holds;
   const std::vector<int> &hcount;
   int ent(int b, int l, int a) const { return blk[((size_t)b * ND + a) * 64 + l]; }
   int dof(int b, int l, int a) const { return ent(b, l, a) & 0x3fffffff; }
   bool held(int b, int l, int a) const { return holds[((size_t)b * 64 + l) * ND + a]; }
   bool held_shared(int b, int l, int a) const { return held(b, l, a) && hcount[dof(b, l, a)] > 1; }
};

// Regular block (the AFFINE kernel): the block's 64 elements a 4x4x4 lattice brick (lane = ex +
// 4 ey + 16 ez) of a lattice-numbered region, d = base + X sx + Y sy + Z sz on the block's
// (4(D-1)+1)^3 lattice, every dof owned, no orientation signs, and the held shared dofs exactly
// those on the block faces a 6-bit mask names.  The kernel then reads 5 ints per block instead of
// 64 ND map entries (C4: 136 MB per Mult and a dependent load chain at the gather and the store).
// (The brick version, brick_regular, walks lattice points and probes face centres instead of the
// held entries: two predicates, one face-mask rule, lattice_faces.)
bool block_regular(const BlockView &V, int b, int *r)
{
   const int D = V.D, L = 4 * (D - 1) + 1;
   const int base = V.dof(b, 0, 0), sx = V.dof(b, 0, 1) - base, sy = V.dof(b, 0, D) - base, sz = V.dof(b, 0, D * D) - base;
   int mask = 0;
   for (int l = 0; l < 64; l++)
      for (int a = 0; a < V.ND; a++)
      {
         const LatticeXYZ p = block_lattice_xyz(D, l, a);
         const unsigned g = (unsigned)V.ent(b, l, a);
         const int d = (int)(g & 0x3fffffffu);
         if ((g >> 31) || d >= V.n_owned || d != base + p.X * sx + p.Y * sy + p.Z * sz) { return false; }
         // a held entry on exactly one face sets that face's bit
         const int f = lattice_faces(L, L, L, p.X, p.Y, p.Z);
         if (V.held_shared(b, l, a) && f && !(f & (f - 1))) { mask |= f; }
      }
   for (int l = 0; l < 64; l++)
      for (int a = 0; a < V.ND; a++)
      {
         if (!V.held(b, l, a)) { continue; }
         const LatticeXYZ p = block_lattice_xyz(D, l, a);
         if ((V.hcount[V.dof(b, l, a)] > 1) != ((lattice_faces(L, L, L, p.X, p.Y, p.Z) & mask) != 0)) { return false; }
      }
   r[0] = base; r[1] = sx; r[2] = sy; r[3] = sz; r[4] = mask; r[7] = 1;
   return true;
}

// Lattice-slot block (flag 2): a complete block whose dofs are not a lattice (the reference's
// entity numbering) but whose held shared entries all sit on distinct points of the block
// surface: its partial slots are face-grouped like a regular block's, so the summation plan's
// runs stay long (with the dofs from its entry list).  Its dofs come from a block lattice map lm
// (tpe_lattice_slot order, one entry per lattice point): every entry of the block at one lattice
// point must encode the same dof, none with an orientation sign.
bool block_lattice_slots(const BlockView &V, int b, std::vector<int> &lm)
{
   std::vector<char> used(tpe_surface_points(V.D), 0);
   lm.assign(tpe_lattice_points(V.D), -1);
   for (int l = 0; l < 64; l++)
      for (int a = 0; a < V.ND; a++)
      {
         const LatticeXYZ p = block_lattice_xyz(V.D, l, a);
         const int g = V.ent(b, l, a);
         int &m = lm[tpe_lattice_slot(V.D, p.X, p.Y, p.Z)];
         if (((unsigned)g >> 31) || !(m < 0 || m == g)) { return false; }
         m = g;
      }
   for (int l = 0; l < 64; l++)
      for (int a = 0; a < V.ND; a++)
      {
         if (!V.held_shared(b, l, a)) { continue; }
         const LatticeXYZ p = block_lattice_xyz(V.D, l, a);
         const int si = tpe_surface_index(V.D, p.X, p.Y, p.Z);
         if (si < 0 || used[si]) { return false; }
         used[si] = 1;
      }
   return true;
}
} // namespace

// (brick blocks satisfy it by construction: lanes 3 and 4, or 12 and 16, are not x or y neighbours)
bool tpe_lane_flags_in_row(const int *flags64)
{
   for (int l = 0; l < 64; l++)
   {
      if (((flags64[l] & 1) && (l & 3) == 3) || ((flags64[l] & 4) && ((l >> 2) & 3) == 3) || ((flags64[l] & 16) && l >= 48)) { return false; }
   }
   return true;
}

TpePlan build_tpe_plan(int ne, int D, int ndofs, int n_owned, const std::vector<int> &gmap_host,
                       const std::vector<int> &perm_host, const std::vector<int> &splits, int latency_from,
                       bool lattice_layout, const PlanOptions &opt)
{
   const int ND = D * D * D, nblk = (ne + kElemBlock - 1) / kElemBlock;
   TpePlan P;
   P.perm_derived = perm_host.empty();
   P.perm = P.perm_derived ? derive_element_order(ne, D, gmap_host, splits) : perm_host;
   std::vector<int> gint((size_t)ne * ND);
   P.pos.resize(ne);
   for (int i = 0; i < ne; i++)
   {
      const int e = P.perm[i];
      P.pos[e] = i;
      std::copy(&gmap_host[(size_t)e * ND], &gmap_host[(size_t)e * ND] + ND, &gint[(size_t)i * ND]);
   }
   check_dof_bits(ndofs);
   ECM2_VERIFY((size_t)nblk * ND * 64 < (1ull << 31), ERR_UNSUPPORTED, "too many elements for int slots");
   std::vector<char> holds;
   std::vector<int> hcount;
   build_merge_plan(ne, D, gint, ndofs, holds, hcount, P.lane_flags, workgroup_groups(nblk, splits, latency_from, lattice_layout));
   P.gmap_blk.assign((size_t)nblk * ND * 64, 0);
   for (int i = 0; i < ne; i++)
   {
      const int b = i / 64, l = i % 64;
      for (int a = 0; a < ND; a++)
      {
         const int g = gint[(size_t)i * ND + a];
         P.gmap_blk[((size_t)b * ND + a) * 64 + l] = encode_entry(dofv(g), hcount[dofv(g)] > 1, g < 0);
      }
   }
   // Decided per block (a partitioned rank's interior blocks are regular, its boundary blocks are
   // not); treg_all / tlat_all when every block is.  Incomplete blocks, blocks the latency kernel
   // applies and blocks with an in-wave x / y link outside a 16-lane row (tpe_lane_flags_in_row)
   // store [a][lane] slots: neither regular nor lattice-slot.
   const BlockView V{D, ND, n_owned, P.gmap_blk, holds, hcount};
   const int ns = tpe_surface_points(D), NL = tpe_lattice_points(D);
   std::vector<char> unit(nblk, 0);  // 1 regular, 2 lattice slots
   if (lattice_layout)
   {
      std::vector<int> reg((size_t)nblk * 8, 0), lm;
      for (int b = 0; b < nblk; b++)
      {
         if ((long)(b + 1) * 64 > ne || (latency_from >= 0 && b >= latency_from)) { continue; }
         // The snapshot kernel's lattice epilogue moves the x and y faces by DPP row shifts.  (The block
         // classes are shared: the other lattice kernels -- k_apply_tpe_tlb, k_apply_tpe_sf, the diagonal --
         // shuffle through LDS and do not need the condition, but lose the class with it.  No brick fails it.)
         if (!tpe_lane_flags_in_row(&P.lane_flags[(size_t)b * 64])) { continue; }
         if (block_regular(V, b, &reg[(size_t)b * 8])) { unit[b] = 1; }
         else if (block_lattice_slots(V, b, lm))
         {
            reg[(size_t)b * 8 + 7] = 2;
            unit[b] = 2;
            if (P.lmap.empty()) { P.lmap.assign((size_t)nblk * NL, 0); }
            std::copy(lm.begin(), lm.end(), P.lmap.begin() + (size_t)b * NL);
         }
      }
      P.n_treg = (int)std::count(unit.begin(), unit.end(), 1);
      P.n_tlat = (int)std::count(unit.begin(), unit.end(), 2);
      if (P.n_treg || P.n_tlat)
      {
         P.treg = std::move(reg);
         P.treg_all = P.n_treg == nblk && (latency_from < 0 || latency_from >= nblk);
         P.tlat_all = P.n_tlat == nblk && (latency_from < 0 || latency_from >= nblk);
      }
   }
   P.part_stride = P.treg_all || P.tlat_all ? ns : ND * 64;
   // partial slots: [blk][a][lane]; on regular and lattice-slot blocks [blk][face-grouped surface
   // index of the block lattice] (tpe_surface_index: a face's two holders list it at the same
   // offset, so the summation pass reads both holders' runs contiguously)
   std::vector<int> hdof, hslot;
   for (int b = 0; b < nblk; b++)
      for (int a = 0; a < ND; a++)
         for (int l = 0; l < 64; l++)
         {
            if (!V.held_shared(b, l, a)) { continue; }
            hdof.push_back(V.dof(b, l, a));
            if (unit[b])
            {
               const LatticeXYZ p = block_lattice_xyz(D, l, a);
               const int si = tpe_surface_index(D, p.X, p.Y, p.Z);
               ECM2_VERIFY(si >= 0, ERR_INTERNAL, "block " << b << ": interior lattice point shared");  // (checked)
               hslot.push_back(b * P.part_stride + si);
            }
            else { hslot.push_back(b * P.part_stride + a * 64 + l); }
         }
   sort_holders_by_slot(hdof, hslot);
   P.shared = build_shared_plan(ndofs, n_owned, hcount, hdof, hslot, opt);
   return P;
}

// ---- line kernel family ----
namespace
{
// Regular brick: the brick's lattice map b[np] an affine function of the lattice point (d = base +
// X sx + Y sy + Z sz, a lattice-numbered mesh) and its shared points exactly those on the brick
// faces other holders touch (one face-mask bit per face) -- the kernel then computes dofs and
// shared flags from 5 ints per brick instead of reading the map
bool brick_regular(int LX, int LY, int LZ, const int *b, const std::vector<int> &hcount, int *r)
{
   const int base = b[0], sx = b[1] - base, sy = b[LX] - base, sz = b[LX * LY] - base;
   // face bit = sharing of a point inside that face (on no other face)
   const int cx = LX / 2, cy = LY / 2, cz = LZ / 2;
   const int probe[6][3] = {{0, cy, cz}, {LX - 1, cy, cz}, {cx, 0, cz}, {cx, LY - 1, cz}, {cx, cy, 0}, {cx, cy, LZ - 1}};
   int mask = 0;
   for (int f = 0; f < 6; f++)
   {
      if (hcount[b[(probe[f][2] * LY + probe[f][1]) * LX + probe[f][0]]] > 1) { mask |= 1 << f; }
   }
   r[0] = base; r[1] = sx; r[2] = sy; r[3] = sz; r[4] = mask;
   for (int p = 0; p < LX * LY * LZ; p++)
   {
      const int X = p % LX, Y = (p / LX) % LY, Z = p / (LX * LY);
      if (b[p] != base + X * sx + Y * sy + Z * sz) { return false; }
      if ((hcount[b[p]] > 1) != ((lattice_faces(LX, LY, LZ, X, Y, Z) & mask) != 0)) { return false; }
   }
   return true;
}
} // namespace

// Bricks of 2 x 2 x bz elements (deterministic scatter, both integrators) take every element they
// can; the leftovers run the per-element line kernel, listed per 64-element block (apply_blocks
// ranges map to list ranges).  Then the encoded maps and the deterministic-scatter plan over the
// holding entries: the bricks' lattice points, the leftovers' entries.
LinePlan build_line_plan(int ne, int D, int ndofs, int n_owned, const std::vector<int> &gmap_host,
                         const std::vector<int> &splits, int bz, const PlanOptions &opt)
{
   check_dof_bits(ndofs);
   const int ND = D * D * D, nblk = (ne + kElemBlock - 1) / kElemBlock;
   ECM2_VERIFY((size_t)ne * ND < (1ull << 31) && ne < (1 << 24), ERR_UNSUPPORTED,
               "too many elements for the line kernel's chunk table");
   LinePlan P;
   std::vector<char> in_brick(ne, 0);
   if (bz)
   {
      std::vector<int> seg(ne, 0);
      for (int e = 0; e < ne; e++)
      {
         for (int sp : splits) { seg[e] += (e / kElemBlock >= sp); }
      }
      find_bricks(ne, D, gmap_host, bz, seg, P.belem, in_brick);
   }
   const int nbe = 4 * (bz ? bz : 1);
   P.n_bricks = bz ? (int)(P.belem.size() / nbe) : 0;
   P.brick_bz = P.n_bricks ? bz : 0;
   const int LX = 2 * D - 1, LY = LX, LZ = P.brick_bz * (D - 1) + 1;
   P.brick_np = P.brick_bz ? LX * LY * LZ : 0;
   // lattice map of each brick (dof per lattice point; internal faces coincide by construction)
   std::vector<int> bdof((size_t)P.n_bricks * P.brick_np, -1);
   for (int k = 0; k < P.n_bricks; k++)
      for (int elt = 0; elt < nbe; elt++)
      {
         const int e = P.belem[(size_t)k * nbe + elt], ex = elt & 1, ey = (elt >> 1) & 1, ez = elt >> 2;
         for (int dz = 0; dz < D; dz++)
            for (int dy = 0; dy < D; dy++)
               for (int dx = 0; dx < D; dx++)
               {
                  const int p = ((ez * (D - 1) + dz) * LY + ey * (D - 1) + dy) * LX + ex * (D - 1) + dx;
                  const int d = dofv(gmap_host[(size_t)e * ND + (dz * D + dy) * D + dx]);
                  int &b = bdof[(size_t)k * P.brick_np + p];
                  ECM2_VERIFY(b < 0 || b == d, ERR_INTERNAL, "brick " << k << " lattice point " << p
                                                                 << " holds two dofs");
                  b = d;
               }
      }
   P.lelem_off.assign(nblk + 1, 0);
   P.brick_off.assign(nblk + 1, 0);
   std::vector<char> holds((size_t)ne * ND, 0);
   for (int bk = 0; bk < nblk; bk++)
   {
      for (int e = bk * 64; e < std::min(ne, bk * 64 + 64); e++)
      {
         if (in_brick[e]) { continue; }
         P.lelem.push_back(e);
         for (int a = 0; a < ND; a++) { holds[(size_t)e * ND + a] = 1; }
      }
      P.lelem_off[bk + 1] = (int)P.lelem.size();
   }
   P.n_left = (int)P.lelem.size();
   for (int k = 0, bk = 0; bk < nblk; bk++)
   {
      while (k < P.n_bricks && P.belem[(size_t)k * nbe] / kElemBlock == bk) { k++; }
      P.brick_off[bk + 1] = k;
   }
   ECM2_VERIFY(P.brick_off[nblk] == P.n_bricks, ERR_INTERNAL, "bricks not ordered by first element");
   std::vector<int> hcount(ndofs, 0);
   for (int d : bdof) { hcount[d]++; }
   for (size_t i = 0; i < gmap_host.size(); i++) { if (holds[i]) { hcount[dofv(gmap_host[i])]++; } }
   // brick partial slots: [brick][face-grouped surface index]; only surface points can be
   // shared (a brick holds its interior lattice points alone: checked)
   const int nsurf = P.brick_bz ? brick_surface_points(D, P.brick_bz) : 0;
   P.part_line_off = (long)P.n_bricks * nsurf;
   ECM2_VERIFY(P.part_line_off + (long)nblk * ND * 64 < (1l << 31), ERR_UNSUPPORTED, "too many partial slots");
   std::vector<int> hdof, hslot;
   P.bmap.resize(bdof.size());
   for (size_t i = 0; i < bdof.size(); i++)
   {
      P.bmap[i] = encode_entry(bdof[i], hcount[bdof[i]] > 1, false);
      if (hcount[bdof[i]] > 1)
      {
         const int k = (int)(i / P.brick_np), p = (int)(i % P.brick_np);
         const int si = brick_surface_index(D, P.brick_bz, p % LX, (p / LX) % LY, p / (LX * LY));
         ECM2_VERIFY(si >= 0, ERR_INTERNAL, "brick " << k << ": interior lattice point " << p << " is shared");
         hdof.push_back(bdof[i]);
         hslot.push_back(k * nsurf + si);
      }
   }
   sort_holders_by_slot(hdof, hslot);  // (the leftovers' slots below are ascending and above the bricks')
   P.gmap_line.resize(gmap_host.size());
   for (size_t i = 0; i < gmap_host.size(); i++)
   {
      const int g = gmap_host[i], d = dofv(g);
      P.gmap_line[i] = encode_entry(d, hcount[d] > 1, g < 0);
      if (holds[i] && hcount[d] > 1)
      {
         hdof.push_back(d);
         hslot.push_back((int)(P.part_line_off + (long)i));
      }
   }
   P.shared = build_shared_plan(ndofs, n_owned, hcount, hdof, hslot, opt);
   if (P.n_bricks && n_owned == ndofs)
   {
      P.breg.assign((size_t)P.n_bricks * 8, 0);
      for (int k = 0; k < P.n_bricks; k++)
      {
         if (!brick_regular(LX, LY, LZ, &bdof[(size_t)k * P.brick_np], hcount, &P.breg[(size_t)k * 8])) { P.breg.clear(); break; }
      }
   }
   return P;
}

} // namespace ecm2
