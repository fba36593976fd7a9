// scatter_plan.hpp -- host-side planning of the fused kernels' deterministic scatter.
//
// Everything the scatter depends on is decided here, from the element->dof map alone: the derived
// element order, the in-wave / cross-wave merge flags, the blocked and encoded dof maps, which
// 4 x 4 x 4 blocks and 2 x 2 x bz bricks are lattice units, the partial-slot numbering and the
// run-compressed summation plan kern::sum_partials executes.  Free functions over plain vectors
// (like bricks.hpp, partition.hpp): no device, no stream, no PAForm.  Each plan's scalars are a small
// ...Info base that its device-side owner (plan_dev.hpp) copies whole.  PAForm::assemble calls the
// builders and uploads what they return; tests/cpp/plan_check.cpp replays them on the host.
#pragma once

#include <vector>

namespace ecm2
{

struct PlanOptions
{
   int run_order = -1;  // summation-run order: -1 decided by the lines touched, 0 slot, 1 dof, 2 chain
   bool dump = false;   // print the run-order decision and the run classes to stderr
};
// ECM2_RUN_ORDER=slot|dof|chain and ECM2_PLAN_DUMP (set: dump)
PlanOptions plan_options_from_env();

// Second-pass plan of the deterministic scatter (kern::sum_partials): every dof not held exactly
// once, the owned ones first, then the ghosts.
struct SharedPlanInfo
{
   int n_sh = 0, n_sh_owned = 0, nblk_owned = 0, nblk = 0;
   long n_slots = 0, n_runs = 0, n_explicit_runs = 0;
};
struct SharedPlan : SharedPlanInfo
{
   std::vector<int> runs;    // [n_runs + 1][12] run descriptors, sentinel row last
   std::vector<int> rslots;  // first slots of every run's holders (read for holders past the fourth)
   std::vector<int> blocks;  // [nblk][4]: first run, end run, first entry, entries | explicit << 30
   std::vector<int> pdof;    // plan entry -> dof
};
// hcount[d]: holders of dof d; (hdof[i], hslot[i]): the holders of the dofs held more than once
SharedPlan build_shared_plan(int ndofs, int n_owned, const std::vector<int> &hcount, const std::vector<int> &hdof,
                             const std::vector<int> &hslot, const PlanOptions &opt);

// lattice point of entry a of lane `lane` in a 4 x 4 x 4 block (lane = ex + 4 ey + 16 ez)
struct LatticeXYZ { int X, Y, Z; };
inline LatticeXYZ block_lattice_xyz(int D, int lane, int a)
{
   return {(D - 1) * (lane & 3) + a % D, (D - 1) * ((lane >> 2) & 3) + (a / D) % D, (D - 1) * (lane >> 4) + a / (D * D)};
}

// Thread-per-element kernel (p <= 2): 64 elements per block, one per lane.
struct TpePlanInfo
{
   int n_treg = 0, n_tlat = 0, part_stride = 0;  // regular blocks, lattice-slot blocks, partial slots per block
   bool treg_all = false, tlat_all = false;      // every block regular / a lattice-slot block
};
struct TpePlan : TpePlanInfo
{
   std::vector<int> perm;       // internal position -> caller element (the order used)
   bool perm_derived = false;   // derived here (face_brick_order per apply segment), not the caller's
   std::vector<int> pos;        // caller element -> internal position
   std::vector<int> gmap_blk;   // [blk][nd][64]: dof | shared << 30 | sign << 31
   std::vector<int> lane_flags; // [blk][64] merge flags (build_merge_plan)
   std::vector<int> treg;       // [blk][8]: base, sx, sy, sz, face mask, -, -, 1 regular / 2 lattice slots; empty: none
   std::vector<int> lmap;       // [blk][tpe_lattice_points] lattice maps; empty: no lattice-slot block
   SharedPlan shared;
};
// What the lattice blocks' epilogue (tpe_assemble_store_lattice, k_tpe.hip) needs of a block's 64 merge
// flags (lane = ex + 4 ey + 16 ez): an in-wave x receive bit (1) only on lanes with ex < 3 and a y
// receive bit (4) only on lanes with ey < 3, so the sending lane l + 1 / l + 4 lies in the receiver's
// 16-lane DPP row; and a z receive bit (16) only on lanes below 48, so lane l + 16 exists.  build_tpe_plan
// classes a block that fails it neither regular nor lattice-slot, for every kernel that reads the classes.
bool tpe_lane_flags_in_row(const int *flags64);
// perm_host empty: derive the order.  lattice_layout: the AFFINE / TRILINEAR qdata layouts (cross-wave
// links, regular and lattice-slot blocks).
TpePlan build_tpe_plan(int ne, int D, int ndofs, int n_owned, const std::vector<int> &gmap_host,
                       const std::vector<int> &perm_host, const std::vector<int> &splits, int latency_from,
                       bool lattice_layout, const PlanOptions &opt);

// Line kernel family (p >= 3): bricks of 2 x 2 x bz elements, the other elements one by one.
struct LinePlanInfo
{
   int n_bricks = 0, brick_bz = 0, brick_np = 0, n_left = 0;  // bricks, 2 x 2 x bz, lattice points, elements outside bricks
   long part_line_off = 0;  // the leftover elements' [e][nd] partial slots start here
};
struct LinePlan : LinePlanInfo
{
   std::vector<int> gmap_line;  // [e][nd]: dof | shared << 30 | sign << 31
   std::vector<int> lelem;      // elements outside bricks
   std::vector<int> lelem_off;  // those of block b: [lelem_off[b], lelem_off[b + 1])
   std::vector<int> belem;      // [nbrick][4 bz] members
   std::vector<int> bmap;       // [nbrick][np] encoded lattice maps
   std::vector<int> brick_off;  // bricks of block b: [brick_off[b], brick_off[b + 1])
   std::vector<int> breg;       // [nbrick][8]: base, sx, sy, sz, face mask; empty unless every brick is regular
   SharedPlan shared;
};
LinePlan build_line_plan(int ne, int D, int ndofs, int n_owned, const std::vector<int> &gmap_host,
                         const std::vector<int> &splits, int bz, const PlanOptions &opt);

} // namespace ecm2
