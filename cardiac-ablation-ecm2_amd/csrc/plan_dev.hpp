// plan_dev.hpp -- the device side of the scatter plans scatter_plan.hpp builds: each struct owns one
// plan's scalars (the builder's ...Info, copied whole), its arrays on the device and the few host
// vectors the launches and the qdata export read.  PAForm holds one of each; `valid` says whether
// the plan still matches the form's inputs (PAForm::invalidate_plans).
#pragma once

#include "common.hpp"
#include "scatter_plan.hpp"

#include <vector>

namespace ecm2
{

// kern::sum_partials' plan (PAForm::finish_shared): uploaded with the TPE or the LINE plan it belongs
// to, so it is current whenever that one is (no flag of its own)
struct SharedPlanDev
{
   SharedPlanInfo info;
   // runs [n_runs + 1][12], the first slots of holders beyond the fourth, blocks [nblk][4] (owned runs'
   // blocks first), plan entry -> dof (runs whose dofs are not affine read it)
   DeviceArray<int> runs, rslots, blocks, pdof;

   void upload(const SharedPlan &p, hipStream_t s)
   {
      info = p;
      runs.upload(p.runs, s);
      // (the summation kernel wants non-null pointers)
      rslots.upload(p.rslots.empty() ? std::vector<int>{0} : p.rslots, s);
      blocks.upload(p.blocks.empty() ? std::vector<int>{0, 0, 0, 0} : p.blocks, s);
      pdof.upload(p.pdof.empty() ? std::vector<int>{0} : p.pdof, s);
   }
};

// Thread-per-element kernels (p <= 2)
struct TpePlanDev
{
   TpePlanInfo info;
   bool valid = false;
   int kind = -1;                 // qdata layout the plan (merges, regular blocks, slots) was built for
   std::vector<int> perm;         // internal position -> caller element: the order used (caller's or derived)
   DeviceArray<int> gmap_blk;     // blocked [blk][nd][64] (internal element order)
   DeviceArray<int> lane_flags;   // [blk][64] in-wave merge flags
   DeviceArray<int> treg;         // [nblk][8] (base, sx, sy, sz, face mask, -, -, flag 1 regular / 2 lattice slots)
   DeviceArray<int> lmap;         // lattice-slot blocks' lattice maps [nblk][tpe_lattice_points] (tpe_lattice_slot order)
   DeviceArray<int> pos, perm_dev;  // caller element -> internal position, and back

   // (the caller synchronises s before p goes away)
   void upload(const TpePlan &p, int layout_kind, hipStream_t s)
   {
      info = p;
      kind = layout_kind;
      perm = p.perm;
      gmap_blk.upload(p.gmap_blk, s);
      lane_flags.upload(p.lane_flags, s);
      treg.upload(p.treg, s);
      lmap.upload(p.lmap, s);
      pos.upload(p.pos, s);
      perm_dev.upload(p.perm, s);
      valid = true;
   }
   void reset()
   {
      info = {};
      valid = false;
      kind = -1;
   }
};

// Line kernel family (p >= 3); every qdata layout shares one plan
struct LinePlanDev
{
   LinePlanInfo info;
   bool valid = false;
   std::vector<int> lelem_off;    // listed elements of block b = [lelem_off[b], lelem_off[b + 1])
   std::vector<int> brick_off;    // bricks of block b = [brick_off[b], brick_off[b + 1])
   DeviceArray<int> gmap_line;    // [e][nd] dof | shared << 30 | sign << 31
   DeviceArray<int> lelem;        // elements outside bricks
   DeviceArray<int> belem, bmap;  // bricks: [nbrick][4 bz] elements, [nbrick][np] lattice map
   DeviceArray<int> breg;         // lattice-numbered bricks: [nbrick][8] (base, sx, sy, sz, face mask)

   void upload(const LinePlan &p, hipStream_t s)
   {
      info = p;
      lelem_off = p.lelem_off;
      brick_off = p.brick_off;
      gmap_line.upload(p.gmap_line, s);
      lelem.upload(p.lelem.empty() ? std::vector<int>{0} : p.lelem, s);  // (non-null for the launcher)
      belem.upload(p.belem, s);
      bmap.upload(p.bmap, s);
      breg.upload(p.breg, s);
      valid = true;
   }
   void reset()
   {
      info = {};
      valid = false;
   }
};

} // namespace ecm2
