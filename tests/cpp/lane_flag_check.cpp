// lane_flag_check.cpp -- CPU check of the merge-flag condition the lattice blocks' epilogue rests on
// (tpe_assemble_store_lattice, k_tpe.hip; tpe_lane_flags_in_row, csrc/scatter_plan.hpp).
//
// The epilogue moves the x and y faces of a 4 x 4 x 4 block with DPP row shifts by 1 and 4 lanes, which
// reach only the lanes of the receiver's 16-lane row (lane = ex + 4 ey + 16 ez).  So on every block the
// planner classes regular or lattice-slot, an in-wave x receive bit must sit on a lane with ex < 3 and
// a y receive bit on a lane with ey < 3 (and a z receive bit on a lane below 48: the z permute reads lane
// l + 16); a block with such a bit elsewhere must get neither class.
// Checked on the thread-per-element plans of the meshes of tests/test_gpu_ts_epilogue_bitwise.py in
// both numberings (element orders as the Python binding passes them), on a z-slab rank's local form,
// and on a doctored one-block map whose lane 3 receives from lane 4.
// Links scatter_plan.cpp, bricks.cpp, mesh.cpp, fe.cpp and partition.cpp only; meant to run under
// ASan + UBSan (tests/test_lane_flags_host.py).
#include "kernels.hpp"
#include "mesh.hpp"
#include "partition.hpp"
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

// the row condition, written out lane by lane (not through tpe_lane_flags_in_row)
static bool in_row(const TpePlan &P, int b)
{
   for (int l = 0; l < 64; l++)
   {
      const int fl = P.lane_flags[(size_t)b * 64 + l], ex = l & 3, ey = (l >> 2) & 3;
      if ((fl & 1) && ex == 3) { return false; }
      if ((fl & 4) && ey == 3) { return false; }
      if ((fl & 16) && l >= 48) { return false; }
   }
   return true;
}

// every lattice block of the plan satisfies the condition; returns how many there are
static int check_plan(const char *name, const TpePlan &P, int nblk)
{
   g_case = name;
   CHECK(P.lane_flags.size() == (size_t)nblk * 64, "flags of %d blocks", nblk);
   int lattice = 0, in_wave = 0;
   for (int b = 0; b < nblk; b++)
   {
      const int unit = P.treg.empty() ? 0 : P.treg[(size_t)b * 8 + 7];
      CHECK(in_row(P, b) == tpe_lane_flags_in_row(&P.lane_flags[(size_t)b * 64]), "block %d: the planner's predicate", b);
      if (!unit) { continue; }
      lattice++;
      CHECK(in_row(P, b), "lattice block %d (class %d) has a receive bit outside its DPP row", b, unit);
      for (int l = 0; l < 64; l++)
      {
         const int fl = P.lane_flags[(size_t)b * 64 + l];
         in_wave += (fl & 1) + ((fl >> 2) & 1);
         CHECK(!(fl & 16) || l < 48, "block %d lane %d receives z from beyond the wave", b, l);
      }
   }
   CHECK(lattice == P.n_treg + P.n_tlat, "%d lattice blocks, plan says %d + %d", lattice, P.n_treg, P.n_tlat);
   std::printf("ok  %-44s blocks %d regular %d lattice-slot %d in-wave x/y receives %d\n", name, nblk, P.n_treg, P.n_tlat, in_wave);
   return lattice;
}

int main()
{
   try
   {
      const int meshes[5][3] = {{4, 4, 4}, {8, 8, 4}, {4, 4, 8}, {8, 8, 8}, {12, 12, 12}};
      for (const auto &n : meshes)
      {
         for (int numbering : {NUMBERING_STRUCTURED, NUMBERING_ENTITY})
         {
            // (the binding: structured -- the mesh's brick order; entity -- the reference's MakeCartesian3D
            // element order, the form derives face-linked bricks from the map)
            const bool ent = numbering == NUMBERING_ENTITY;
            const HexMesh m = HexMesh::cartesian(n[0], n[1], n[2], 1.0, 1.0, 1.0, ent);
            const H1Space h = H1Space::build(m, 2, numbering);
            const std::vector<int> perm = ent ? std::vector<int>() : element_order(m, ORDER_BRICK);
            const TpePlan P = build_tpe_plan(h.ne, 3, h.ndofs, h.ndofs, h.gather_map, perm, {}, -1, true, {});
            const std::string name = std::to_string(n[0]) + "x" + std::to_string(n[1]) + "x" + std::to_string(n[2]) +
                                     (ent ? " entity" : " structured");
            const int nblk = h.ne / 64;
            CHECK(check_plan(name.c_str(), P, nblk) == nblk, "every block of the mesh is a lattice block");
            CHECK(ent ? P.tlat_all : P.treg_all, "block class of the numbering");
            // a brick's interior links: 3 x and 3 y receivers in each of its 16 rows
            for (int b = 0; b < nblk; b++)
               for (int l = 0; l < 64; l++)
               {
                  const int fl = P.lane_flags[(size_t)b * 64 + l];
                  CHECK(((fl & 1) != 0) == ((l & 3) < 3) && ((fl & 4) != 0) == (((l >> 2) & 3) < 3),
                        "block %d lane %d: flags %#x", b, l, fl);
               }
         }
      }
      {
         // a z-slab rank's local form (OVERLAP decomposition, one launch over [interior | boundary])
         const HexMesh m = HexMesh::cartesian(8, 8, 8, 1.0, 1.0, 1.0);
         const H1Space h = H1Space::build(m, 2, NUMBERING_STRUCTURED);
         const std::vector<int> er = partition_slabs_z(m, 2);
         for (int rank = 0; rank < 2; rank++)
         {
            const LocalPart part = build_local_part(h, er, rank, 2, &m, true);
            const int nblk = (part.ne_local + 63) / 64, bi = part.ne_interior / 64;
            const TpePlan P = build_tpe_plan(part.ne_local, 3, part.n_owned + part.n_ghost, part.n_owned, part.gather_map, {},
                                             {bi / 4 * 4}, -1, true, {});
            const std::string name = "8x8x8 z-slab rank " + std::to_string(rank) + " of 2, local form";
            CHECK(check_plan(name.c_str(), P, nblk) > 0, "the rank has lattice blocks");
         }
      }
      {
         // One 4x4x4 brick whose element 4 = (0, 1, 0) has, as its low x face, the dofs of the high x
         // face of element 3 = (3, 0, 0): lane 3 then receives x from lane 4, across the row's end of
         // the x links (ex = 3).  The block must be classed neither regular nor lattice-slot.
         const HexMesh m = HexMesh::cartesian(4, 4, 4, 1.0, 1.0, 1.0);
         const H1Space h = H1Space::build(m, 2, NUMBERING_STRUCTURED);
         std::vector<int> sub(h.ndofs);
         for (int d = 0; d < h.ndofs; d++) { sub[d] = d; }
         for (int j = 0; j < 3; j++)
            for (int i = 0; i < 3; i++) { sub[h.gather_map[4 * 27 + (j * 3 + i) * 3 + 0]] = h.gather_map[3 * 27 + (j * 3 + i) * 3 + 2]; }
         std::vector<int> gm(h.gather_map.size()), newid(h.ndofs, -1);
         int nd = 0;
         for (size_t k = 0; k < gm.size(); k++)
         {
            const int d = sub[h.gather_map[k]];
            if (newid[d] < 0) { newid[d] = nd++; }
            gm[k] = newid[d];
         }
         CHECK(nd == h.ndofs - 9, "nine dofs identified, %d left of %d", nd, h.ndofs);
         const TpePlan P = build_tpe_plan(h.ne, 3, nd, nd, gm, element_order(m, ORDER_BRICK), {}, -1, true, {});
         g_case = "4x4x4 with lane 3 linked to lane 4";
         CHECK(P.lane_flags[3] & 1, "lane 3 does not receive x: flags %#x", P.lane_flags[3]);
         CHECK(P.lane_flags[4] & 2, "lane 4 does not send x: flags %#x", P.lane_flags[4]);
         CHECK(!in_row(P, 0) && !tpe_lane_flags_in_row(&P.lane_flags[0]), "the row condition holds");
         CHECK(P.n_treg == 0 && P.n_tlat == 0 && !P.treg_all && !P.tlat_all && (P.treg.empty() || P.treg[7] == 0),
               "a block with a receive bit outside its DPP row is a lattice block");
         CHECK(P.part_stride == 27 * 64, "[a][lane] partial slots");
         check_plan(g_case.c_str(), P, 1);
      }
   }
   catch (const Error &e)
   {
      std::printf("FAIL [%s] ecm2 error %d: %s\n", g_case.c_str(), e.code, e.what());
      return 1;
   }
   std::printf("PASS\n");
   return 0;
}
