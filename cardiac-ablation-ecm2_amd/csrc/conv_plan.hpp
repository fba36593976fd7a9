// conv_plan.hpp -- host-only planning of the convection term (conv_term.hpp): which elements are
// kept, their gather rows in the apply kernel's layout, and the CSR that adds the term's E-vector into
// an L-vector.  A pure function of plain vectors (no device, stream or form), like scatter_plan.hpp's
// builders, so a stand-alone program can run it under sanitizers (tests/cpp/conv_plan_check.cpp).
//
// Reference mirrored:
//   ElementRestriction's offsets / indices     fem/restriction.cpp:68-106 (index -1 - lid = minus sign)
//   AddMultWithMarkers over elem_attributes    fem/bilinearform_ext.cpp:753-774 (an excluded element's
//                                              E-vector rows are zero: here they do not exist)
#pragma once

#include <vector>

namespace ecm2
{

constexpr int kConvBlock = 64;  // elements per wave of the thread-per-element convection kernel

struct ConvPlan
{
   int n_act = 0;               // active elements
   int n_rows = 0;              // dofs some active element touches
   int blocked = 0;             // layout of map and of the E-vector (below)
   size_t ev_size = 0;          // doubles of the E-vector scratch
   std::vector<int> act;        // [n_act] element indices, ascending
   // the active elements' gather rows (entries as in the gather map: g, or -1 - g for a minus sign)
   //   blocked: [blk][nd][64], lanes past n_act repeat the block's first element (in-bounds loads)
   //   else:    [n_act][nd]
   std::vector<int> map;
   // rows: the touched dofs, ascending; a row's entries are E-vector positions in ascending (element,
   // local index) order, -1 - position for a minus sign (build_restriction_csr's encoding)
   std::vector<int> csr_dof, csr_off, csr_idx;
};

// E-vector position of local dof i of active element k
inline size_t conv_ev_index(bool blocked, int nd, int k, int i)
{
   return blocked ? ((size_t)(k / kConvBlock) * nd + i) * kConvBlock + (k % kConvBlock) : (size_t)k * nd + i;
}

// gather_map [ne][nd]; keep [ne]: non-zero = the element is active.  Throws ecm2::Error (ERR_ARG) on
// a map entry outside [0, ndofs).
ConvPlan build_conv_plan(const std::vector<int> &gather_map, int ne, int nd, int ndofs,
                         const std::vector<unsigned char> &keep, bool blocked);

} // namespace ecm2
