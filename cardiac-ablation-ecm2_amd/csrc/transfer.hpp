// transfer.hpp -- the transfer operator between a coarse and a fine H1 space, of either kind, and the host-side
// construction of its plan:
//   p-refinement: orders pc < pf on the same elements;
//   h-refinement: one order p on a hex mesh and on its uniform refinement.
// Both are one operator: a unit of work (an element; a parent) has NCH children (the element itself; its eight
// fine elements), and child o of a unit maps the unit's coarse dofs by B_oz (x) B_oy (x) B_ox.  The p kind is the h
// kind with one child per unit and one table.
//
// Reference, p kind:
//   TensorProductPRefinementTransferOperator   fem/transfer.cpp:2223-2287 (constructor)
//   TransferKernels::Prolongation3D            fem/transfer.cpp:2338-2423
//   TransferKernels::Restriction3D             fem/transfer.cpp:2470-2539
//   Mult / MultTranspose                       fem/transfer.cpp:2542-2592
//   ElementRestriction::BooleanMask            fem/restriction.cpp:248-283
// Reference, h kind:
//   FiniteElementSpace::RefinementOperator         fem/fespace.cpp:1833-2120 (Mult :1942-2019, MultTranspose :2021-2120)
//   FiniteElementSpace::GetLocalRefinementMatrices fem/fespace.cpp:1786-1807
//   ScalarFiniteElement::NodalLocalInterpolation   fem/fe/fe_base.cpp:860-895 (entries below 1e-12 set to zero)
//   CoarseFineTransformations::embeddings          mesh/mesh.hpp (parent and point matrix of every fine element)
//   TransferOperator's choice of it                fem/transfer.cpp:2055-
//
// Each space is given by its gather map [ne][(p + 1)^3] (lexicographic local dofs, x fastest, the caller's
// element order, as ecm2_pa_form_create takes it), an h-refinement also by an embedding per fine element:
// parent[f] and octant[f] = ox + 2 oy + 4 oz in the parent's lexicographic frame.  Nothing else about the spaces
// or the meshes is read, so any pair of numberings, any element order and any geometry is admitted: as in the
// reference the transfer is geometry-free.
//   Mult (prolongation):  y_f = R_f^T mask (B_oz (x) B_oy (x) B_ox) R_c x_c.  mask is 1 at an L-dof's first
//     occurrence in the fine E-vector -- in the lowest-numbered fine element that holds it (BooleanMask; the
//     `processed` marks of RefinementOperator::MultTranspose) -- and 0 elsewhere, so every fine dof is written
//     once, by its owner: y is overwritten, no zero fill, no atomics.  (RefinementOperator::Mult lets the last
//     element's SetSubVector stand; the elements that share a dof compute the same value up to rounding.)
//   MultTranspose (restriction):  y_c = R_c^T sum_children (B_oz^T (x) B_oy^T (x) B_ox^T) mask R_f x_f, a unit's
//     children summed in ascending octant order into a coarse E-vector, then the elements that share a coarse dof
//     in ascending E-vector order through the coarse space's transposed map (a CSR): no atomics, y overwritten.
// The tables B[o][q + Df d] (Df = pf + 1):
//   p kind, table 0 alone: the coarse GLL Lagrange basis function d at the fine GLL node q (fe.cpp's gauss_lobatto
//     and basis_eval, as the reference's DofToQuad of the coarse element at the fine element's nodes).
//   h kind, o = 0, 1: l_d((o + xi_q) / 2), xi the GLL nodes on [0, 1], l_d the GLL Lagrange basis.  The children
//     of the reference's hex refinement keep the parent's axes (child k sits at native corner k,
//     HexMesh::refine_uniform), so these two serve every octant.  The reference zeroes the entries of the dense
//     D^3 x D^3 matrix below 1e-12; here the 1D tables are thresholded.  For p <= 4 that is the same set of
//     zeros: a 1D entry is either an exact 0 where the child's node is a parent's node (at worst a rounding
//     residue below 1e-15) or at least 0.0319 in magnitude (p = 4; 0.0559 at p = 3, 0.125 at p = 2, 0.5 at
//     p = 1), and none exceeds 1; so a 3D product with such a factor is below 1e-15 < 1e-12 and one without is
//     above 0.0319^3 = 3.2e-5 > 1e-12 (tests/test_hmg_reference.py checks the figures and the equality of the
//     zero patterns).
// The mask is not stored as ne Df^3 doubles: the plan holds owner bits, two 64-bit words per fine element
// (Df^3 <= 125), bit i of word i / 64 for local fine dof i.
#pragma once

#include "common.hpp"

#include <cstdint>
#include <vector>

namespace ecm2
{

constexpr int kTransferMaxOrder = 4;                // kernels exist for 1 <= pc < pf <= 4 (p) and 1 <= p <= 4 (h)
constexpr int kTransferMaxD = kTransferMaxOrder + 1;
constexpr double kHTransferZero = 1e-12;            // fe_base.cpp:884-893

enum TransferKind : int
{
   TRANSFER_P = 0,  // two orders on one mesh: every element is its own single child
   TRANSFER_H = 1   // one order on a mesh and its uniform refinement: eight children per parent
};

// Kernel-argument copy of the 1D tables (read with scalar loads where the index is a constant).  One type for both
// kinds: the p kernels are passed the second table too and never read it.
struct TransferBasis
{
   double B[2][kTransferMaxD * kTransferMaxD];  // [o][q + Df d]
};

// What the host builds (plain C++; tests/cpp/transfer_plan_check.cpp replays it on the CPU)
struct TransferPlan
{
   TransferKind kind = TRANSFER_P;
   int ne_c = 0, ne_f = 0, pc = 0, pf = 0, nc = 0, nf = 0;  // (p: ne_c == ne_f; h: pc == pf)
   TransferBasis basis = {};
   std::vector<uint64_t> owner;   // [ne_f][2] owner bits of the fine E-vector
   std::vector<int> children;     // h: [ne_c][8], the fine element at octant o of parent i; p: empty
   std::vector<int> c_off, c_idx; // the coarse space's transposed map: row c lists its E-vector entries e Dc^3 + a, ascending
};

// The two thresholded 1D tables of the h kind at order p (1..4)
TransferBasis htransfer_basis(int p);

// Validates both maps and builds the p plan.  pc >= pf, ne < 0, a null map: ERR_ARG; an order outside 1..4:
// ERR_UNSUPPORTED; an entry >= ndofs: ERR_ARG; a negative (signed) entry: ERR_UNSUPPORTED (H1 has none); a fine
// dof that no element holds (it would never be written): ERR_ARG.
TransferPlan build_transfer_plan(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f);

// Validates both maps and the embedding and builds the h plan.  A null map or embedding, a negative size, a map
// entry >= ndofs, a fine dof that no element holds, a parent outside 0..ne_c - 1, an octant outside 0..7: ERR_ARG;
// an order outside 1..4, a negative (signed) entry, a parent that does not have exactly one child per octant
// (non-conforming or partial refinement): ERR_UNSUPPORTED.
TransferPlan build_htransfer_plan(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                                  const int *parent, const int *octant);

// The device operator, what the multigrid cycle and the C handle hold.  Vectors are device L-vectors of nc (coarse)
// and nf (fine) doubles; the kernels read and write single entries through the maps, so no alignment beyond a
// double's is asked.  Two calls are bitwise equal.
class Transfer
{
public:
   static Transfer p_refinement(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f);
   static Transfer h_refinement(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                                const int *parent, const int *octant);
   int ne() const { return ne_f_; }      // elements of the fine space
   int order_lo() const { return pc_; }
   int order_hi() const { return pf_; }
   int width() const { return nc_; }     // the coarse space's size (Operator::Width)
   int height() const { return nf_; }    // the fine space's size (Operator::Height)
   size_t plan_bytes() const;            // both maps, the owner words, the children table and the transposed map on the device
   void mult(const double *x_c, double *y_f, hipStream_t s) const;
   void mult_transpose(const double *x_f, double *y_c, hipStream_t s) const;

private:
   Transfer(const TransferPlan &p, const int *gather_c, const int *gather_f);  // uploads a validated plan
   TransferKind kind_;
   int ne_c_, ne_f_, pc_, pf_, nc_, nf_;
   TransferBasis basis_;
   DeviceArray<int> gc_, gf_, children_, c_off_, c_idx_;
   DeviceArray<uint64_t> owner_;
   mutable DeviceArray<double> ye_;  // the restriction's coarse E-vector [ne_c][Dc^3]
};

} // namespace ecm2
