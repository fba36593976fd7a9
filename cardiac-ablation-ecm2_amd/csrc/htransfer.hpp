// htransfer.hpp -- the h-refinement transfer operator between an H1 space on a hex mesh and the H1 space of the
// same order p on its uniform refinement, and the host-side construction of its plan.
//
// Reference:
//   FiniteElementSpace::RefinementOperator         fem/fespace.cpp:1833-2120 (Mult :1942-2019, MultTranspose :2021-2120)
//   FiniteElementSpace::GetLocalRefinementMatrices fem/fespace.cpp:1786-1807
//   ScalarFiniteElement::NodalLocalInterpolation   fem/fe/fe_base.cpp:860-895 (entries below 1e-12 set to zero)
//   CoarseFineTransformations::embeddings          mesh/mesh.hpp (parent and point matrix of every fine element)
//   TransferOperator's choice of it                fem/transfer.cpp:2055-
//
// Each space is given by its gather map [ne][D^3] (D = p + 1, lexicographic local dofs, x fastest), the refinement
// by an embedding per fine element: parent[f] and octant[f] = ox + 2 oy + 4 oz in the parent's lexicographic frame.
// Nothing else about either mesh is read: as in the reference the transfer is geometry-free.  The children of the
// reference's hex refinement keep the parent's axes (child k sits at native corner k, HexMesh::refine_uniform), so
// the local matrix of octant (ox, oy, oz) is B_oz (x) B_oy (x) B_ox with
//   B_o[q + D d] = l_d((o + xi_q) / 2),  xi the GLL nodes on [0, 1], l_d the GLL Lagrange basis.
// The reference zeroes the entries of the dense D^3 x D^3 matrix below 1e-12; here the 1D tables are thresholded.
// For p <= 4 that is the same set of zeros: a 1D entry is either an exact 0 where the child's node is a parent's
// node (at worst a rounding residue below 1e-15) or at least 0.0319 in magnitude (p = 4; 0.0559 at p = 3, 0.125
// at p = 2, 0.5 at p = 1), and none exceeds 1; so a 3D product with such a factor is below 1e-15 < 1e-12 and one
// without is above 0.0319^3 = 3.2e-5 > 1e-12 (tests/test_hmg_reference.py checks the figures and the equality of
// the zero patterns).
//   Mult (prolongation):  y_f = R_f^T mask (B_o (x) B_o (x) B_o) R_c x_c.  mask is 1 where the fine element is the
//     lowest-numbered one that holds the dof -- the `processed` marks of RefinementOperator::MultTranspose, kept as
//     the owner bits of transfer.hpp -- so every fine dof is written once: y is overwritten, no zero fill, no
//     atomics.  (The reference's Mult lets the last element's SetSubVector stand; the elements that share a dof
//     compute the same value up to rounding.)
//   MultTranspose (restriction):  y_c = R_c^T sum_children (B_o^T (x) B_o^T (x) B_o^T) mask R_f x_f, a parent's eight
//     children summed in ascending octant order into a coarse E-vector, then the elements that share a coarse dof
//     in ascending order through the coarse space's transposed map: no atomics, y overwritten.
#pragma once

#include "transfer.hpp"

namespace ecm2
{

constexpr int kHTransferMaxD = kTransferMaxOrder + 1;  // kernels exist for 1 <= p <= 4
constexpr double kHTransferZero = 1e-12;               // fe_base.cpp:884-893

// Kernel-argument copy of the two 1D tables
struct HTransferBasis
{
   double B[2][kHTransferMaxD * kHTransferMaxD];  // [o][q + D d]
};

// What the host builds (plain C++; tests/cpp/htransfer_plan_check.cpp replays it on the CPU)
struct HTransferPlan
{
   int p = 0, ne_c = 0, ne_f = 0, nc = 0, nf = 0;
   HTransferBasis basis = {};
   std::vector<uint64_t> owner;   // [ne_f][2] owner bits of the fine E-vector
   std::vector<int> children;     // [ne_c][8]: the fine element at octant o of parent i
   std::vector<int> c_off, c_idx; // the coarse space's transposed map: row c lists its E-vector entries e D^3 + a, ascending
};

// The two thresholded 1D tables of order p (1..4)
HTransferBasis htransfer_basis(int p);

// Validates both maps and the embedding and builds the plan.  A null map or embedding, a negative size, a map
// entry >= ndofs, a fine dof that no element holds, a parent outside 0..ne_c - 1, an octant outside 0..7: ERR_ARG;
// an order outside 1..4, a negative (signed) entry, a parent that does not have exactly one child per octant
// (non-conforming or partial refinement): ERR_UNSUPPORTED.
HTransferPlan build_htransfer_plan(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f,
                                   const int *parent, const int *octant);

// The device operator.  Vectors are device L-vectors of nc (coarse) and nf (fine) doubles; no alignment beyond a
// double's is asked.  Two calls are bitwise equal.
class HTransfer final : public Transfer
{
public:
   HTransfer(int p, int ne_c, int nc, const int *gather_c, int ne_f, int nf, const int *gather_f, const int *parent,
             const int *octant);
   int ne() const override { return ne_f_; }
   int order_lo() const override { return p_; }
   int order_hi() const override { return p_; }
   int width() const override { return nc_; }
   int height() const override { return nf_; }
   size_t plan_bytes() const override;  // both maps, the owner words, the children table and the transposed map
   void mult(const double *x_c, double *y_f, hipStream_t s) const override;
   void mult_transpose(const double *x_f, double *y_c, hipStream_t s) const override;

private:
   int p_, ne_c_, ne_f_, nc_, nf_;
   HTransferBasis basis_;
   DeviceArray<int> gc_, gf_, children_, c_off_, c_idx_;
   DeviceArray<uint64_t> owner_;
   mutable DeviceArray<double> ye_;  // the restriction's coarse E-vector [ne_c][D^3]
};

namespace kern
{
// y_f[gf[f][i]] = (B_oz (x) B_oy (x) B_ox x_c[gc[parent]])_i where fine element f = children[parent][o] owns dof i
void htransfer_prolong(int p, int ne_c, const int *gc, const int *gf, const int *children, const uint64_t *owner,
                       const HTransferBasis &b, const double *x_c, double *y_f, hipStream_t s);
// ye[parent][a] = sum_o (B_oz^T (x) B_oy^T (x) B_ox^T (mask_f .* x_f[gf[f]]))_a, f = children[parent][o], o ascending
void htransfer_restrict(int p, int ne_c, const int *gf, const int *children, const uint64_t *owner,
                        const HTransferBasis &b, const double *x_f, double *ye, hipStream_t s);
} // namespace kern

} // namespace ecm2
