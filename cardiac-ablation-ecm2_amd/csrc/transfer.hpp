// transfer.hpp -- the p-refinement transfer operator between two H1 spaces of orders pc < pf on the same
// elements, and the host-side construction of its plan.
//
// Reference:
//   TensorProductPRefinementTransferOperator   fem/transfer.cpp:2223-2287 (constructor)
//   TransferKernels::Prolongation3D            fem/transfer.cpp:2338-2423
//   TransferKernels::Restriction3D             fem/transfer.cpp:2470-2539
//   Mult / MultTranspose                       fem/transfer.cpp:2542-2592
//   ElementRestriction::BooleanMask            fem/restriction.cpp:248-283
//
// Each space is given by its gather map [ne][(p + 1)^3] (lexicographic local dofs, x fastest, the caller's
// element order, as ecm2_pa_form_create takes it); nothing else about the spaces is read, so any pair of
// numberings, any element order and any geometry is admitted.
//   Mult (prolongation):  y_f = R_f^T mask (B (x) B (x) B) R_c x_c.  mask (BooleanMask) is 1 at an L-dof's first
//     occurrence in the fine E-vector -- in the lowest-numbered element that holds it -- and 0 elsewhere, so every
//     fine dof is written once, by its owner: y is overwritten, no zero fill, no atomics.
//   MultTranspose (restriction):  y_c = R_c^T (B^T (x) B^T (x) B^T) mask R_f x_f, the sum over the elements that
//     share a coarse dof in ascending E-vector order through the coarse space's transposed map (a CSR): no
//     atomics, y overwritten.
// B[q + Df d] (Df = pf + 1): the coarse GLL Lagrange basis function d at the fine GLL node q (fe.cpp's
// gauss_lobatto and basis_eval, as the reference's DofToQuad of the coarse element at the fine element's nodes).
// The mask is not stored as ne Df^3 doubles: the plan holds owner bits, two 64-bit words per element (Df^3 <= 125),
// bit i of word i / 64 for local fine dof i.
#pragma once

#include "common.hpp"

#include <cstdint>
#include <vector>

namespace ecm2
{

constexpr int kTransferMaxOrder = 4;                                  // kernels exist for 1 <= pc < pf <= 4
constexpr int kTransferMaxDc = kTransferMaxOrder, kTransferMaxDf = kTransferMaxOrder + 1;

// Kernel-argument copy of the 1D table (read with scalar loads where the index is a constant)
struct TransferBasis
{
   double B[kTransferMaxDf * kTransferMaxDc];  // [q + Df d]
};

// What the host builds (plain C++; tests/cpp/transfer_plan_check.cpp replays it on the CPU)
struct TransferPlan
{
   int ne = 0, pc = 0, pf = 0, nc = 0, nf = 0;
   TransferBasis basis = {};
   std::vector<uint64_t> owner;   // [ne][2] owner bits of the fine E-vector
   std::vector<int> c_off, c_idx; // the coarse space's transposed map: row c lists its E-vector entries e Dc^3 + a, ascending
};

// Validates both maps and builds the plan.  pc >= pf, ne < 0, a null map: ERR_ARG; an order outside 1..4:
// ERR_UNSUPPORTED; an entry >= ndofs: ERR_ARG; a negative (signed) entry: ERR_UNSUPPORTED (H1 has none); a fine
// dof that no element holds (it would never be written): ERR_ARG.
TransferPlan build_transfer_plan(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f);

// What the multigrid cycle and the C handle hold: a transfer between a coarse and a fine space, whichever kind
// (PTransfer below: two orders on one mesh; HTransfer, htransfer.hpp: one order on a mesh and its refinement).
class Transfer
{
public:
   virtual ~Transfer() = default;
   virtual int ne() const = 0;        // elements of the fine space
   virtual int order_lo() const = 0;
   virtual int order_hi() const = 0;
   virtual int width() const = 0;     // the coarse space's size (Operator::Width)
   virtual int height() const = 0;    // the fine space's size (Operator::Height)
   virtual size_t plan_bytes() const = 0;
   virtual void mult(const double *x_c, double *y_f, hipStream_t s) const = 0;
   virtual void mult_transpose(const double *x_f, double *y_c, hipStream_t s) const = 0;
};

// The device operator.  Vectors are device L-vectors of nc (coarse) and nf (fine) doubles; the kernels read and
// write single entries through the maps, so no alignment beyond a double's is asked.  Two calls are bitwise equal.
class PTransfer final : public Transfer
{
public:
   PTransfer(int ne, int pc, int nc, const int *gather_c, int pf, int nf, const int *gather_f);
   int ne() const override { return ne_; }
   int order_lo() const override { return pc_; }
   int order_hi() const override { return pf_; }
   int width() const override { return nc_; }
   int height() const override { return nf_; }
   size_t plan_bytes() const override;  // both maps, the owner words and the transposed map on the device
   void mult(const double *x_c, double *y_f, hipStream_t s) const override;
   void mult_transpose(const double *x_f, double *y_c, hipStream_t s) const override;

private:
   int ne_, pc_, pf_, nc_, nf_;
   TransferBasis basis_;
   DeviceArray<int> gc_, gf_, c_off_, c_idx_;
   DeviceArray<uint64_t> owner_;
   mutable DeviceArray<double> ye_;  // the restriction's coarse E-vector [ne][Dc^3]
};

namespace kern
{
// y_f[gf[e][i]] = (B (x) B (x) B x_c[gc[e]])_i where element e owns local fine dof i
void transfer_prolong(int pc, int pf, int ne, const int *gc, const int *gf, const uint64_t *owner, const TransferBasis &b,
                      const double *x_c, double *y_f, hipStream_t s);
// ye[e][a] = (B^T (x) B^T (x) B^T (mask_e .* x_f[gf[e]]))_a
void transfer_restrict(int pc, int pf, int ne, const int *gf, const uint64_t *owner, const TransferBasis &b,
                       const double *x_f, double *ye, hipStream_t s);
} // namespace kern

} // namespace ecm2
