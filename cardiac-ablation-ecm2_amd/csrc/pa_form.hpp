// pa_form.hpp -- MI355X PA form: the drop-in for the reference's
// BilinearForm(PARTIAL) + {MassIntegrator(alpha), DiffusionIntegrator(beta)[, ConvectionIntegrator(v, a)]}
// and its PABilinearFormExtension.
//
// Reference interface mirrored:
//   PABilinearFormExtension::Assemble / Mult / AssembleDiagonal
//                                          fem/bilinearform_ext.hpp:67-144, .cpp:332-564
//   BilinearFormIntegrator::AssemblePA / AddMultPA / AssembleDiagonalPA
//                                          fem/bilininteg.hpp:49-97
//   ElementRestriction::Mult / MultTranspose fem/restriction.cpp:109-186
// Ownership follows the reference: the form owns qdata and its work vectors;
// x / y are caller-owned device arrays; all work is enqueued on the caller's
// stream (the reference uses the null stream, forall.hpp:782).
//
// The fused kernels' scatter planning (element order, merge flags, dof maps, lattice blocks and
// bricks, partial slots, the summation plan) is host-only code in scatter_plan.hpp.  The form owns
// what those functions return as three plan objects (plan_dev.hpp): tpe_ (p <= 2), line_ (p >= 3)
// and shared_ (the summation pass of whichever is in use); a setter that feeds a plan's builder
// invalidates it (invalidate_plans), Assemble rebuilds what is not valid.  A launch takes two kinds
// of arguments (kernels.hpp): TpeArgs / LineArgs, built once at the end of Assemble from the plan
// and the snapshot, and ApplyArgs, filled per call (vectors, block range, the qdata to read).
#pragma once

#include "bdr_term.hpp"
#include "common.hpp"
#include "conv_term.hpp"
#include "fe.hpp"
#include "kernels.hpp"
#include "plan_dev.hpp"

#include <memory>
#include <utility>
#include <vector>

namespace ecm2
{

enum KernelMode : int
{
   KERNEL_AUTO = 0,     // TPE for p = 1, 2; LINE for p = 3..6; else WPE
   KERNEL_TPE = 1,      // fused, thread per element (p = 1, 2)
   KERNEL_WPE = 2,      // fused, workgroup per element, all intermediates in LDS (any p)
   KERNEL_UNFUSED = 3,  // reference-shaped: restriction, per-integrator AddMultPA, CSR transpose
   KERNEL_LINE = 4      // fused, one wave per element, register lines (Q1D <= 8)
};

// How the fused TPE kernel combines contributions to dofs held by more than one element
// entry (after in-wave face assembly):
enum ScatterMode : int
{
   SCATTER_PARTIALS = 0,  // dense partial slots + a fixed-order summation pass (deterministic)
   SCATTER_ATOMIC = 1     // FP64 atomic adds into a zeroed y
};

enum IntegratorKind : int { INTEG_MASS = 0, INTEG_DIFFUSION = 1, INTEG_CONVECTION = 2 };

// The CSR transpose of a gather map [ne][nd] (ElementRestriction's offsets / indices,
// restriction.cpp:68-106; index -1 - lid = minus sign) that kern::restriction_mult_transpose sums:
// shared by PAForm and LinearForm.
void build_restriction_csr(const std::vector<int> &gmap, int ndofs, std::vector<int> &off, std::vector<int> &idx);

class PAForm
{
public:
   // n_owned < ndofs: the local L-vector is split [owned | ghost] (distributed form);
   // x/y hold dofs < n_owned, xg/yg the ghosts (apply_blocks).
   PAForm(int ne, int order, int ndofs, const int *gather_map_host, int q1d = 0, int n_owned = -1);
   ~PAForm();

   int ne() const { return ne_; }
   int order() const { return order_; }
   int ndofs() const { return ndofs_; }
   int d1d() const { return D_; }
   int q1d() const { return Q_; }
   int layout() const { return layout_.kind; }
   int kernel_mode() const { return resolved_mode_; }

   // Geometry: lexicographic corner coordinates (host, [ne][3][8]) or
   // MFEM-layout Jacobians (device, NQ x 3 x 3 x NE; the pointer must stay
   // valid until assemble()).
   void set_element_nodes(const double *enodes_host);
   void set_jacobians(const double *J_device);
   // AFFINE qdata (kernels.hpp) for the fused p <= 2 kernel when every element is a
   // parallelepiped (checked on the corners) and both integrators are present: on by default.
   void set_geometry_compression(bool on);
   bool affine_geometry() const { return affine_; }
   // Coefficient snapshot (AFFINE, p = 2, lattice blocks, the diffusion coefficient an affine law
   // of an H1 field, unmarked): the law applied to the field's dofs at Assemble and interpolated by
   // the kernel, instead of a stored W beta per point.  On by default; coefficient_snapshot() says
   // whether the last Assemble took it.
   void set_coefficient_snapshot(bool on);
   bool coefficient_snapshot() const { return layout_.tsnap != 0; }
   // with the snapshot: the mass values (QLayout::tmass) and where the laws are applied (QLayout::tlaw)
   int snapshot_mass() const { return layout_.tmass; }
   int snapshot_law_at_point() const { return layout_.tlaw; }
   bool flux_diagonal() const { return cdiag_ && (layout_.tsnap || layout_.kind == QLAYOUT_AFFINE_E); }
   // bytes of quadrature data the form stores (diffusion + mass + the coefficient snapshot)
   size_t qdata_bytes() const { return qd_diff_.bytes() + qd_mass_.bytes() + tsnap_.bytes(); }

   // Optional element permutation (internal position i <- caller element perm[i]) used by
   // the blocked layout; ORDER_BRICK puts one 4x4x4 brick in each 64-lane wave so the
   // fused kernel can assemble shared faces in-wave.  Without one, assemble() derives a
   // brick order from the element->dof map (face_brick_order, any conforming mesh).  All
   // APIs keep caller element order.
   void set_element_order(const int *perm_host);
   // Block indices at which apply_blocks ranges may start or end besides 0 and nblocks()
   // (the distributed form's interior | boundary split).  The line kernel's bricks never
   // straddle one.
   void set_block_splits(const std::vector<int> &splits);
   // Bricks of the line kernel family (p >= 3, both integrators, partial scatter): -1 =
   // default (2 x 2 x 1), 0 = none, 1 = 2 x 2 x 1, 2 = 2 x 2 x 2 elements per workgroup.
   void set_line_bricks(int bz);
   // Blocks >= b are applied with the one-block-per-workgroup latency kernel (apply_blocks
   // latency = true): no cross-wave face assembly there.  -1: none.
   void set_latency_from(int b);
   int n_bricks() const { return line_.info.n_bricks; }
   // units (p <= 2 blocks, p >= 3 bricks) whose dofs the fused kernel computes from 5 ints
   // instead of reading the map
   int lattice_units() const
   {
      if (resolved_mode_ == KERNEL_TPE)
      {
         return (layout_.kind == QLAYOUT_AFFINE || layout_.kind == QLAYOUT_TRILINEAR) ? tpe_.info.n_treg : 0;
      }
      return (resolved_mode_ == KERNEL_LINE && line_.breg.size()) ? n_bricks() : 0;
   }
   int n_units() const { return resolved_mode_ == KERNEL_TPE ? layout_.nblk() : n_bricks(); }
   // p <= 2 blocks with face-grouped partial slots but map-addressed dofs (a numbering that is not a lattice)
   int lattice_slot_units() const { return resolved_mode_ == KERNEL_TPE ? tpe_.info.n_tlat : 0; }
   int brick_bz() const { return line_.info.brick_bz; }
   // BilinearForm::AddDomainIntegrator(integ[, elem_marker]) (bilinearform.cpp:231-242): with a
   // marker (host marker[n_marker], 0 / 1 per attribute), the integrator acts on the elements
   // whose attribute a has a > 0 and marker[a - 1] != 0 only (AddMultWithMarkers,
   // bilinearform_ext.cpp:753-774,807-847); the attributes come from set_attributes.
   void add_integrator(int kind, const CoeffDesc &c, const int *marker = nullptr, int n_marker = 0);
   // BilinearForm::AddDomainIntegrator(new ConvectionIntegrator(vel, alpha)[, elem_marker]) (conv_term.hpp):
   // c a velocity (COEFF_CONST_VECTOR / COEFF_QUAD_VECTOR, anything else ERR_ARG); at most one per form; the
   // form's rule must be p + 1 or p + 2 points with p = 1..4 (ConvectionIntegrator's specialisations,
   // bilininteg_convection_pa.cpp:30-58; its GetRule is the form's default p + 2), else ERR_UNSUPPORTED; a
   // distributed local form (n_owned < ndofs) refuses it.  Mult then adds C x after the volume part and the
   // boundary term, mult_transpose C^T x; the diagonal is refused as the reference's AssembleDiagonalPA aborts
   // (bilininteg_convection_pa.cpp:216-227) and the Mult's energy is not folded (energy_parts() = 0).
   void add_convection(const CoeffDesc &c, double alpha, const int *marker = nullptr, int n_marker = 0);
   bool has_convection() const { return conv_.present(); }
   // (present, active elements of the last Assemble, MultTranspose differs from Mult)
   void convection_info(int *present, int *n_active, int *transpose_distinct) const;
   // element attributes (host [ne], caller element order), as Mesh::GetAttribute
   void set_attributes(const int *attr_host);
   // Boundary integrators (BilinearForm::AddBoundaryIntegrator(new MassIntegrator(h), bdr_marker):
   // the Robin term; PABilinearFormExtension's boundary blocks, bilinearform_ext.cpp:300-328, 441-452,
   // 625-675; MassIntegrator::AssemblePABoundary, bilininteg_mass_pa.cpp:81-125).  set_boundary: the
   // boundary elements' dofs (host [nbe][(p+1)^2]), attributes (host [nbe]) and lexicographic corners
   // (host [nbe][3][4], the frame of the dof rows); q1d <= 0 selects MassIntegrator::GetRule's p + 1
   // points (order 2p + 1 on a bilinear quad), p + 1 and p + 2 are supported.  A distributed local
   // form (n_owned < ndofs) has no boundary terms.  set_boundary_detj: FaceGeometricFactors::detJ
   // (device [nbe][q1d^2], valid until assemble()) instead of the corners.  All boundary integrators
   // share the rule; their qdata are summed at assemble() and one face apply, run after the volume
   // result is complete, serves Mult in every kernel mode.
   void set_boundary(int nbe, const int *bdr_map_host, const int *bdr_attr_host, const double *bdr_nodes_host, int q1d);
   void set_boundary_detj(const double *detj_device);
   void add_boundary_integrator(int kind, const CoeffDesc &c, const int *marker = nullptr, int n_marker = 0);
   // pa_data of boundary integrator `index` (host [nbe][q1d^2]; zeros on faces its marker excludes)
   void get_boundary_qdata(int index, double *out_host, hipStream_t s);
   void boundary_info(int *nbe, int *n_integrators, int *n_active, int *q1d) const;
   bool has_boundary_integrators() const { return bdr_.n_integrators() > 0; }
   void set_kernel(int mode);
   void set_scatter(int mode);
   int scatter() const { return scatter_; }
   bool use_partials() const
   {
      return (resolved_mode_ == KERNEL_TPE || resolved_mode_ == KERNEL_LINE) && scatter_ == SCATTER_PARTIALS;
   }
   void assemble(hipStream_t s);

   // y = A x (BilinearForm::Mult semantics: y overwritten).
   void mult(const double *x, double *y, hipStream_t s);
   // y = A^T x (PABilinearFormExtension::MultTranspose, bilinearform_ext.cpp:679-): the symmetric volume and
   // boundary parts as Mult, then C^T x of a convection integrator
   void mult_transpose(const double *x, double *y, hipStream_t s);
   // y += a A x (Operator::AddMult, linalg/operator.hpp:87-92): Mult into a form-owned work
   // vector, then one axpy.  Like every call on a form (the reference's Mult reuses its
   // localX / localY too, bilinearform_ext.hpp:75), AddMult is stream-serial per form: two calls
   // on the same form must be ordered (same stream or an event), not run concurrently.
   void add_mult(const double *x, double *y, double a, hipStream_t s);
   // The Mult with its energy x^T A x folded in (CGSolver's den = (A d, d), solvers.cpp:993, without
   // a dot pass over the vectors): energy_parts() partials (one per workgroup of the single apply
   // launch, summed in a fixed order by the caller) -- or 0 when this form's kernel does not fold it
   // (only the coefficient-snapshot kernel k_apply_tpe_ts does, and not for a form with a boundary
   // integrator, whose face term the folded sum would miss; the caller then runs the dot).
   int energy_parts() const;
   void mult_energy(const double *x, double *y, double *en, hipStream_t s);
   bool assembled() const { return assembled_; }
   // Incremented by every assemble(): whoever caches device pointers or launches of this form
   // (the distributed form's HIP graphs) rebuilds them when it changes.
   long generation() const { return gen_; }
   // Fused apply of element blocks [b0, b1) (64 elements per block); x / xg as in the
   // constructor's split.  Atomic scatter: accumulates into zero-initialised y / yg.
   // Partial scatter: stores the dofs held once, writes the shared ones' partial slots;
   // finish_shared over the shared-dof range [i0, i1) then stores those (the owned
   // shared dofs are [0, n_shared_owned()), the ghost ones [n_shared_owned(), n_shared())).
   // latency: small block range on a critical path (the p <= 2 AFFINE kernel then gives each
   // block a workgroup with one quadrature plane per wave).
   void apply_blocks(const double *x, const double *xg, double *y, double *yg, int b0, int b1,
                     hipStream_t s, bool latency = false, double *en = nullptr);
   void finish_shared(int i0, int i1, double *y, double *yg, hipStream_t s) const;
   int n_shared() const { return shared_.info.n_sh; }
   int n_shared_owned() const { return shared_.info.n_sh_owned; }
   long n_partial_slots() const { return shared_.info.n_slots; }
   long n_summation_runs() const { return shared_.info.n_runs; }
   long n_explicit_runs() const { return shared_.info.n_explicit_runs; }
   int nblocks() const { return layout_.nblk(); }
   bool has_mass() const { return have_mass_; }
   bool has_diffusion() const { return have_diff_; }
   void assemble_diagonal(double *diag, hipStream_t s);  // cached per assembly (gen_)

   // Reference-shaped pieces (E-vector layout [e][nd], lexicographic).
   void restriction_mult(const double *x, double *xe, hipStream_t s);
   void restriction_mult_transpose(const double *xe, double *y, hipStream_t s);
   // (transpose: AddMultTransposePA -- the plain apply for the symmetric mass and diffusion)
   void integrator_add_mult(int kind, const double *xe, double *ye, hipStream_t s, bool transpose = false);
   // qdata in the reference's native layout, copied to the host.
   void get_qdata(int kind, double *out_host, hipStream_t s);

   // HIP-event timing of the dominant (apply) kernel; record_start / record_stop bracket one
   // (the distributed form brackets its own apply_blocks calls).
   void timing_enable(bool on);
   bool timing_on() const { return timing_; }
   void timing_get(double *total_ms, long *launches);
   void record_start(hipStream_t s);
   void record_stop(hipStream_t s);
   size_t algorithmic_bytes() const;

private:
   // stored qdata to read: the form's own, or a caller's scaled copy (the marker diagonal)
   struct QData
   {
      const double *diff, *mass;
   };
   QData qdata() const { return {qd_diff_.data(), qd_mass_.data()}; }
   void ensure_csr();
   void ensure_work(hipStream_t s);
   // the volume part of Mult (y overwritten); mult adds the boundary term after it
   void mult_volume(const double *x, double *y, hipStream_t s);
   // a setter that feeds build_tpe_plan / build_line_plan drops that plan: Assemble rebuilds it
   void invalidate_plans(bool tpe, bool line);
   // assemble()'s steps, in order: kernel mode and qdata layout; the fused kernel's scatter plan
   // (built by scatter_plan.hpp's host functions unless the cached one still holds, then uploaded);
   // the coefficient snapshot; setup_qdata; the marker diagonal's weights
   void resolve_layout(hipStream_t s);
   void plan_tpe(hipStream_t s);
   void plan_line(hipStream_t s);
   void choose_snapshot(hipStream_t s);
   void setup_marker_diagonal(hipStream_t s);
   // the launch arguments fixed by an assembly (targs_ / largs_), and one call's
   void build_launch_args();
   ApplyArgs apply_args(const double *x, const double *xg, double *y, double *yg, int b0, int b1, QData q) const;
   // qdata of the integrators present (resized, padding cleared, coefficients projected, setup
   // kernel)
   void setup_qdata(hipStream_t s);
   // element weights [ne] of integrator kind k: 1 / 0 per its attribute marker, all 1 unmarked
   std::vector<double> marker_weights(int k) const;
   void diagonal_from_qdata(double *diag, QData q, hipStream_t s) const;
   void assemble_diagonal_uncached(double *diag, hipStream_t s) const;
   // TRILINEAR(_E) forms and diffusion-only AFFINE(_E) forms: their per-point qdata in the BLOCKED
   // (p <= 2) or NATIVE (p >= 3) layout, expand_kind() (temporaries of the caller) for the
   // diagonal, the E-vector apply and the qdata export
   bool expand_needed() const
   {
      return layout_.trilinear() || layout_.tsnap || (layout_.affine() && layout_.pw == 1);
   }
   // coefficient values at the quadrature points ([e][q], tmp holds computed ones)
   const double *coeff_points(const CoeffDesc &c, DeviceArray<double> &tmp, hipStream_t s) const;
   int expand_kind() const { return layout_.blocked() ? QLAYOUT_BLOCKED : QLAYOUT_NATIVE; }
   // (q: the stored compressed qdata to expand)
   void expand_compressed(QData q, DeviceArray<double> &fd, DeviceArray<double> &fm, hipStream_t s) const;

   int ne_, order_, ndofs_, n_owned_, D_, Q_, ND_, NQ_;
   BoundaryTerm bdr_;               // boundary integrators (empty unless set_boundary was called)
   ConvectionTerm conv_;            // the convection integrator (empty unless add_convection was called)
   DofToQuad maps_;
   QPts qp_ = {};                   // maps_.qpts as a kernel argument
   Basis1D basis_, basis1_;
   QLayout layout_;
   int mode_ = KERNEL_AUTO, resolved_mode_ = KERNEL_AUTO;
   int scatter_ = SCATTER_PARTIALS;
   // the fused kernels' scatter plans (plan_dev.hpp) and the launch arguments of the last Assemble
   TpePlanDev tpe_;
   LinePlanDev line_;
   SharedPlanDev shared_;
   TpeArgs targs_;
   LineArgs largs_;
   // partial slots: TPE [blk][part_stride]; LINE [bricks | [e][nd]] (scratch every apply and diagonal writes)
   mutable DeviceArray<double> part_;
   bool assembled_ = false;
   DeviceArray<double> diag_cache_;  // the diagonal of assembly diag_gen_ (assemble_diagonal)
   long diag_gen_ = -1;
   long gen_ = 0;
   DeviceArray<double> ywork_;      // add_mult
   bool have_mass_ = false, have_diff_ = false;
   CoeffDesc cmass_, cdiff_;
   std::vector<int> attr_;               // element attributes (set_attributes)
   std::vector<int> marker_[2];          // per integrator kind: attribute marker (empty: none)
   bool marked_[2] = {false, false};
   std::vector<int> order_added_;        // integrator kinds in AddDomainIntegrator order (the diagonal's markers)
   DeviceArray<double> emask_[2];        // per integrator kind: element weights [ne] (marked only)
   int diag_integ_ = -1;                 // the marker diagonal: integrator whose qdata diag_w_ scales (-1: none)
   DeviceArray<double> diag_w_;          // its element weights [ne] (the second integrator's marker, at Assemble)

   std::vector<int> gmap_host_;
   DeviceArray<int> gmap_;          // native [e][nd]
   std::vector<int> splits_;        // apply_blocks range boundaries besides 0 / nblk
   std::vector<int> user_perm_;     // set_element_order's (empty: none, the TPE plan derives one)
   bool cdiag_ = false;             // snapshot forms: every element's C diagonal (axis-aligned: the diagonal flux)
   DeviceArray<int> cdflag_;        // its test's device scratch
   int line_bricks_ = -1;           // requested brick mode (set_line_bricks)
   bool affine_ = false;            // every element a parallelepiped (set_element_nodes)
   bool compress_ = true;           // set_geometry_compression
   bool tsnap_pref_ = true;         // set_coefficient_snapshot
   DeviceArray<double> tsnap_;      // coefficient snapshot T' = A + B T (local L-vector)
   int latency_from_ = -1;          // set_latency_from
   DeviceArray<int> csr_off_, csr_idx_;
   DeviceArray<double> enodes_;     // [e][3][8]
   DeviceArray<double> cfit_;       // TRILINEAR from Jacobians: fitted map coefficients [e][21]
   const double *jac_ = nullptr;    // device, not owned
   DeviceArray<double> W_, rowtab_, drowtab_;
   DeviceArray<BasisDev> btab_;     // device copy of basis_ + its even/odd split (line / brick / diagonal / coefficient kernels)
   const Basis1D *btab() const { return btab_.size() ? &btab_.data()->b : nullptr; }
   DeviceArray<double> qd_diff_, qd_mass_;
   DeviceArray<double> xe_, ye_;    // unfused work E-vectors
   DeviceArray<double> ctmp_m_, ctmp_d_;

   bool timing_ = false;
   std::vector<hipEvent_t> ev_start_, ev_stop_;
   size_t ev_count_ = 0;
};

} // namespace ecm2
