// linear_form.hpp -- MI355X device linear form: the drop-in for the reference's
// LinearForm + DomainLFIntegrator(Q) on the device path, the right-hand side of the bioheat
// problem (the RF Joule heat sigma(T) |grad phi|^2 and the perfusion sink's w c_b T_a).
//
// Reference interface mirrored:
//   LinearFormExtension::Assemble            fem/linearform_ext.cpp:20-68
//   DomainLFIntegrator::AssembleDevice       fem/integ/lininteg_domain.cpp:22-59
//   DLFEvalAssemble3D                        fem/integ/lininteg_domain_kernels.hpp:164-300
//   ElementRestriction::MultTranspose        fem/restriction.cpp:146-186
// Ownership follows PAForm: the form owns its maps, geometry and E-vector scratch; the
// coefficients' device arrays and b are caller-owned; all work is enqueued on the caller's stream.
#pragma once

#include "bdr_term.hpp"
#include "common.hpp"
#include "fe.hpp"
#include "kernels.hpp"

#include <vector>

namespace ecm2
{

// A DomainLFIntegrator's source (kernels.hpp LFormArgs): the scalar kinds of CoeffDesc plus
// COEFF_JOULE (lvec = phi, lvec2 = T or null, sigma = scale (1 + slope (T - t_ref))).
struct SourceDesc
{
   int kind = COEFF_CONSTANT;
   double value = 0.0;
   const double *quad = nullptr, *lvec = nullptr, *lvec2 = nullptr;
   double scale = 1.0, slope = 0.0, t_ref = 0.0;
};

class LinearForm
{
public:
   // DomainLFIntegrator(Q, a = 2, b = 0): the rule of order a p + b (lininteg.hpp:116), p + 1
   // Gauss-Legendre points per direction (intrules.cpp:1181-1200)
   static int default_q1d(int order) { return order + 1; }

   LinearForm(int ne, int order, int ndofs, const int *gather_map_host, int q1d = 0);

   int ne() const { return ne_; }
   int ndofs() const { return ndofs_; }
   int d1d() const { return D_; }
   int q1d() const { return Q_; }
   int n_integrators() const { return (int)integs_.size(); }
   int n_boundary_integrators() const { return bdr_.n_integrators(); }
   // BoundaryLFIntegrator(Q, a = 1, b = 1): the rule of order a p + b (lininteg.hpp:200),
   // (p + 1) / 2 + 1 Gauss-Legendre points per direction (2, 2, 3, 3 for p = 1..4)
   static int default_bdr_q1d(int order) { return (order + 1) / 2 + 1; }

   // Geometry: lexicographic corners (host [ne][3][8]) or MFEM-layout Jacobians (device,
   // NQ x 3 x 3 x NE, valid for as long as the form is assembled); the last call wins.
   void set_element_nodes(const double *enodes_host);
   void set_jacobians(const double *J_device);
   // element attributes (host [ne]) for marked integrators
   void set_attributes(const int *attr_host);
   // LinearForm::AddDomainIntegrator(lfi[, elem_marker]) (linearform.cpp): marker host [n_marker],
   // 0 / 1 per attribute, null = all elements
   void add_domain_integrator(const SourceDesc &c, const int *marker = nullptr, int n_marker = 0);
   // Boundary integrators (LinearForm::AddBoundaryIntegrator(new BoundaryLFIntegrator(g), bdr_marker);
   // LinearFormExtension::Assemble's boundary loop, linearform_ext.cpp:70-111; BLFEvalAssemble3D,
   // lininteg_boundary.cpp:74-153): set_boundary takes PAForm::set_boundary's arguments, q1d <= 0
   // selects default_bdr_q1d, and that, p + 1 and p + 2 points are supported.  The coefficient is a
   // constant or per-point values (device [nbe][q1d^2], read at every assemble).
   void set_boundary(int nbe, const int *bdr_map_host, const int *bdr_attr_host, const double *bdr_nodes_host, int q1d);
   void set_boundary_detj(const double *detj_device);
   void add_boundary_integrator(const SourceDesc &c, const int *marker = nullptr, int n_marker = 0);
   // b = sum over the integrators, in the order they were added: each one's element vectors, then
   // the CSR transpose -- the first stores, the later ones add (linearform_ext.cpp:64-67).  The
   // coefficients' device arrays are read here, every time.  The boundary integrators follow the domain
   // ones, each added through the boundary dofs' CSR in ascending face order (no atomics).
   void assemble(double *b, hipStream_t s);

private:
   struct Integ
   {
      SourceDesc c;
      bool marked = false;
      std::vector<int> marker;
      DeviceArray<int> emark;  // device [ne] 0 / 1 (marked only), built at assemble
      bool emark_valid = false;
   };
   void ensure_csr();

   int ne_, order_, ndofs_, D_, Q_, ND_, NQ_;
   BoundaryTerm bdr_;
   DofToQuad maps_;
   Basis1D basis_;
   QPts qp_ = {};
   std::vector<int> gmap_host_, attr_;
   DeviceArray<int> gmap_, csr_off_, csr_idx_;
   DeviceArray<double> W_, enodes_;
   const double *jac_ = nullptr;  // device, not owned
   std::vector<Integ> integs_;
   DeviceArray<double> be_, bwork_;  // E-vector scratch [ne][nd]; the later integrators' R^T be [ndofs]
};

} // namespace ecm2
