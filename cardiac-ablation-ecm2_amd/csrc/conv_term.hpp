// conv_term.hpp -- the convection part of a form: what PAForm owns beside its boundary term for
// a.AddDomainIntegrator(new ConvectionIntegrator(vel, alpha)[, elem_marker]) at AssemblyLevel::PARTIAL
// (the blood-flow advection rho_b c_b u . grad T of the bioheat operator).
//
// Reference interface mirrored:
//   ConvectionIntegrator::AssemblePA           fem/integ/bilininteg_convection_pa.cpp:174-214
//   PAConvectionSetup3D                        bilininteg_convection_pa.cpp:100-152
//   AddMultPA / AddMultTransposePA             bilininteg_convection_pa.cpp (ApplyPAKernels / ApplyPATKernels),
//                                              kernels bilininteg_convection_kernels.hpp:274-451, 897-
//   AssembleDiagonalPA                         bilininteg_convection_pa.cpp:216-227 (aborts)
//   ConvectionIntegrator::GetRule              fem/bilininteg.cpp:1610-1623 (order 2p + 2 on a trilinear
//                                              hex, fem/eltrans.cpp:477-523: p + 2 points per direction)
//   AddMultWithMarkers                         fem/bilinearform_ext.cpp:753-774
//
// Markers: the term acts on element e when attr[e] > 0 and marker[attr[e] - 1] != 0 (all elements
// without a marker).  Only those active elements are stored and launched (the blood pool is usually a
// small part of the mesh), ascending in element index, as BoundaryTerm keeps its active faces; a term
// with no active element launches nothing.  The qdata is built at assemble() from the live
// coefficient array (assemble-time semantics: a later change of the velocity shows after the next
// assemble()).  A Mult is two launches: the apply into an E-vector over the active elements, then a
// fixed-order add (a thread per touched dof): no atomics, no memset, two Mults are bitwise equal.
#pragma once

#include "common.hpp"
#include "conv_plan.hpp"
#include "fe.hpp"
#include "kernels.hpp"

#include <vector>

namespace ecm2
{

// the form's geometry and rule, handed over at assemble()
struct ConvGeometry
{
   const double *enodes = nullptr;  // device [ne][3][8], or
   const double *J = nullptr;       // device, MFEM layout NQ x 3 x 3 x NE
   const double *W = nullptr;       // device tensor weights [nq]
   QPts qp = {};
};

class ConvectionTerm
{
public:
   ConvectionTerm(int ne, int order, int q1d, int ndofs)
      : ne_(ne), ndofs_(ndofs), D_(order + 1), Q_(q1d), ND_(D_ * D_ * D_), NQ_(q1d * q1d * q1d)
   {
   }

   bool present() const { return present_; }
   int n_active() const { return plan_n_act_; }  // after assemble()
   bool blocked() const { return kern::conv_blocked(D_); }

   // c: COEFF_CONST_VECTOR (cv[0..2]) or COEFF_QUAD_VECTOR (device [ne][nq][3]); anything else ERR_ARG
   void set(const CoeffDesc &c, double alpha, const int *marker, int n_marker);
   // the active list, maps and CSR from the gather map and the attributes (a marked term needs
   // them), then the qdata
   void assemble(const std::vector<int> &gmap_host, const std::vector<int> &attr, const ConvGeometry &g,
                 const Basis1D &basis, hipStream_t s);
   // y += C x (transpose: C^T x) on L-vectors
   void add_mult(const double *x, double *y, bool transpose, hipStream_t s);
   // AddMultPA / AddMultTransposePA on E-vectors [ne][nd] (all elements, caller order)
   void add_mult_evec(const double *xe, double *ye, bool transpose, hipStream_t s);
   // pa_data in the reference's layout, host [ne][3][nq]; zeros on excluded elements
   void get_qdata(double *out_host, hipStream_t s);

private:
   std::vector<unsigned char> keep(const std::vector<int> &attr) const;
   kern::ConvSetupArgs setup_args(const ConvGeometry &g, int n, const int *act, bool blocked, double *qd) const;

   int ne_, ndofs_, D_, Q_, ND_, NQ_;
   bool present_ = false, marked_ = false;
   CoeffDesc c_;
   double alpha_ = 1.0;
   std::vector<int> marker_;
   Basis1D basis_ = {};
   // the last assemble()'s plan on the device
   int plan_n_act_ = 0, n_rows_ = 0;
   std::vector<int> act_host_;
   DeviceArray<int> act_, map_;                     // [n_act], the gather rows in the kernel's layout
   DeviceArray<int> csr_dof_, csr_off_, csr_idx_;  // rows: the dofs of the active elements
   DeviceArray<double> qd_, ye_;                    // qdata and the E-vector scratch (active elements)
   // the E-vector entry points: identity rows of the active elements and their add rows (built on
   // first use after an assemble())
   DeviceArray<int> emap_, ecsr_dof_, ecsr_off_, ecsr_idx_;
   int e_rows_ = 0;
   bool evec_ready_ = false;
};

} // namespace ecm2
