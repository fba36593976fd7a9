// bdr_term.hpp -- the boundary-face part of a form: what PAForm (boundary MassIntegrator) and
// LinearForm (BoundaryLFIntegrator) share.  It owns the boundary elements' dof map, attributes and
// geometry, the integrators with their attribute markers, the compacted list of faces some
// integrator acts on, and the CSR that adds face vectors into an L-vector.
//
// Reference interface mirrored:
//   PABilinearFormExtension, boundary blocks   fem/bilinearform_ext.cpp:300-328, 354 (setup),
//                                              :625-675 (Mult), :441-452 (AssembleDiagonal),
//                                              :807-847 (AddMultWithMarkers over bdr_face_attributes)
//   MassIntegrator::AssemblePABoundary         fem/integ/bilininteg_mass_pa.cpp:81-125
//   LinearFormExtension::Assemble, boundary    fem/linearform_ext.cpp:70-111
//   BoundaryLFIntegrator::AssembleDevice       fem/integ/lininteg_boundary.cpp:74-153
//
// Markers: integrator i acts on face f when attr[f] > 0 and marker_i[attr[f] - 1] != 0 (all faces
// without a marker).  The weight is folded into the face qdata, as for the domain integrators.  Only
// faces with a non-zero weight in some integrator are kept (the Robin surface is usually a small
// part of the boundary); a term with no such face launches nothing.
#pragma once

#include "common.hpp"
#include "fe.hpp"
#include "kernels.hpp"

#include <vector>

namespace ecm2
{

struct BdrCoeff
{
   int kind = COEFF_CONSTANT;     // COEFF_CONSTANT or COEFF_QUAD
   double value = 1.0;
   const double *quad = nullptr;  // device [nbe][q1d^2], boundary element order
};

class BoundaryTerm
{
public:
   BoundaryTerm(int order, int ndofs) : order_(order), ndofs_(ndofs), D_(order + 1) {}

   bool has_boundary() const { return have_bdr_; }
   int nbe() const { return nbe_; }
   int q1d() const { return Q_; }
   int n_integrators() const { return (int)integs_.size(); }
   int n_active() const { return n_act_; }  // after prepare()

   // bdr_map host [nbe][(p+1)^2], bdr_attr host [nbe], bdr_nodes host [nbe][3][4] (lexicographic
   // corners in the frame of bdr_map; may be null when set_detj supplies the geometry); q1d resolved
   void set_boundary(int nbe, const int *bdr_map, const int *bdr_attr, const double *bdr_nodes, int q1d);
   // FaceGeometricFactors::detJ, device [nbe][q1d^2], not owned; replaces the corners
   void set_detj(const double *detj_device);
   void add_integrator(const BdrCoeff &c, const int *marker, int n_marker);

   // the active faces, the integrators' weights on them and the CSR (cached until an input changes)
   void prepare(hipStream_t s);
   // bilinear form: the summed face qdata of the Mult and of the diagonal (the reference's shared
   // bdr_face_Y rule: integrator j counts on a face only where every marked integrator added at or
   // after j acts, bilinearform_ext.cpp:441-452)
   void assemble_mass(hipStream_t s);
   void add_mult(const double *x, double *y, hipStream_t s);
   void add_diagonal(double *diag, hipStream_t s);
   // pa_data of integrator `index` over all faces, zeros where its marker excludes: host [nbe][q1d^2]
   void get_qdata(int index, double *out_host, hipStream_t s);
   // linear form: b += every integrator's B^T (W c detJ w_f), in the order they were added
   void add_linear(double *b, hipStream_t s);

private:
   struct Integ
   {
      BdrCoeff c;
      bool marked = false;
      std::vector<int> marker;
      DeviceArray<double> w, wdiag;  // device [n_act]: the Mult's / the diagonal's weights
   };
   std::vector<double> face_weights(const Integ &g) const;  // host [nbe]
   kern::BdrSetupArgs setup_args(const Integ &g, const double *wf, double *qd, bool accumulate) const;

   int order_, ndofs_, D_, Q_ = 0, nbe_ = 0, n_act_ = 0;
   bool have_bdr_ = false, prepared_ = false;
   std::vector<int> bmap_host_, attr_;
   DeviceArray<int> bmap_;
   DeviceArray<double> nodes_;
   const double *detj_ = nullptr;
   DofToQuad maps_;
   Basis1D basis_ = {};
   DeviceArray<double> Bdev_, wq_, qpts_;
   std::vector<Integ> integs_;
   DeviceArray<int> faces_;                        // [n_act] boundary element indices, ascending
   DeviceArray<int> csr_dof_, csr_off_, csr_idx_;  // rows: the dofs of the active faces
   int n_rows_ = 0;
   DeviceArray<double> qd_, qd_diag_, yf_;         // [n_act][q1d^2] (x2), [n_act][d1d^2]
   bool diag_differs_ = false;
};

} // namespace ecm2
