// linear_form.cpp -- see linear_form.hpp.
#include "linear_form.hpp"
#include "pa_form.hpp"

namespace ecm2
{

LinearForm::LinearForm(int ne, int order, int ndofs, const int *gather_map_host, int q1d)
   : ne_(ne), order_(order), ndofs_(ndofs), bdr_(order, ndofs)
{
   ECM2_VERIFY(ne >= 0 && ndofs >= 0, ERR_ARG, "negative sizes");
   ECM2_VERIFY(order >= 1 && order + 1 <= MAX_D1D, ERR_ARG, "unsupported order " << order);
   ECM2_VERIFY(ne == 0 || gather_map_host != nullptr, ERR_ARG, "null gather map");
   require_device();
   D_ = order + 1;
   Q_ = q1d > 0 ? q1d : default_q1d(order);
   ECM2_VERIFY(Q_ <= MAX_Q1D && kern::has_lform(D_, Q_), ERR_UNSUPPORTED,
               "no linear-form kernel for order " << order << " with " << Q_
                                                  << " points (p = 1..4 with p + 1 or p + 2 points)");
   ND_ = D_ * D_ * D_;
   NQ_ = Q_ * Q_ * Q_;
   maps_ = make_dof_to_quad(order, Q_);
   basis_ = make_basis1d(maps_);
   for (int q = 0; q < Q_; q++) { qp_.x[q] = maps_.qpts[q]; }
   gmap_host_.assign(gather_map_host, gather_map_host + (size_t)ne * ND_);
   for (int g : gmap_host_)
   {
      const int d = g >= 0 ? g : -1 - g;
      ECM2_VERIFY(d >= 0 && d < ndofs, ERR_ARG, "gather map entry " << g << " out of range [0," << ndofs << ")");
   }
   gmap_.upload(gmap_host_);
   W_.upload(maps_.W);
   ECM2_HIP(hipDeviceSynchronize());
}

void LinearForm::set_element_nodes(const double *enodes_host)
{
   ECM2_VERIFY(ne_ == 0 || enodes_host, ERR_ARG, "null element nodes");
   enodes_.upload(enodes_host, (size_t)ne_ * 24);
   ECM2_HIP(hipDeviceSynchronize());
   jac_ = nullptr;
}

void LinearForm::set_jacobians(const double *J_device)
{
   ECM2_VERIFY(ne_ == 0 || J_device, ERR_ARG, "null Jacobian array");
   jac_ = J_device;
}

void LinearForm::set_attributes(const int *attr_host)
{
   ECM2_VERIFY(ne_ == 0 || attr_host, ERR_ARG, "null attribute array");
   attr_.assign(attr_host, attr_host + ne_);
   for (Integ &g : integs_) { g.emark_valid = false; }
}

void LinearForm::add_domain_integrator(const SourceDesc &c, const int *marker, int n_marker)
{
   ECM2_VERIFY(!marker || n_marker >= 0, ERR_ARG, "negative marker size");
   ECM2_VERIFY(c.kind == COEFF_CONSTANT || c.kind == COEFF_QUAD || c.kind == COEFF_GRIDFUNC ||
               c.kind == COEFF_GRIDFUNC_AFFINE || c.kind == COEFF_JOULE, ERR_ARG,
               "coefficient kind " << c.kind << " is not a scalar source of a DomainLFIntegrator");
   ECM2_VERIFY(c.kind != COEFF_QUAD || ne_ == 0 || c.quad, ERR_ARG, "null quadrature coefficient");
   const bool field = c.kind == COEFF_GRIDFUNC || c.kind == COEFF_GRIDFUNC_AFFINE || c.kind == COEFF_JOULE;
   ECM2_VERIFY(!field || ndofs_ == 0 || c.lvec, ERR_ARG, "null grid function");
   integs_.emplace_back();
   Integ &g = integs_.back();
   g.c = c;
   g.marked = marker != nullptr;
   g.marker.assign(marker, marker ? marker + n_marker : marker);
}

void LinearForm::set_boundary(int nbe, const int *bdr_map_host, const int *bdr_attr_host, const double *bdr_nodes_host, int q1d)
{
   const int q = q1d > 0 ? q1d : default_bdr_q1d(order_);
   ECM2_VERIFY(q == default_bdr_q1d(order_) || q == D_ || q == D_ + 1, ERR_UNSUPPORTED,
               "boundary rule of " << q << " points (the default, p + 1 or p + 2)");
   ECM2_VERIFY(bdr_.n_integrators() == 0, ERR_STATE, "set_boundary after a boundary integrator was added");
   bdr_.set_boundary(nbe, bdr_map_host, bdr_attr_host, bdr_nodes_host, q);
}

void LinearForm::set_boundary_detj(const double *detj_device) { bdr_.set_detj(detj_device); }

void LinearForm::add_boundary_integrator(const SourceDesc &c, const int *marker, int n_marker)
{
   BdrCoeff bc;
   bc.kind = c.kind;
   bc.value = c.value;
   bc.quad = c.quad;
   bdr_.add_integrator(bc, marker, n_marker);
}

void LinearForm::ensure_csr()
{
   if (csr_off_.size() || ndofs_ == 0) { return; }
   std::vector<int> off, idx;
   build_restriction_csr(gmap_host_, ndofs_, off, idx);
   csr_off_.upload(off);
   csr_idx_.upload(idx);
   ECM2_HIP(hipDeviceSynchronize());
}

void LinearForm::assemble(double *b, hipStream_t s)
{
   ECM2_VERIFY(ndofs_ == 0 || b, ERR_ARG, "null output vector");
   ECM2_VERIFY(ne_ == 0 || jac_ || enodes_.size(), ERR_STATE,
               "the linear form has no geometry (ecm2_linear_form_set_element_nodes / _set_jacobians)");
   if (ndofs_ == 0) { return; }
   if (integs_.empty() || ne_ == 0)
   {
      // (a form with boundary integrators only still overwrites b)
      ECM2_HIP(hipMemsetAsync(b, 0, (size_t)ndofs_ * sizeof(double), s));
      if (bdr_.n_integrators()) { bdr_.add_linear(b, s); }
      return;
   }
   // the markers of this assembly: 0 / 1 per element from the attributes (linearform_ext.cpp:49-61)
   for (Integ &g : integs_)
   {
      if (!g.marked || g.emark_valid) { continue; }
      ECM2_VERIFY((int)attr_.size() == ne_, ERR_STATE,
                  "a marked integrator needs the element attributes (ecm2_linear_form_set_attributes)");
      std::vector<int> m(ne_);
      for (int e = 0; e < ne_; e++)
      {
         const int a = attr_[e];
         ECM2_VERIFY(a <= (int)g.marker.size(), ERR_ARG, "element " << e << " has attribute " << a << " beyond the marker's "
                                                                   << g.marker.size() << " entries");
         m[e] = (a > 0 && g.marker[a - 1] != 0) ? 1 : 0;
      }
      g.emark.upload(m);
      ECM2_HIP(hipDeviceSynchronize());  // (m is a temporary)
      g.emark_valid = true;
   }
   ensure_csr();
   be_.resize((size_t)ne_ * ND_);
   if (integs_.size() > 1) { bwork_.resize(ndofs_); }
   for (size_t k = 0; k < integs_.size(); k++)
   {
      const Integ &g = integs_[k];
      kern::LFormArgs a;
      a.ne = ne_;
      a.kind = g.c.kind;
      a.gmap = gmap_.data();
      a.enodes = jac_ ? nullptr : enodes_.data();
      a.J = jac_;
      a.W = W_.data();
      a.qp = qp_;
      a.value = g.c.value;
      a.quad = g.c.quad;
      a.lvec = g.c.lvec;
      a.lvec2 = g.c.lvec2;
      a.scale = g.c.scale;
      a.slope = g.c.slope;
      a.t_ref = g.c.t_ref;
      a.emark = g.marked ? g.emark.data() : nullptr;
      a.be = be_.data();
      kern::lform_element_vectors(D_, Q_, a, basis_, s);
      // ElementRestriction::MultTranspose for the first integrator, AddMultTranspose for the others
      double *dst = k == 0 ? b : bwork_.data();
      kern::restriction_mult_transpose(ndofs_, ND_, csr_off_.data(), csr_idx_.data(), be_.data(), dst, s);
      if (k > 0) { kern::add_scaled(ndofs_, b, 1.0, bwork_.data(), b, s); }
   }
   // the boundary integrators, after the domain ones (linearform_ext.cpp:70-111)
   if (bdr_.n_integrators()) { bdr_.add_linear(b, s); }
}

} // namespace ecm2
