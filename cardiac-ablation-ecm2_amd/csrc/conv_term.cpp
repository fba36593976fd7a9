// conv_term.cpp -- see conv_term.hpp.
#include "conv_term.hpp"

#include <algorithm>

namespace ecm2
{

void ConvectionTerm::set(const CoeffDesc &c, double alpha, const int *marker, int n_marker)
{
   ECM2_VERIFY(c.kind == COEFF_CONST_VECTOR || c.kind == COEFF_QUAD_VECTOR, ERR_ARG,
               "coefficient kind " << c.kind << " is not a velocity (a constant vector or per-point vectors)");
   ECM2_VERIFY(c.kind != COEFF_QUAD_VECTOR || ne_ == 0 || c.quad, ERR_ARG, "null quadrature velocity");
   ECM2_VERIFY(!marker || n_marker >= 0, ERR_ARG, "negative marker size");
   ECM2_VERIFY(!present_, ERR_UNSUPPORTED, "a ConvectionIntegrator is already present");
   ECM2_VERIFY(kern::has_conv_apply(D_, Q_), ERR_UNSUPPORTED,
               "no convection kernel for order " << D_ - 1 << " with " << Q_ << " points (p = 1..4, p + 1 or p + 2 points)");
   c_ = c;
   alpha_ = alpha;
   marked_ = marker != nullptr;
   marker_.assign(marker, marker ? marker + n_marker : marker);
   present_ = true;
}

std::vector<unsigned char> ConvectionTerm::keep(const std::vector<int> &attr) const
{
   std::vector<unsigned char> k(ne_, 1);
   if (!marked_) { return k; }
   ECM2_VERIFY((int)attr.size() == ne_, ERR_STATE, "a marked integrator needs the element attributes "
                                                   "(ecm2_pa_form_set_attributes)");
   for (int e = 0; e < ne_; e++)
   {
      const int a = attr[e];
      ECM2_VERIFY(a <= (int)marker_.size(), ERR_ARG, "element " << e << " has attribute " << a
                                                      << " beyond the marker's " << marker_.size() << " entries");
      k[e] = (a > 0 && marker_[a - 1] != 0) ? 1 : 0;
   }
   return k;
}

kern::ConvSetupArgs ConvectionTerm::setup_args(const ConvGeometry &g, int n, const int *act, bool blocked,
                                               double *qd) const
{
   ECM2_VERIFY(g.enodes || g.J || n == 0, ERR_STATE, "the convection term has no geometry (corners or Jacobians)");
   kern::ConvSetupArgs a;
   a.n = n;
   a.q1d = Q_;
   a.blocked = blocked ? 1 : 0;
   a.act = act;
   a.enodes = g.J ? nullptr : g.enodes;
   a.J = g.J;
   a.W = g.W;
   a.qp = g.qp;
   a.alpha = alpha_;
   if (c_.kind == COEFF_CONST_VECTOR)
   {
      for (int i = 0; i < 3; i++) { a.v[i] = c_.cv[i]; }
   }
   else { a.vq = c_.quad; }
   a.qd = qd;
   return a;
}

void ConvectionTerm::assemble(const std::vector<int> &gmap_host, const std::vector<int> &attr, const ConvGeometry &g,
                              const Basis1D &basis, hipStream_t s)
{
   if (!present_) { return; }
   basis_ = basis;
   const ConvPlan p = build_conv_plan(gmap_host, ne_, ND_, ndofs_, keep(attr), blocked());
   plan_n_act_ = p.n_act;
   n_rows_ = p.n_rows;
   act_host_ = p.act;
   evec_ready_ = false;
   act_.upload(p.act, s);
   map_.upload(p.map, s);
   csr_dof_.upload(p.csr_dof, s);
   csr_off_.upload(p.csr_off, s);
   csr_idx_.upload(p.csr_idx, s);
   ye_.resize(p.ev_size);
   const size_t nslots = blocked() ? (size_t)((p.n_act + kConvBlock - 1) / kConvBlock) * kConvBlock : (size_t)p.n_act;
   qd_.resize(nslots * 3 * NQ_);
   ECM2_HIP(hipStreamSynchronize(s));  // the uploads read p
   kern::conv_setup_qdata(setup_args(g, p.n_act, act_.data(), blocked(), qd_.data()), s);
}

void ConvectionTerm::add_mult(const double *x, double *y, bool transpose, hipStream_t s)
{
   if (plan_n_act_ == 0) { return; }
   kern::conv_apply(D_, Q_, transpose, plan_n_act_, map_.data(), qd_.data(), x, ye_.data(), basis_, s);
   kern::conv_add(n_rows_, csr_dof_.data(), csr_off_.data(), csr_idx_.data(), ye_.data(), y, s);
}

void ConvectionTerm::add_mult_evec(const double *xe, double *ye, bool transpose, hipStream_t s)
{
   if (plan_n_act_ == 0) { return; }
   if (!evec_ready_)
   {
      // the E-vector as an "L-vector" of ne nd dofs with the identity as its gather map
      ECM2_VERIFY((size_t)ne_ * ND_ < ((size_t)1 << 31), ERR_UNSUPPORTED, "E-vector of " << (size_t)ne_ * ND_ << " entries");
      std::vector<int> ident((size_t)ne_ * ND_);
      for (size_t i = 0; i < ident.size(); i++) { ident[i] = (int)i; }
      std::vector<unsigned char> k(ne_, 0);
      for (int e : act_host_) { k[e] = 1; }
      const ConvPlan p = build_conv_plan(ident, ne_, ND_, ne_ * ND_, k, blocked());
      e_rows_ = p.n_rows;
      emap_.upload(p.map, s);
      ecsr_dof_.upload(p.csr_dof, s);
      ecsr_off_.upload(p.csr_off, s);
      ecsr_idx_.upload(p.csr_idx, s);
      ECM2_HIP(hipStreamSynchronize(s));  // the uploads read p
      evec_ready_ = true;
   }
   kern::conv_apply(D_, Q_, transpose, plan_n_act_, emap_.data(), qd_.data(), xe, ye_.data(), basis_, s);
   kern::conv_add(e_rows_, ecsr_dof_.data(), ecsr_off_.data(), ecsr_idx_.data(), ye_.data(), ye, s);
}

void ConvectionTerm::get_qdata(double *out_host, hipStream_t s)
{
   ECM2_VERIFY(present_, ERR_ARG, "convection integrator not present");
   ECM2_VERIFY(ne_ == 0 || out_host, ERR_ARG, "null output");
   const size_t per = (size_t)3 * NQ_;
   std::fill(out_host, out_host + (size_t)ne_ * per, 0.0);
   if (plan_n_act_ == 0) { return; }
   // the stored (Assemble-time) values of the active elements, decoded from the kernel's layout
   std::vector<double> h(qd_.size());
   qd_.download(h.data(), s);
   const bool blk = blocked();
   for (int k = 0; k < plan_n_act_; k++)
      for (int c = 0; c < 3; c++)
         for (int q = 0; q < NQ_; q++)
         {
            const size_t src = blk ? (((size_t)(k / kConvBlock) * NQ_ + q) * 3 + c) * kConvBlock + (k % kConvBlock)
                                   : ((size_t)k * 3 + c) * NQ_ + q;
            out_host[(size_t)act_host_[k] * per + (size_t)c * NQ_ + q] = h[src];
         }
}

} // namespace ecm2
