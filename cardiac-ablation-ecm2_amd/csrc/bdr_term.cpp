// bdr_term.cpp -- see bdr_term.hpp.
#include "bdr_term.hpp"

#include <algorithm>
#include <utility>

namespace ecm2
{

void BoundaryTerm::set_boundary(int nbe, const int *bdr_map, const int *bdr_attr, const double *bdr_nodes, int q1d)
{
   ECM2_VERIFY(nbe >= 0, ERR_ARG, "negative boundary element count");
   ECM2_VERIFY(nbe == 0 || (bdr_map && bdr_attr), ERR_ARG, "null boundary map or attributes");
   ECM2_VERIFY(q1d >= 1 && q1d <= MAX_Q1D, ERR_UNSUPPORTED, "boundary rule of " << q1d << " points");
   const int dd = D_ * D_;
   std::vector<int> bm(bdr_map, bdr_map + (size_t)nbe * dd);
   for (int g : bm) { ECM2_VERIFY(g >= 0 && g < ndofs_, ERR_ARG, "boundary map entry " << g << " out of range [0," << ndofs_ << ")"); }
   nbe_ = nbe;
   Q_ = q1d;
   bmap_host_.swap(bm);
   attr_.assign(bdr_attr, bdr_attr + nbe);
   bmap_.upload(bmap_host_);
   if (bdr_nodes) { nodes_.upload(bdr_nodes, (size_t)nbe * 12); }
   else { nodes_.resize(0); }
   maps_ = make_dof_to_quad(order_, Q_);
   basis_ = make_basis1d(maps_);
   Bdev_.upload(maps_.B);
   std::vector<double> w2((size_t)Q_ * Q_);
   for (int j = 0; j < Q_; j++)
      for (int i = 0; i < Q_; i++) { w2[i + Q_ * j] = maps_.qw1[i] * maps_.qw1[j]; }
   wq_.upload(w2);
   qpts_.upload(maps_.qpts);
   ECM2_HIP(hipDeviceSynchronize());  // (w2 is a temporary)
   have_bdr_ = true;
   prepared_ = false;
}

void BoundaryTerm::set_detj(const double *detj_device)
{
   ECM2_VERIFY(have_bdr_, ERR_STATE, "a boundary detJ array needs the boundary first (set_boundary)");
   ECM2_VERIFY(nbe_ == 0 || detj_device, ERR_ARG, "null boundary detJ array");
   detj_ = detj_device;
}

void BoundaryTerm::add_integrator(const BdrCoeff &c, const int *marker, int n_marker)
{
   ECM2_VERIFY(have_bdr_, ERR_STATE, "a boundary integrator needs the boundary first (set_boundary)");
   ECM2_VERIFY(c.kind == COEFF_CONSTANT || c.kind == COEFF_QUAD, ERR_ARG,
               "coefficient kind " << c.kind << " is not supported on boundary faces (constant or per-point values)");
   ECM2_VERIFY(c.kind != COEFF_QUAD || nbe_ == 0 || c.quad, ERR_ARG, "null boundary quadrature coefficient");
   ECM2_VERIFY(!marker || n_marker >= 0, ERR_ARG, "negative marker size");
   integs_.emplace_back();
   Integ &g = integs_.back();
   g.c = c;
   g.marked = marker != nullptr;
   g.marker.assign(marker, marker ? marker + n_marker : marker);
   prepared_ = false;
}

std::vector<double> BoundaryTerm::face_weights(const Integ &g) const
{
   std::vector<double> w(nbe_, 1.0);
   if (!g.marked) { return w; }
   for (int f = 0; f < nbe_; f++)
   {
      const int a = attr_[f];
      ECM2_VERIFY(a <= (int)g.marker.size(), ERR_ARG, "boundary element " << f << " has attribute " << a
                                                       << " beyond the marker's " << g.marker.size() << " entries");
      w[f] = (a > 0 && g.marker[a - 1] != 0) ? 1.0 : 0.0;
   }
   return w;
}

void BoundaryTerm::prepare(hipStream_t s)
{
   if (prepared_) { return; }
   const int ni = n_integrators(), dd = D_ * D_;
   std::vector<std::vector<double>> w(ni);
   for (int i = 0; i < ni; i++) { w[i] = face_weights(integs_[i]); }
   // the diagonal's weights: every marked integrator added at or after j masks j's part
   // (the reference adds every integrator's diagonal into one face vector and zeroes a marked one's
   // excluded faces of that vector after adding it)
   std::vector<std::vector<double>> wd(ni);
   std::vector<double> mask(nbe_, 1.0);
   for (int j = ni - 1; j >= 0; j--)
   {
      if (integs_[j].marked)
      {
         for (int f = 0; f < nbe_; f++) { mask[f] *= w[j][f]; }
      }
      wd[j] = mask;
   }
   std::vector<int> act;
   for (int f = 0; f < nbe_; f++)
   {
      bool any = false;
      for (int i = 0; i < ni && !any; i++) { any = w[i][f] != 0.0; }
      if (any) { act.push_back(f); }
   }
   n_act_ = (int)act.size();
   faces_.upload(act, s);
   diag_differs_ = false;
   std::vector<std::vector<double>> hw(ni), hwd(ni);
   for (int i = 0; i < ni; i++)
   {
      hw[i].resize(n_act_);
      hwd[i].resize(n_act_);
      for (int k = 0; k < n_act_; k++)
      {
         hw[i][k] = w[i][act[k]];
         hwd[i][k] = wd[i][act[k]];
      }
      diag_differs_ = diag_differs_ || hw[i] != hwd[i];
      integs_[i].w.upload(hw[i], s);
      integs_[i].wdiag.upload(hwd[i], s);
   }
   // CSR over the dofs of the active faces: each dof's entries of the face vectors [k][d1d^2] in
   // ascending face (then local) order
   std::vector<std::pair<int, int>> ent;
   ent.reserve((size_t)n_act_ * dd);
   for (int k = 0; k < n_act_; k++)
      for (int i = 0; i < dd; i++) { ent.emplace_back(bmap_host_[(size_t)act[k] * dd + i], k * dd + i); }
   std::sort(ent.begin(), ent.end());
   std::vector<int> dof, off, idx(ent.size());
   for (size_t e = 0; e < ent.size(); e++)
   {
      if (e == 0 || ent[e].first != ent[e - 1].first)
      {
         dof.push_back(ent[e].first);
         off.push_back((int)e);
      }
      idx[e] = ent[e].second;
   }
   off.push_back((int)ent.size());
   n_rows_ = (int)dof.size();
   csr_dof_.upload(dof, s);
   csr_off_.upload(off, s);
   csr_idx_.upload(idx, s);
   yf_.resize((size_t)n_act_ * dd);
   ECM2_HIP(hipStreamSynchronize(s));  // the uploads read host temporaries
   prepared_ = true;
}

kern::BdrSetupArgs BoundaryTerm::setup_args(const Integ &g, const double *wf, double *qd, bool accumulate) const
{
   ECM2_VERIFY(detj_ || nodes_.size() || nbe_ == 0, ERR_STATE, "the boundary has no geometry (corners or a detJ array)");
   kern::BdrSetupArgs a;
   a.n = n_act_;
   a.q1d = Q_;
   a.faces = faces_.data();
   a.nodes = detj_ ? nullptr : nodes_.data();
   a.detj = detj_;
   a.wq = wq_.data();
   a.qpts = qpts_.data();
   a.value = g.c.kind == COEFF_CONSTANT ? g.c.value : 1.0;
   a.quad = g.c.kind == COEFF_QUAD ? g.c.quad : nullptr;
   a.wf = wf;
   a.qd = qd;
   a.accumulate = accumulate;
   return a;
}

void BoundaryTerm::assemble_mass(hipStream_t s)
{
   prepare(s);
   ECM2_VERIFY(n_integrators() == 0 || kern::has_bdr_apply(D_, Q_), ERR_UNSUPPORTED,
               "no face mass kernel for order " << order_ << " with " << Q_ << " points");
   const size_t nq = (size_t)Q_ * Q_;
   qd_.resize((size_t)n_act_ * nq);
   qd_diag_.resize(diag_differs_ ? (size_t)n_act_ * nq : 0);
   if (n_act_ == 0) { return; }
   for (int i = 0; i < n_integrators(); i++)
   {
      const Integ &g = integs_[i];
      kern::bdr_setup_qdata(setup_args(g, g.w.data(), qd_.data(), i > 0), s);
      if (diag_differs_) { kern::bdr_setup_qdata(setup_args(g, g.wdiag.data(), qd_diag_.data(), i > 0), s); }
   }
}

void BoundaryTerm::add_mult(const double *x, double *y, hipStream_t s)
{
   if (n_act_ == 0) { return; }
   kern::bdr_mass_apply(D_, Q_, n_act_, faces_.data(), bmap_.data(), qd_.data(), x, yf_.data(), basis_, Bdev_.data(), s);
   kern::bdr_add(n_rows_, csr_dof_.data(), csr_off_.data(), csr_idx_.data(), yf_.data(), y, s);
}

void BoundaryTerm::add_diagonal(double *diag, hipStream_t s)
{
   if (n_act_ == 0) { return; }
   kern::bdr_transpose_apply(D_, Q_, n_act_, diag_differs_ ? qd_diag_.data() : qd_.data(), true, yf_.data(),
                             Bdev_.data(), s);
   kern::bdr_add(n_rows_, csr_dof_.data(), csr_off_.data(), csr_idx_.data(), yf_.data(), diag, s);
}

void BoundaryTerm::get_qdata(int index, double *out_host, hipStream_t s)
{
   ECM2_VERIFY(index >= 0 && index < n_integrators(), ERR_ARG, "boundary integrator " << index << " not present");
   ECM2_VERIFY(nbe_ == 0 || out_host, ERR_ARG, "null output");
   if (nbe_ == 0) { return; }
   const Integ &g = integs_[index];
   std::vector<int> all(nbe_);
   for (int f = 0; f < nbe_; f++) { all[f] = f; }
   DeviceArray<int> faces;
   DeviceArray<double> w, qd;
   faces.upload(all, s);
   w.upload(face_weights(g), s);
   ECM2_HIP(hipStreamSynchronize(s));  // (the weights are a temporary)
   qd.resize((size_t)nbe_ * Q_ * Q_);
   kern::BdrSetupArgs a = setup_args(g, w.data(), qd.data(), false);
   a.n = nbe_;
   a.faces = faces.data();
   kern::bdr_setup_qdata(a, s);
   qd.download(out_host, s);
}

void BoundaryTerm::add_linear(double *b, hipStream_t s)
{
   prepare(s);
   if (n_act_ == 0) { return; }
   qd_.resize((size_t)n_act_ * Q_ * Q_);
   for (const Integ &g : integs_)
   {
      kern::bdr_setup_qdata(setup_args(g, g.w.data(), qd_.data(), false), s);
      kern::bdr_transpose_apply(D_, Q_, n_act_, qd_.data(), false, yf_.data(), Bdev_.data(), s);
      kern::bdr_add(n_rows_, csr_dof_.data(), csr_off_.data(), csr_idx_.data(), yf_.data(), b, s);
   }
}

} // namespace ecm2
