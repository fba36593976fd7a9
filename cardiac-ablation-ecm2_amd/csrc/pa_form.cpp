// pa_form.cpp -- see pa_form.hpp.  The device side of a form: geometry, qdata, uploads and kernel
// launches.  What the fused kernels' deterministic scatter needs (element order, merge flags, maps,
// lattice units, partial slots, the summation plan) is planned on the host in scatter_plan.cpp;
// plan_tpe / plan_line below call it and hand the result to the plan objects (plan_dev.hpp).
#include "pa_form.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

namespace ecm2
{

void require_device()
{
   int n = 0;
   const hipError_t e = hipGetDeviceCount(&n);
   ECM2_VERIFY(e == hipSuccess && n > 0, ERR_HIP,
               "no HIP device available (the PA path has no CPU fallback)");
}

PAForm::PAForm(int ne, int order, int ndofs, const int *gather_map_host, int q1d, int n_owned)
   : ne_(ne), order_(order), ndofs_(ndofs), n_owned_(n_owned < 0 ? ndofs : n_owned), bdr_(order, ndofs),
     conv_(ne, order, q1d > 0 ? q1d : default_q1d(order), ndofs)
{
   ECM2_VERIFY(n_owned_ <= ndofs, ERR_ARG, "n_owned > ndofs");
   ECM2_VERIFY(ne >= 0 && ndofs >= 0, ERR_ARG, "negative sizes");
   ECM2_VERIFY(order >= 1 && order + 1 <= MAX_D1D, ERR_ARG, "unsupported order " << order);
   ECM2_VERIFY(ne == 0 || gather_map_host != nullptr, ERR_ARG, "null gather map");
   require_device();
   D_ = order + 1;
   Q_ = q1d > 0 ? q1d : default_q1d(order);
   ECM2_VERIFY(Q_ >= D_ && Q_ <= MAX_Q1D, ERR_ARG, "q1d must satisfy p+1 <= q1d <= " << MAX_Q1D);
   ND_ = D_ * D_ * D_;
   NQ_ = Q_ * Q_ * Q_;
   maps_ = make_dof_to_quad(order, Q_);
   basis_ = make_basis1d(maps_);
   basis1_ = make_basis1d(make_dof_to_quad(1, Q_));
   for (int q = 0; q < Q_; q++) { qp_.x[q] = maps_.qpts[q]; }
   gmap_host_.assign(gather_map_host, gather_map_host + (size_t)ne * ND_);
   for (int g : gmap_host_)
   {
      const int d = g >= 0 ? g : -1 - g;
      ECM2_VERIFY(d >= 0 && d < ndofs, ERR_ARG, "gather map entry " << g << " out of range [0," << ndofs << ")");
   }
   gmap_.upload(gmap_host_);
   W_.upload(maps_.W);
   layout_.ne = ne;
   layout_.nq = NQ_;
}

PAForm::~PAForm()
{
   for (auto &e : ev_start_) { (void)hipEventDestroy(e); }
   for (auto &e : ev_stop_) { (void)hipEventDestroy(e); }
}

// Every element a parallelepiped: the trilinear map's bilinear and trilinear terms vanish
// (to 1e-13 of the element's edge length, i.e. below the operator's 1e-12 parity bar), so
// its Jacobian is constant.  Terms are differences of edge vectors (exact for lattices).
static bool all_affine(int ne, const double *X)
{
   for (int e = 0; e < ne; e++)
   {
      const double *p = X + (size_t)e * 24;
      double h = 0.0, dev = 0.0;
      for (int i = 0; i < 3; i++)
      {
         const double *c = p + i * 8;  // corner a = ax + 2 ay + 4 az
         const double ex = c[1] - c[0], ey = c[2] - c[0], ez = c[4] - c[0];
         h = std::max({h, std::fabs(ex), std::fabs(ey), std::fabs(ez)});
         dev = std::max({dev, std::fabs((c[3] - c[2]) - ex), std::fabs((c[5] - c[4]) - ex),
                         std::fabs((c[6] - c[4]) - ey), std::fabs((c[7] - c[6]) - ex),
                         std::fabs((c[7] - c[5]) - ey), std::fabs((c[7] - c[3]) - ez)});
      }
      if (!(dev <= 1e-13 * h)) { return false; }
   }
   return true;
}

void PAForm::set_element_nodes(const double *enodes_host)
{
   ECM2_VERIFY(ne_ == 0 || enodes_host, ERR_ARG, "null element nodes");
   enodes_.upload(enodes_host, (size_t)ne_ * 24);
   ECM2_HIP(hipDeviceSynchronize());
   affine_ = all_affine(ne_, enodes_host);
   jac_ = nullptr;
   assembled_ = false;
}

void PAForm::set_jacobians(const double *J_device)
{
   ECM2_VERIFY(ne_ == 0 || J_device, ERR_ARG, "null Jacobian array");
   jac_ = J_device;
   affine_ = false;
   assembled_ = false;
}

void PAForm::set_geometry_compression(bool on)
{
   compress_ = on;
   assembled_ = false;
}

void PAForm::set_coefficient_snapshot(bool on)
{
   tsnap_pref_ = on;
   assembled_ = false;
}

void PAForm::set_block_splits(const std::vector<int> &splits)
{
   for (int b : splits) { ECM2_VERIFY(b >= 0 && b <= layout_.nblk(), ERR_ARG, "block split " << b << " out of range"); }
   splits_ = splits;
   // (the derived element order, the workgroup groups of the merge plan and the bricks respect the segments)
   invalidate_plans(true, true);
   assembled_ = false;
}

void PAForm::set_latency_from(int b)
{
   latency_from_ = b;
   invalidate_plans(true, false);  // the face-assembly plan depends on it
   assembled_ = false;
}

void PAForm::set_line_bricks(int bz)
{
   ECM2_VERIFY(bz >= -1 && bz <= 2, ERR_ARG, "brick mode " << bz << " not in {-1, 0, 1, 2}");
   line_bricks_ = bz;
   invalidate_plans(false, true);
   assembled_ = false;
}

void PAForm::set_attributes(const int *attr_host)
{
   ECM2_VERIFY(ne_ == 0 || attr_host, ERR_ARG, "null attribute array");
   attr_.assign(attr_host, attr_host + ne_);
   assembled_ = false;
}

void PAForm::add_integrator(int kind, const CoeffDesc &c, const int *marker, int n_marker)
{
   ECM2_VERIFY(!marker || n_marker >= 0, ERR_ARG, "negative marker size");
   ECM2_VERIFY(kind == INTEG_MASS || kind == INTEG_DIFFUSION, ERR_ARG, "unknown integrator " << kind);
   ECM2_VERIFY(c.kind >= COEFF_CONSTANT && c.kind <= COEFF_GRIDFUNC, ERR_ARG, "unknown coefficient kind " << c.kind);
   ECM2_VERIFY(c.dim() == 1 || kind == INTEG_DIFFUSION, ERR_ARG,
               "vector / matrix coefficients belong to a DiffusionIntegrator");
   ECM2_VERIFY(!c.quad_values() || ne_ == 0 || c.quad, ERR_ARG, "null quadrature coefficient");
   ECM2_VERIFY(!c.gridfunc() || ndofs_ == 0 || c.lvec, ERR_ARG, "null grid function");
   if (kind == INTEG_MASS)
   {
      ECM2_VERIFY(!have_mass_, ERR_UNSUPPORTED, "a MassIntegrator is already present");
      have_mass_ = true;
      cmass_ = c;
   }
   else
   {
      ECM2_VERIFY(!have_diff_, ERR_UNSUPPORTED, "a DiffusionIntegrator is already present");
      have_diff_ = true;
      cdiff_ = c;
   }
   // (the marker state changes only once the integrator is accepted: a rejected duplicate leaves
   // the installed one untouched)
   marked_[kind] = marker != nullptr;
   marker_[kind].assign(marker, marker ? marker + n_marker : marker);
   order_added_.push_back(kind);
   invalidate_plans(false, true);  // bricks need both integrators
   assembled_ = false;
}

void PAForm::add_convection(const CoeffDesc &c, double alpha, const int *marker, int n_marker)
{
   ECM2_VERIFY(n_owned_ == ndofs_, ERR_UNSUPPORTED, "a distributed local form has no convection integrator");
   conv_.set(c, alpha, marker, n_marker);
   assembled_ = false;
}

void PAForm::convection_info(int *present, int *n_active, int *transpose_distinct) const
{
   if (present) { *present = conv_.present() ? 1 : 0; }
   if (n_active) { *n_active = conv_.n_active(); }
   if (transpose_distinct) { *transpose_distinct = conv_.n_active() > 0 ? 1 : 0; }
}

void PAForm::set_boundary(int nbe, const int *bdr_map_host, const int *bdr_attr_host, const double *bdr_nodes_host, int q1d)
{
   ECM2_VERIFY(n_owned_ == ndofs_, ERR_UNSUPPORTED, "a distributed local form has no boundary integrators");
   const int q = q1d > 0 ? q1d : D_;  // MassIntegrator::GetRule on the boundary quad: p + 1 points
   ECM2_VERIFY(q == D_ || q == D_ + 1, ERR_UNSUPPORTED, "boundary rule of " << q << " points (p + 1 or p + 2)");
   ECM2_VERIFY(kern::has_bdr_apply(D_, q), ERR_UNSUPPORTED, "no face mass kernel for order " << order_);
   ECM2_VERIFY(bdr_.n_integrators() == 0, ERR_STATE, "set_boundary after a boundary integrator was added");
   bdr_.set_boundary(nbe, bdr_map_host, bdr_attr_host, bdr_nodes_host, q);
   assembled_ = false;
}

void PAForm::set_boundary_detj(const double *detj_device)
{
   bdr_.set_detj(detj_device);
   assembled_ = false;
}

void PAForm::add_boundary_integrator(int kind, const CoeffDesc &c, const int *marker, int n_marker)
{
   ECM2_VERIFY(kind == INTEG_MASS || kind == INTEG_DIFFUSION, ERR_ARG, "unknown integrator " << kind);
   ECM2_VERIFY(kind == INTEG_MASS, ERR_UNSUPPORTED, "only a MassIntegrator is supported on the boundary");
   BdrCoeff bc;
   bc.kind = c.kind;
   bc.value = c.value;
   bc.quad = c.quad;
   bdr_.add_integrator(bc, marker, n_marker);
   assembled_ = false;
}

void PAForm::get_boundary_qdata(int index, double *out_host, hipStream_t s)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "get_boundary_qdata before Assemble");
   bdr_.get_qdata(index, out_host, s);
}

void PAForm::boundary_info(int *nbe, int *n_integrators, int *n_active, int *q1d) const
{
   if (nbe) { *nbe = bdr_.nbe(); }
   if (n_integrators) { *n_integrators = bdr_.n_integrators(); }
   if (n_active) { *n_active = bdr_.n_active(); }
   if (q1d) { *q1d = bdr_.q1d(); }
}

void PAForm::set_element_order(const int *perm)
{
   std::vector<int> seen(ne_, 0);
   user_perm_.assign(perm, perm + ne_);
   for (int e : user_perm_)
   {
      ECM2_VERIFY(e >= 0 && e < ne_ && !seen[e], ERR_ARG, "element order is not a permutation");
      seen[e] = 1;
   }
   invalidate_plans(true, false);
   assembled_ = false;
}

void PAForm::set_kernel(int mode)
{
   ECM2_VERIFY(mode >= KERNEL_AUTO && mode <= KERNEL_LINE, ERR_ARG, "unknown kernel mode " << mode);
   mode_ = mode;
   invalidate_plans(true, true);  // the summation plan belongs to one fused kernel
   assembled_ = false;
}

void PAForm::invalidate_plans(bool tpe, bool line)
{
   if (tpe) { tpe_.reset(); }
   if (line) { line_.reset(); }
}

static bool has_tpe(int D, int Q) { return (D == 2 && Q == 3) || (D == 3 && Q == 4); }

// Assemble: the kernel and the qdata layout, the fused kernel's scatter plan (scatter_plan.hpp:
// built on the host, uploaded here, kept until an input of it changes), then the quadrature data.
void PAForm::assemble(hipStream_t s)
{
   ECM2_VERIFY(enodes_.size() || jac_ || ne_ == 0, ERR_STATE, "assemble: no geometry set");
   resolve_layout(s);
   plan_tpe(s);
   if (!btab_.size())
   {
      const BasisDev bd = make_basis_dev(basis_, D_, Q_);
      btab_.upload(&bd, 1, s);
   }
   plan_line(s);
   layout_.pos = layout_.blocked() ? tpe_.pos.data() : nullptr;
   layout_.perm = layout_.blocked() ? tpe_.perm_dev.data() : nullptr;
   if (!use_partials()) { part_.resize(0); }
   else if (resolved_mode_ == KERNEL_LINE)
   {
      // [bricks' lattice slots | leftover elements' [e][nd] slots (when there are any)]
      part_.resize(std::max<size_t>(1, (size_t)line_.info.part_line_off + (line_.info.n_left ? (size_t)ne_ * ND_ : 0)));
   }
   else { part_.resize((size_t)layout_.nblk() * tpe_.info.part_stride); }
   choose_snapshot(s);
   setup_qdata(s);
   setup_marker_diagonal(s);
   build_launch_args();
   if (bdr_.has_boundary()) { bdr_.assemble_mass(s); }  // face qdata and the add pass's CSR
   if (conv_.present())
   {
      // the active elements' rows, the add pass's CSR and the qdata from the live velocity
      ConvGeometry g;
      g.enodes = enodes_.data();
      g.J = jac_;
      g.W = W_.data();
      g.qp = qp_;
      conv_.assemble(gmap_host_, attr_, g, basis_, s);
   }
   assembled_ = true;
   gen_++;
}

void PAForm::resolve_layout(hipStream_t s)
{
   resolved_mode_ = mode_;
   if (mode_ == KERNEL_AUTO)
   {
      resolved_mode_ = has_tpe(D_, Q_) ? KERNEL_TPE : (kern::has_line(D_, Q_) ? KERNEL_LINE : KERNEL_WPE);
   }
   ECM2_VERIFY(resolved_mode_ != KERNEL_TPE || has_tpe(D_, Q_), ERR_UNSUPPORTED,
               "thread-per-element kernel needs (D1D,Q1D) in {(2,3),(3,4)}");
   ECM2_VERIFY(resolved_mode_ != KERNEL_LINE || kern::has_line(D_, Q_), ERR_UNSUPPORTED,
               "line kernel needs Q1D in {D1D, D1D+1} and Q1D <= 8");
   // a general (nonsymmetric) matrix coefficient: the reference's 9-entry qdata (NATIVE9), read by
   // the workgroup-per-element kernels; any other vector / matrix coefficient keeps 6 symmetric
   // entries but varies per point in direction: no geometry compression
   const int cdim = have_diff_ ? cdiff_.dim() : 1;
   if (cdim == 9)
   {
      ECM2_VERIFY(mode_ == KERNEL_AUTO || mode_ == KERNEL_WPE || mode_ == KERNEL_UNFUSED, ERR_UNSUPPORTED,
                  "a general matrix coefficient runs the workgroup-per-element or unfused kernels");
      if (mode_ == KERNEL_AUTO) { resolved_mode_ = KERNEL_WPE; }
   }
   layout_.kind = (resolved_mode_ == KERNEL_TPE) ? QLAYOUT_BLOCKED : (cdim == 9 ? QLAYOUT_NATIVE9 : QLAYOUT_NATIVE);
   layout_.pw = 2;
   // Compressed geometry for the fused kernels (thread-per-element p <= 2: AFFINE / TRILINEAR;
   // line / brick p >= 3: AFFINE_E / TRILINEAR_E), with both integrators or a diffusion-only form
   // such as ex16's K (point values W beta [/ det J] alone, 8 B per point).  A mass-only form keeps
   // the mass stream, already one 8-byte W alpha det J per point.
   const bool fused = resolved_mode_ == KERNEL_TPE || resolved_mode_ == KERNEL_LINE;
   const bool comp = compress_ && have_diff_ && cdim == 1 && fused;
   const bool tpe = resolved_mode_ == KERNEL_TPE;
   bool affine = affine_;
   if (jac_ && comp)
   {
      affine = kern::jacobians_affine(ne_, NQ_, jac_, s);  // the reference binding's geometry
   }
   if (affine && comp)
   {
      layout_.kind = tpe ? QLAYOUT_AFFINE : QLAYOUT_AFFINE_E;
      layout_.pw = have_mass_ ? 2 : 1;
   }
   else if (!affine && comp)
   {
      // general trilinear hexes: the map coefficients per element (from the corners, or fitted
      // to the reference binding's Jacobians when they are a trilinear map's), J per point
      bool tl = !jac_ && enodes_.size();
      if (jac_)
      {
         cfit_.resize(std::max(1, ne_) * 21);
         tl = kern::jacobians_trilinear_fit(ne_, Q_, qp_, jac_, cfit_.data(), s);
      }
      if (tl)
      {
         layout_.kind = tpe ? QLAYOUT_TRILINEAR : QLAYOUT_TRILINEAR_E;
         layout_.pw = have_mass_ ? 2 : 1;
      }
   }
}

void PAForm::plan_tpe(hipStream_t s)
{
   // the merge plan (cross-wave faces), the regular blocks and the partial-slot layout belong
   // to the qdata layout they were built for
   if (tpe_.valid && tpe_.kind != layout_.kind) { invalidate_plans(true, false); }
   if (resolved_mode_ != KERNEL_TPE || tpe_.valid || ne_ == 0) { return; }
   const bool lattice_layout = layout_.kind == QLAYOUT_AFFINE || layout_.kind == QLAYOUT_TRILINEAR;
   const TpePlan p = build_tpe_plan(ne_, D_, ndofs_, n_owned_, gmap_host_, user_perm_, splits_, latency_from_,
                                    lattice_layout, plan_options_from_env());
   tpe_.upload(p, layout_.kind, s);
   shared_.upload(p.shared, s);
   rowtab_.upload(kern::make_row_table(maps_), s);
   drowtab_.upload(kern::make_diag_row_table(maps_), s);
   ECM2_HIP(hipStreamSynchronize(s));  // the uploads read p
}

void PAForm::plan_line(hipStream_t s)
{
   if (resolved_mode_ != KERNEL_LINE || line_.valid || ne_ == 0) { return; }
   // default 2 x 2 x 1 (C5, profiles/ab_brick.sh: 0.861 ms against 1.018 ms per element and
   // 1.114 ms for 2 x 2 x 2)
   int bz = (scatter_ == SCATTER_PARTIALS && have_mass_ && have_diff_) ? (line_bricks_ >= 0 ? line_bricks_ : 1) : 0;
   if (bz == 2 && !kern::has_brick(D_, Q_, 2)) { bz = 1; }
   if (bz == 1 && !kern::has_brick(D_, Q_, 1)) { bz = 0; }
   const LinePlan p = build_line_plan(ne_, D_, ndofs_, n_owned_, gmap_host_, splits_, bz, plan_options_from_env());
   line_.upload(p, s);
   shared_.upload(p.shared, s);
   ECM2_HIP(hipStreamSynchronize(s));  // the uploads read p
}

void PAForm::choose_snapshot(hipStream_t s)
{
   // Coefficient snapshot (k_apply_tpe_ts): the diffusion coefficient a law of an H1 field on this
   // space (GridFunctionCoefficient, AffineGridFunctionCoefficient, the perfusion law), AFFINE
   // geometry, p = 2, every block a lattice brick, no attribute marker on the diffusion integrator.
   // The mass then streams W alpha det J per point (tmass 1), or nothing per point when its
   // coefficient is a constant or a law of the same field (tmass 2: (c alpha) det J per element).
   layout_.tsnap = 0;
   layout_.tmass = 0;
   layout_.tlaw = 0;
   tsnap_.resize(0);
   // (p >= 3: the same snapshot in the brick kernel was measured and rejected, profiles/r5/ab_c5*.txt)
   const bool ts_tpe = layout_.kind == QLAYOUT_AFFINE && resolved_mode_ == KERNEL_TPE && D_ == 3 && Q_ == 4 &&
                       (tpe_.info.treg_all || tpe_.info.tlat_all);
   if (tsnap_pref_ && ts_tpe && have_diff_ && cdiff_.gridfunc() && cdiff_.lvec && !marked_[INTEG_DIFFUSION])
   {
      layout_.tsnap = 1;
      const bool mass_law = have_mass_ && cmass_.gridfunc() && cmass_.lvec == cdiff_.lvec;
      layout_.tmass = !have_mass_ ? 0 : (cmass_.kind == COEFF_CONSTANT || mass_law) ? 2 : 1;
      layout_.pw = layout_.tmass == 1 ? 1 : 0;
      // an affine (or identity) diffusion law alone is applied to the dofs (the interpolated T' is
      // the law at the point: the basis sums to 1); a nonlinear law, or a mass law of the same field,
      // needs the field itself at the point
      layout_.tlaw = (mass_law || cdiff_.kind == COEFF_GRIDFUNC_PERFUSION) ? 1 : 0;
      // T' = A + B T at every dof, taken here only: the Assemble-time field (the reference's qdata
      // semantics; the diagonal and the qdata export read the same snapshot)
      double A = 0.0, B = 1.0;
      if (!layout_.tlaw && cdiff_.kind == COEFF_GRIDFUNC_AFFINE)
      {
         A = cdiff_.scale * (1.0 - cdiff_.slope * cdiff_.t_ref);
         B = cdiff_.scale * cdiff_.slope;
      }
      if (tpe_.info.treg_all)
      {
         tsnap_.resize(std::max(1, ndofs_));
         kern::affine_snapshot(ndofs_, cdiff_.lvec, A, B, tsnap_.data(), s);
      }
      else
      {
         // lattice-map blocks (the reference's numbering): the snapshot in their lattice-slot order,
         // read contiguously by the kernel (no second dependent gather through the map)
         layout_.tsnap = 2;
         const int nlp = tpe_lattice_points(D_);
         tsnap_.resize((size_t)layout_.nblk() * nlp);
         kern::affine_snapshot_lattice(layout_.nblk(), nlp, tpe_.lmap.data(), cdiff_.lvec, A, B, tsnap_.data(), s);
      }
   }
}

// The marker diagonal's element weights (assemble_diagonal), from the Assemble-time attributes
// (the reference reads them in SetupRestrictionOperators, bilinearform_ext.cpp:269)
void PAForm::setup_marker_diagonal(hipStream_t s)
{
   diag_integ_ = -1;
   diag_w_.resize(0);
   if (order_added_.size() == 2 && marked_[order_added_[1]])
   {
      const int F = order_added_[0], S = order_added_[1];
      const std::vector<double> wf = marker_weights(F), ws = marker_weights(S);
      bool differ = false;
      for (int e = 0; e < ne_ && !differ; e++) { differ = wf[e] != 0.0 && ws[e] == 0.0; }
      if (differ)
      {
         diag_integ_ = F;
         diag_w_.upload(ws, s);
         ECM2_HIP(hipStreamSynchronize(s));  // ws is a host temporary
      }
   }
}

std::vector<double> PAForm::marker_weights(int k) const
{
   std::vector<double> w(ne_, 1.0);
   if (!marked_[k]) { return w; }
   ECM2_VERIFY((int)attr_.size() == ne_, ERR_STATE, "a marked integrator needs the element attributes "
                                                    "(ecm2_pa_form_set_attributes)");
   for (int e = 0; e < ne_; e++)
   {
      const int a = attr_[e];
      ECM2_VERIFY(a <= (int)marker_[k].size(), ERR_ARG, "element " << e << " has attribute " << a
                                                         << " beyond the marker's " << marker_[k].size() << " entries");
      w[e] = (a > 0 && marker_[k][a - 1] != 0) ? 1.0 : 0.0;
   }
   return w;
}

const double *PAForm::coeff_points(const CoeffDesc &c, DeviceArray<double> &tmp, hipStream_t s) const
{
   if (c.quad_values()) { return c.quad; }
   if (c.gridfunc())
   {
      tmp.resize((size_t)ne_ * NQ_);
      kern::coeff_gridfunc(ne_, D_, Q_, gmap_.data(), basis_, btab(), c, tmp.data(), s);
      return tmp.data();
   }
   return nullptr;
}

void PAForm::setup_qdata(hipStream_t s)
{
   // (compressed layouts: qd_mass_ holds the point values, present with either integrator)
   const bool comp = layout_.compressed();
   qd_diff_.resize(have_diff_ ? layout_.diff_size() : 0);
   qd_mass_.resize(have_mass_ || comp ? layout_.mass_size() : 0);
   // the setup kernels write every entry except the padding lanes of a partial last block
   // (blocked layout), which are cleared so the apply kernels stream defined values
   if (layout_.blocked() && ne_ % kElemBlock)
   {
      const size_t nb = layout_.nblk();
      if (qd_diff_.size())
      {
         const size_t per = qd_diff_.size() / nb;
         ECM2_HIP(hipMemsetAsync(qd_diff_.data() + (nb - 1) * per, 0, per * sizeof(double), s));
      }
      if (qd_mass_.size())
      {
         const size_t per = qd_mass_.size() / nb;
         ECM2_HIP(hipMemsetAsync(qd_mass_.data() + (nb - 1) * per, 0, per * sizeof(double), s));
      }
   }

   // Attribute markers: per marked integrator, element weights 1 (marker[attr - 1] != 0) or 0,
   // applied to its coefficient at setup (the reference masks the integrator's E-vector output,
   // AddWithMarkers_, bilinearform_ext.cpp:753-774: the same operator)
   for (int k = 0; k < 2; k++)
   {
      CoeffDesc &c = k == INTEG_MASS ? cmass_ : cdiff_;
      c.emask = nullptr;
      if (!(k == INTEG_MASS ? have_mass_ : have_diff_)) { continue; }
      if (!marked_[k]) { continue; }
      std::vector<double> w = marker_weights(k);
      w.resize(std::max(1, ne_));
      emask_[k].upload(w, s);
      ECM2_HIP(hipStreamSynchronize(s));  // w is a host temporary
      c.emask = emask_[k].data();
   }

   // Coefficient values at quadrature points (CoefficientVector::Project).
   // (coefficient snapshot: the diffusion law is evaluated by the kernel, and with tmass 2 the mass law
   // too -- the stored per-element value is then det J times the marker weight alone)
   const bool mass_in_kernel = layout_.tsnap && layout_.tmass == 2 && cmass_.gridfunc();
   CoeffDesc cm_one = cmass_;
   cm_one.kind = COEFF_CONSTANT;
   cm_one.value = 1.0;
   const double *cm_q = have_mass_ && !mass_in_kernel ? coeff_points(cmass_, ctmp_m_, s) : nullptr;
   const double *cd_q = have_diff_ && !layout_.tsnap ? coeff_points(cdiff_, ctmp_d_, s) : nullptr;

   const CoeffDesc *cm = have_mass_ ? (mass_in_kernel ? &cm_one : &cmass_) : nullptr;
   const CoeffDesc *cd = have_diff_ ? &cdiff_ : nullptr;
   if (layout_.affine())
   {
      kern::setup_affine(layout_, Q_, jac_ ? nullptr : enodes_.data(), jac_, W_.data(), cm, cd, cm_q, cd_q,
                         qd_diff_.data(), qd_mass_.data(), s);
      cdiag_ = false;
      if ((layout_.tsnap && layout_.kind == QLAYOUT_AFFINE) || layout_.kind == QLAYOUT_AFFINE_E)
      {
         if (cdflag_.size() < 1) { cdflag_.resize(1); }
         const char *e = std::getenv("ECM2_CDIAG");  // (A/B aid: 0 keeps the general flux product)
         cdiag_ = !(e && std::string(e) == "0") && kern::affine_c_diagonal(layout_, qd_diff_.data(), cdflag_.data(), s);
      }
   }
   else if (layout_.trilinear())
   {
      kern::setup_trilinear(layout_, Q_, jac_ ? nullptr : enodes_.data(), jac_ ? cfit_.data() : nullptr, W_.data(),
                            qp_, cm, cd, cm_q, cd_q, qd_diff_.data(), qd_mass_.data(), s);
   }
   else if (jac_)
   {
      kern::setup_from_jacobians(layout_, jac_, W_.data(), cm, cd, cm_q, cd_q, qd_diff_.data(),
                                 qd_mass_.data(), s);
   }
   else
   {
      kern::setup_from_nodes(layout_, Q_, enodes_.data(), W_.data(), basis1_, cm, cd, cm_q, cd_q,
                             qd_diff_.data(), qd_mass_.data(), s);
   }
}

void PAForm::record_start(hipStream_t s)
{
   if (!timing_) { return; }
   if (ev_count_ >= ev_start_.size())
   {
      hipEvent_t a, b;
      ECM2_HIP(hipEventCreate(&a));
      ECM2_HIP(hipEventCreate(&b));
      ev_start_.push_back(a);
      ev_stop_.push_back(b);
   }
   ECM2_HIP(hipEventRecord(ev_start_[ev_count_], s));
}

void PAForm::record_stop(hipStream_t s)
{
   if (!timing_) { return; }
   ECM2_HIP(hipEventRecord(ev_stop_[ev_count_], s));
   ev_count_++;
}

void PAForm::timing_enable(bool on)
{
   timing_ = on;
   ev_count_ = 0;
}

void PAForm::timing_get(double *total_ms, long *launches)
{
   double t = 0.0;
   for (size_t i = 0; i < ev_count_; i++)
   {
      ECM2_HIP(hipEventSynchronize(ev_stop_[i]));
      float ms = 0.f;
      ECM2_HIP(hipEventElapsedTime(&ms, ev_start_[i], ev_stop_[i]));
      t += ms;
   }
   if (total_ms) { *total_ms = t; }
   if (launches) { *launches = (long)ev_count_; }
}

size_t PAForm::algorithmic_bytes() const
{
   // 8*NE*NQ*(6+1) qdata + 8*ndofs (x) + 8*ndofs (y) + 4*NE*ND (map).
   const size_t nc = (have_diff_ ? 6 : 0) + (have_mass_ ? 1 : 0);
   return 8ull * ne_ * NQ_ * nc + 16ull * n_owned_ + 4ull * ne_ * ND_;
}

void build_restriction_csr(const std::vector<int> &gmap, int ndofs, std::vector<int> &off, std::vector<int> &idx)
{
   // ElementRestriction ctor CSR build (restriction.cpp:68-106).
   off.assign(ndofs + 1, 0);
   idx.resize(gmap.size());
   for (int g : gmap) { off[(g >= 0 ? g : -1 - g) + 1]++; }
   for (int i = 1; i <= ndofs; i++) { off[i] += off[i - 1]; }
   for (size_t lid = 0; lid < gmap.size(); lid++)
   {
      const int g = gmap[lid];
      const int d = g >= 0 ? g : -1 - g;
      idx[off[d]++] = g >= 0 ? (int)lid : (int)(-1 - (long)lid);
   }
   for (int i = ndofs; i > 0; i--) { off[i] = off[i - 1]; }
   off[0] = 0;
}

void PAForm::ensure_csr()
{
   if (csr_off_.size() || ndofs_ == 0) { return; }
   std::vector<int> off, idx;
   build_restriction_csr(gmap_host_, ndofs_, off, idx);
   csr_off_.upload(off);
   csr_idx_.upload(idx);
   ECM2_HIP(hipDeviceSynchronize());
}

void PAForm::ensure_work(hipStream_t)
{
   xe_.resize((size_t)ne_ * ND_);
   ye_.resize((size_t)ne_ * ND_);
}

void PAForm::mult(const double *x, double *y, hipStream_t s)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "Mult before Assemble");
   ECM2_VERIFY(ndofs_ == 0 || (x && y), ERR_ARG, "null vector");
   if (ndofs_ == 0) { return; }
   mult_volume(x, y, s);
   // the boundary block of PABilinearFormExtension::Mult (bilinearform_ext.cpp:625-675), after the
   // volume result is complete (partial scatter: after finish_shared), whatever kernel computed it
   if (has_boundary_integrators()) { bdr_.add_mult(x, y, s); }
   // then the convection term: one apply into its E-vector and a fixed-order add (conv_term.hpp)
   if (has_convection()) { conv_.add_mult(x, y, false, s); }
}

void PAForm::mult_transpose(const double *x, double *y, hipStream_t s)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "MultTranspose before Assemble");
   ECM2_VERIFY(ndofs_ == 0 || (x && y), ERR_ARG, "null vector");
   if (ndofs_ == 0) { return; }
   // Mass, Diffusion and the boundary mass are symmetric: their transposes are the Mult, launch for launch
   mult_volume(x, y, s);
   if (has_boundary_integrators()) { bdr_.add_mult(x, y, s); }
   if (has_convection()) { conv_.add_mult(x, y, true, s); }
}

void PAForm::mult_volume(const double *x, double *y, hipStream_t s)
{
   const bool m = have_mass_, d = have_diff_;
   if (resolved_mode_ == KERNEL_UNFUSED)
   {
      // PABilinearFormExtension::MultInternal, bilinearform_ext.cpp:527-560.
      ensure_work(s);
      ensure_csr();
      record_start(s);
      kern::restriction_mult((long)ne_ * ND_, ND_, gmap_.data(), x, xe_.data(), s);
      if (ne_) { ECM2_HIP(hipMemsetAsync(ye_.data(), 0, ye_.bytes(), s)); }
      ApplyArgs a = apply_args(xe_.data(), nullptr, ye_.data(), nullptr, 0, layout_.nblk(), qdata());
      if (m) { kern::apply_wpe(D_, Q_, true, false, a, true, true, basis_, s); }
      if (d) { kern::apply_wpe(D_, Q_, false, true, a, true, true, basis_, s); }
      kern::restriction_mult_transpose(ndofs_, ND_, csr_off_.data(), csr_idx_.data(), ye_.data(), y, s);
      record_stop(s);
      return;
   }
   if (!m && !d)
   {
      ECM2_HIP(hipMemsetAsync(y, 0, sizeof(double) * (size_t)ndofs_, s));
      return;
   }
   if (use_partials())
   {
      // exclusive dofs are plain-stored, shared ones summed from their partial slots:
      // every y entry is written exactly once, no memset, bitwise reproducible
      record_start(s);
      apply_blocks(x, nullptr, y, nullptr, 0, layout_.nblk(), s);
      record_stop(s);
      finish_shared(0, n_shared(), y, nullptr, s);
      return;
   }
   ECM2_HIP(hipMemsetAsync(y, 0, sizeof(double) * (size_t)ndofs_, s));
   record_start(s);
   apply_blocks(x, nullptr, y, nullptr, 0, layout_.nblk(), s);
   record_stop(s);
}

int PAForm::energy_parts() const
{
   // the coefficient-snapshot kernel (p = 2), one partial per 4-block workgroup.  (The p >= 3 brick kernel
   // folding the same sums was measured twice and rejected: every instantiation carrying the running sum
   // slowed the plain Mult by 3%; a separate instantiation cost the PCG's Mult what the dot pass it removed
   // cost -- profiles/r6/ab_brick_energy.txt.)
   const bool ts = assembled_ && use_partials() && resolved_mode_ == KERNEL_TPE && layout_.kind == QLAYOUT_AFFINE &&
                   layout_.tsnap && have_diff_ && D_ == 3 && Q_ == 4;
   // (a boundary integrator: the folded sum would miss d^T H d of the face term, so the caller runs
   // the dot pass over the complete Mult)
   // (a convection integrator likewise: x^T C x is not in the folded sum)
   return ts && ndofs_ > 0 && !has_boundary_integrators() && !has_convection() ? (layout_.nblk() + 3) / 4 : 0;
}

void PAForm::mult_energy(const double *x, double *y, double *en, hipStream_t s)
{
   ECM2_VERIFY(energy_parts() > 0, ERR_UNSUPPORTED, "this form's Mult does not fold the energy");
   ECM2_VERIFY(x && y && en, ERR_ARG, "null vector");
   record_start(s);
   apply_blocks(x, nullptr, y, nullptr, 0, layout_.nblk(), s, false, en);
   record_stop(s);
   finish_shared(0, n_shared(), y, nullptr, s);
}

void PAForm::add_mult(const double *x, double *y, double a, hipStream_t s)
{
   ECM2_VERIFY(ndofs_ == 0 || y, ERR_ARG, "null vector");
   ywork_.resize(std::max(1, ndofs_));
   mult(x, ywork_.data(), s);
   kern::add_scaled(ndofs_, y, a, ywork_.data(), y, s);
}

void PAForm::set_scatter(int mode)
{
   ECM2_VERIFY(mode == SCATTER_PARTIALS || mode == SCATTER_ATOMIC, ERR_ARG, "unknown scatter mode " << mode);
   scatter_ = mode;
   invalidate_plans(false, true);  // the line kernel's bricks exist only with the partial scatter
   assembled_ = false;
}

void PAForm::finish_shared(int i0, int i1, double *y, double *yg, hipStream_t s) const
{
   if (!use_partials()) { return; }
   // the plan's blocks cover the owned shared dofs [0, n_sh_owned) then the ghost ones
   const SharedPlanInfo &P = shared_.info;
   ECM2_VERIFY((i0 == 0 || i0 == P.n_sh_owned) && (i1 == P.n_sh_owned || i1 == P.n_sh) && i0 <= i1, ERR_INTERNAL,
               "summation range [" << i0 << ", " << i1 << ") is not a plan range");
   const int b0 = i0 == 0 ? 0 : P.nblk_owned, b1 = i1 == P.n_sh_owned ? P.nblk_owned : P.nblk;
   kern::sum_partials(b0, b1, shared_.blocks.data(), shared_.runs.data(), shared_.rslots.data(), shared_.pdof.data(),
                      part_.data(), n_owned_, y, yg, s);
}

// What an assembly fixes of a launch: the plan's arrays and flags, the snapshot and its laws.
void PAForm::build_launch_args()
{
   targs_ = TpeArgs{};
   largs_ = LineArgs{};
   if (resolved_mode_ == KERNEL_TPE)
   {
      TpeArgs &t = targs_;
      t.lane_flags = tpe_.lane_flags.data();
      t.treg = tpe_.treg.size() ? tpe_.treg.data() : nullptr;
      t.treg_all = tpe_.info.treg_all ? 1 : 0;
      t.tlat_all = tpe_.info.tlat_all ? 1 : 0;
      t.part_stride = tpe_.info.part_stride;
      t.lmap = tpe_.lmap.size() ? tpe_.lmap.data() : nullptr;
      t.xwave = (layout_.kind == QLAYOUT_AFFINE || layout_.kind == QLAYOUT_TRILINEAR) ? 1 : 0;
      t.tsnap = layout_.tsnap ? tsnap_.data() : nullptr;
      t.tsnap_kind = layout_.tsnap;
      t.tmass = layout_.tmass;
      t.tlaw = layout_.tlaw;
      if (layout_.tsnap && layout_.tlaw)
      {
         t.law_d = point_law_of(cdiff_);
         if (layout_.tmass == 2 && cmass_.gridfunc()) { t.law_m = point_law_of(cmass_); }
      }
      for (int q = 0; q < Q_; q++) { t.qw.x[q] = maps_.qw1[q]; }
      t.bw = basis_;
      for (int d = 0; d < MAX_D1D; d++)
         for (int q = 0; q < MAX_Q1D; q++) { t.bw.B[q + MAX_Q1D * d] = t.qw.x[q] * basis_.B[q + MAX_Q1D * d]; }
   }
   else if (resolved_mode_ == KERNEL_LINE)
   {
      LineArgs &l = largs_;
      l.btab = btab();
      l.lelem = line_.lelem.data();
      l.lelem_off = line_.lelem_off.empty() ? nullptr : line_.lelem_off.data();
      if (use_partials()) { l.part_brick = part_.data(); }
      if (line_.info.brick_bz)
      {
         l.brick_bz = line_.info.brick_bz;
         l.belem = line_.belem.data();
         l.bmap = line_.bmap.data();
         l.brick_off = line_.brick_off.data();
         l.breg = line_.breg.size() ? line_.breg.data() : nullptr;
      }
   }
}

ApplyArgs PAForm::apply_args(const double *x, const double *xg, double *y, double *yg, int b0, int b1, QData q) const
{
   ApplyArgs a;
   a.kind = layout_.kind;
   a.pw = layout_.pw;
   a.ne = ne_;
   a.blk_begin = b0;
   a.blk_end = b1;
   a.n_owned = n_owned_;
   a.pos = layout_.pos;
   a.gmap = (resolved_mode_ == KERNEL_TPE) ? tpe_.gmap_blk.data()
            : (resolved_mode_ == KERNEL_LINE) ? line_.gmap_line.data() : gmap_.data();
   a.qdd = q.diff;
   a.qdm = q.mass;
   a.x = x; a.xg = xg; a.y = y; a.yg = yg;
   // LINE: the leftover elements' [e][nd] slots follow the bricks'
   if (use_partials()) { a.part = part_.data() + (resolved_mode_ == KERNEL_LINE ? line_.info.part_line_off : 0); }
   a.qp = qp_;
   a.cdiag = cdiag_ && (layout_.tsnap || layout_.kind == QLAYOUT_AFFINE_E) ? 1 : 0;
   return a;
}

void PAForm::apply_blocks(const double *x, const double *xg, double *y, double *yg, int b0, int b1,
                          hipStream_t s, bool latency, double *en)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "apply before Assemble");
   ECM2_VERIFY(resolved_mode_ != KERNEL_UNFUSED, ERR_UNSUPPORTED, "block apply needs a fused kernel");
   if (resolved_mode_ == KERNEL_LINE && line_.info.brick_bz)
   {
      auto boundary = [&](int b) {
         return b == 0 || b == layout_.nblk() || std::find(splits_.begin(), splits_.end(), b) != splits_.end();
      };
      ECM2_VERIFY(boundary(b0) && boundary(b1), ERR_ARG, "apply_blocks [" << b0 << ", " << b1
                                                          << ") cuts a brick: declare the split with set_block_splits");
   }
   ApplyArgs a = apply_args(x, xg, y, yg, b0, b1, qdata());
   a.latency = latency && layout_.kind == QLAYOUT_AFFINE && have_mass_ && have_diff_ && !layout_.tsnap;
   a.en = en;  // (mult_energy: the snapshot kernel only)
   if (resolved_mode_ == KERNEL_TPE)
   {
      kern::apply_tpe(D_, Q_, have_mass_, have_diff_, a, targs_, basis_, rowtab_.data(), s);
   }
   else if (resolved_mode_ == KERNEL_LINE)
   {
      kern::apply_line(D_, Q_, have_mass_, have_diff_, a, largs_, s);
   }
   else
   {
      kern::apply_wpe(D_, Q_, have_mass_, have_diff_, a, false, false, basis_, s);
   }
}

void PAForm::assemble_diagonal(double *diag, hipStream_t s)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "AssembleDiagonal before Assemble");
   // ConvectionIntegrator::AssembleDiagonalPA aborts (bilininteg_convection_pa.cpp:216-227); a term whose
   // marker keeps no element contributes nothing and is let through
   ECM2_VERIFY(!(has_convection() && conv_.n_active() > 0), ERR_UNSUPPORTED,
               "AssembleDiagonal is not implemented for a form with a ConvectionIntegrator (so neither is a "
               "Jacobi-preconditioned solve on it): keep the convection out of the implicit operator");
   if (ndofs_ == 0) { return; }
   // The diagonal is a function of the assembled state alone (every setter clears assembled_, and
   // Assemble bumps gen_): repeated requests between two Assembles -- a Jacobi smoother per PCG
   // solve, three SDIRK stages on one T -- copy the first result instead of recomputing it (at C4
   // with the snapshot: ~3 ms of expansion and diagonal kernels against a 25 us copy).
   if (diag_gen_ == gen_ && diag_cache_.size() == (size_t)ndofs_)
   {
      ECM2_HIP(hipMemcpyAsync(diag, diag_cache_.data(), diag_cache_.bytes(), hipMemcpyDeviceToDevice, s));
      return;
   }
   assemble_diagonal_uncached(diag, s);
   // the boundary block (bilinearform_ext.cpp:441-452), added to the complete volume diagonal
   if (has_boundary_integrators()) { bdr_.add_diagonal(diag, s); }
   diag_cache_.resize(ndofs_);
   ECM2_HIP(hipMemcpyAsync(diag_cache_.data(), diag, diag_cache_.bytes(), hipMemcpyDeviceToDevice, s));
   diag_gen_ = gen_;
}

void PAForm::assemble_diagonal_uncached(double *diag, hipStream_t s) const
{
   // The reference's AssembleDiagonal (bilinearform_ext.cpp:370-411) adds every integrator's
   // AssembleDiagonalPA into ONE localY and then zeroes a marked integrator's excluded elements of
   // that localY, so on those elements the contributions of the integrators added before it vanish
   // too (Mult masks each integrator's output separately, AddMultWithMarkers :753-774).  This
   // library reproduces it: when the second integrator added (S) is marked and excludes elements
   // the first (F) acts on, the diagonal is taken from a copy of the stored (Assemble-time) qdata
   // with F's entries multiplied by S's element weights (diag_w_, set at Assemble); the form's own
   // qdata is only read.
   if (diag_integ_ < 0)
   {
      diagonal_from_qdata(diag, qdata(), s);
      return;
   }
   DeviceArray<double> td, tm;
   td.resize(qd_diff_.size());
   tm.resize(qd_mass_.size());
   if (td.size()) { ECM2_HIP(hipMemcpyAsync(td.data(), qd_diff_.data(), td.bytes(), hipMemcpyDeviceToDevice, s)); }
   if (tm.size()) { ECM2_HIP(hipMemcpyAsync(tm.data(), qd_mass_.data(), tm.bytes(), hipMemcpyDeviceToDevice, s)); }
   kern::scale_elements(layout_, diag_integ_, diag_w_.data(), td.data(), tm.data(), s);
   diagonal_from_qdata(diag, {td.data(), tm.data()}, s);
   ECM2_HIP(hipStreamSynchronize(s));  // the temporaries are freed on return
}

void PAForm::diagonal_from_qdata(double *diag, QData q, hipStream_t s) const
{
   if (resolved_mode_ == KERNEL_TPE && (have_mass_ || have_diff_))
   {
      // thread-per-element diagonal assembled like the Mult (deterministic with partials)
      double *dg = n_owned_ < ndofs_ ? diag + n_owned_ : nullptr;
      if (!use_partials()) { ECM2_HIP(hipMemsetAsync(diag, 0, sizeof(double) * (size_t)ndofs_, s)); }
      ApplyArgs a = apply_args(nullptr, nullptr, diag, dg, 0, layout_.nblk(), q);
      DeviceArray<double> fd, fm;
      if (expand_needed())
      {
         expand_compressed(q, fd, fm, s);  // per-point qdata for the diagonal's tables
         a.kind = expand_kind();
         a.qdd = fd.data();
         a.qdm = fm.data();
      }
      kern::diagonal_tpe(D_, Q_, have_mass_, have_diff_, a, targs_, basis_, drowtab_.data(), s);
      finish_shared(0, n_shared(), diag, dg, s);
      if (fd.size()) { ECM2_HIP(hipStreamSynchronize(s)); }  // the temporaries are freed on return
      return;
   }
   ECM2_HIP(hipMemsetAsync(diag, 0, sizeof(double) * (size_t)ndofs_, s));
   DeviceArray<double> fd, fm;
   int kind = layout_.kind;
   const double *qdd = q.diff, *qdm = q.mass;
   if (expand_needed())
   {
      expand_compressed(q, fd, fm, s);
      kind = expand_kind();
      qdd = fd.data();
      qdm = fm.data();
   }
   kern::diagonal(layout_.pos, D_, Q_, kind, ne_, gmap_.data(), have_diff_ ? qdd : nullptr,
                  have_mass_ ? qdm : nullptr, diag, false, basis_, btab(), s);
   if (fd.size()) { ECM2_HIP(hipStreamSynchronize(s)); }  // the temporaries are freed on return
}

void PAForm::expand_compressed(QData q, DeviceArray<double> &fd, DeviceArray<double> &fm, hipStream_t s) const
{
   QLayout L = layout_;
   L.kind = expand_kind();
   fd.resize(std::max<size_t>(1, have_diff_ ? L.diff_size() : 0));
   fm.resize(std::max<size_t>(1, have_mass_ ? L.mass_size() : 0));
   if (L.blocked() && ne_ % kElemBlock)
   {
      ECM2_HIP(hipMemsetAsync(fd.data(), 0, fd.bytes(), s));
      ECM2_HIP(hipMemsetAsync(fm.data(), 0, fm.bytes(), s));
   }
   if (layout_.tsnap)
   {
      // beta (and a mass law of the same field) at the points from the snapshot -- the field as
      // Assemble saw it, projected as the reference's setup projects a GridFunctionCoefficient and the
      // law applied at the point -- times the STORED element matrices and mass values (which the
      // marker diagonal may have scaled, assemble_diagonal)
      DeviceArray<double> tdof, ctd, ctm;
      const double *tv = tsnap_.data();
      if (layout_.tsnap == 2)
      {
         tdof.resize(std::max(1, ndofs_));
         kern::lattice_to_dofs(layout_.nblk(), tpe_lattice_points(D_), tpe_.lmap.data(), tsnap_.data(), tdof.data(), s);
         tv = tdof.data();
      }
      CoeffDesc cs = cdiff_;
      cs.kind = layout_.tlaw ? cdiff_.kind : COEFF_GRIDFUNC;  // (tlaw 0: the law is in the snapshot)
      cs.lvec = tv;
      cs.emask = nullptr;
      const double *cd_q = coeff_points(cs, ctd, s);
      const double *cm_q = nullptr;
      if (layout_.tmass == 2 && cmass_.gridfunc())
      {
         CoeffDesc cm = cmass_;
         cm.lvec = tv;  // tlaw 1: the snapshot is the field itself
         cm.emask = nullptr;
         cm_q = coeff_points(cm, ctm, s);
      }
      kern::tsnap_expand(layout_, Q_, W_.data(), q.diff, q.mass, cd_q, cm_q, fd.data(),
                         fm.data(), s);
      ECM2_HIP(hipStreamSynchronize(s));  // the temporaries are freed on return
      return;
   }
   if (layout_.trilinear())
   {
      kern::trilinear_expand(layout_, Q_, q.diff, q.mass, qp_, fd.data(), fm.data(), s);
   }
   else { kern::affine_expand(layout_, Q_, q.diff, q.mass, fd.data(), fm.data(), s); }
}

void PAForm::restriction_mult(const double *x, double *xe, hipStream_t s)
{
   kern::restriction_mult((long)ne_ * ND_, ND_, gmap_.data(), x, xe, s);
}

void PAForm::restriction_mult_transpose(const double *xe, double *y, hipStream_t s)
{
   ensure_csr();
   kern::restriction_mult_transpose(ndofs_, ND_, csr_off_.data(), csr_idx_.data(), xe, y, s);
}

void PAForm::integrator_add_mult(int kind, const double *xe, double *ye, hipStream_t s, bool transpose)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "AddMultPA before Assemble");
   if (kind == INTEG_CONVECTION)
   {
      ECM2_VERIFY(has_convection(), ERR_ARG, "integrator " << kind << " not present");
      conv_.add_mult_evec(xe, ye, transpose, s);
      return;
   }
   ECM2_VERIFY((kind == INTEG_MASS && have_mass_) || (kind == INTEG_DIFFUSION && have_diff_),
               ERR_ARG, "integrator " << kind << " not present");
   ApplyArgs a = apply_args(xe, nullptr, ye, nullptr, 0, layout_.nblk(), qdata());
   a.gmap = gmap_.data();
   DeviceArray<double> fd, fm;
   if (expand_needed())
   {
      expand_compressed(qdata(), fd, fm, s);
      a.kind = expand_kind();
      a.qdd = fd.data();
      a.qdm = fm.data();
   }
   kern::apply_wpe(D_, Q_, kind == INTEG_MASS, kind == INTEG_DIFFUSION, a, true, true, basis_, s);
   if (fd.size()) { ECM2_HIP(hipStreamSynchronize(s)); }
}

void PAForm::get_qdata(int kind, double *out, hipStream_t s)
{
   ECM2_VERIFY(assembled_, ERR_STATE, "get_qdata before Assemble");
   if (kind == INTEG_CONVECTION)
   {
      ECM2_VERIFY(has_convection(), ERR_ARG, "integrator " << kind << " not present");
      conv_.get_qdata(out, s);  // [ne][3][nq], zeros on the elements its marker excludes
      return;
   }
   const bool diff = kind == INTEG_DIFFUSION;
   ECM2_VERIFY(diff ? have_diff_ : have_mass_, ERR_ARG, "integrator " << kind << " not present");
   DeviceArray<double> fd, fm;
   const bool tl = expand_needed();  // TRILINEAR(_E), or a diffusion-only AFFINE(_E) form
   const bool aff = layout_.affine() && !tl;
   if (tl) { expand_compressed(qdata(), fd, fm, s); }  // decoded as expand_kind() below
   const int kind_h = tl ? expand_kind() : layout_.kind;
   DeviceArray<double> &src = tl ? (diff ? fd : fm) : ((diff && !aff) ? qd_diff_ : qd_mass_);
   std::vector<double> h(src.size()), hc(aff ? qd_diff_.size() : 0);
   if (src.size())
   {
      ECM2_HIP(hipMemcpyAsync(h.data(), src.data(), src.bytes(), hipMemcpyDeviceToHost, s));
   }
   if (hc.size())
   {
      ECM2_HIP(hipMemcpyAsync(hc.data(), qd_diff_.data(), qd_diff_.bytes(), hipMemcpyDeviceToHost, s));
   }
   ECM2_HIP(hipStreamSynchronize(s));
   const int nc = diff ? (layout_.kind == QLAYOUT_NATIVE9 ? 9 : 6) : 1;
   // (blocked layouts: the TPE plan's element order)
   std::vector<int> invp(layout_.blocked() ? ne_ : 0);
   for (size_t i = 0; i < invp.size(); i++) { invp[tpe_.perm[i]] = (int)i; }
   for (int e = 0; e < ne_; e++)
      for (int c = 0; c < nc; c++)
         for (int q = 0; q < NQ_; q++)
         {
            size_t src_i;
            if (kind_h == QLAYOUT_NATIVE || kind_h == QLAYOUT_NATIVE9) { src_i = ((size_t)e * nc + c) * NQ_ + q; }
            else if (kind_h == QLAYOUT_AFFINE_E)
            {
               const size_t pi = ((size_t)e * NQ_ + q) * 2;
               out[((size_t)e * nc + c) * NQ_ + q] = diff ? h[pi] * hc[(size_t)e * 6 + c] : h[pi + 1];
               continue;
            }
            else
            {
               const int ip = invp[e];
               const int blk = ip / 64, lane = ip % 64;
               if (aff)
               {
                  // AFFINE: D_c(q) = (W beta)(q) * C_c, mass = the pair's second entry
                  const size_t pi = (((size_t)blk * NQ_ + q) * 64 + lane) * 2;
                  out[((size_t)e * nc + c) * NQ_ + q] =
                     diff ? h[pi] * hc[(((size_t)blk * 3 + c / 2) * 64 + lane) * 2 + (c & 1)] : h[pi + 1];
                  continue;
               }
               if (diff) { src_i = (((size_t)blk * NQ_ + q) * 3 + c / 2) * 128 + lane * 2 + (c & 1); }
               else { src_i = ((size_t)blk * ((NQ_ + 1) / 2) + q / 2) * 128 + lane * 2 + (q & 1); }
            }
            out[((size_t)e * nc + c) * NQ_ + q] = h[src_i];
         }
}

// --------------------------------------------------------------------------
// Device PCG
// --------------------------------------------------------------------------

} // namespace ecm2
