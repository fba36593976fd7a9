// mg_potential.cpp -- rf_potential.cpp's problem -div(sigma grad phi) = f at p = 4 through the C ABI alone
// (include/ecm2_pa.h), solved three times: Jacobi-PCG, the PCG preconditioned by OperatorChebyshevSmoother (order
// 2), and the PCG preconditioned by a p-multigrid V-cycle over the orders 1 -> 2 -> 4 with the settings of the
// reference's examples/ex26.cpp: a GeometricMultigrid over PA forms, OperatorChebyshevSmoother(order 2) on every
// level, a Jacobi-CG coarse solve (rel_tol sqrt(1e-4), 200 iterations), TensorProductPRefinementTransferOperator
// between the levels (fem/transfer.cpp:2223-2592), the cycle (fem/multigrid.cpp:106-232) as CGSolver's preconditioner.
//
// Unit cube, n^3 elements, sigma = 1 + x at every level's quadrature points, phi = 0 on the boundary; manufactured
// phi = sin(pi x) sin(pi y) sin(pi z), f interpolated at the p = 4 dofs and assembled by the device linear form.
// Exit status 0 when the three solves converge to 1e-12, the solutions agree to 1e-9 of max|phi|, each meets the
// manufactured one to rf_potential's 6e-5, and V-cycle < Chebyshev < Jacobi in iterations.
//
// Usage: mg_potential [n = 8]
#include "ecm2_pa.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                       \
   do {                                                                                   \
      const int rc_ = (call);                                                             \
      if (rc_ != ECM2_OK)                                                                 \
      {                                                                                   \
         std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ecm2_last_error());     \
         std::exit(2);                                                                    \
      }                                                                                   \
   } while (0)
#define HIPCHECK(call)                                                                    \
   do {                                                                                   \
      if ((call) != hipSuccess) { std::fprintf(stderr, "%s failed\n", #call); std::exit(2); } \
   } while (0)

template <typename T>
static T *device_copy(const std::vector<T> &h)
{
   T *d = nullptr;
   HIPCHECK(hipMalloc(&d, std::max<size_t>(1, h.size()) * sizeof(T)));
   if (!h.empty()) { HIPCHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
   return d;
}

static std::vector<double> host_copy(const double *d, int n)
{
   std::vector<double> h(n);
   HIPCHECK(hipMemcpy(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost));
   return h;
}

// one level of the hierarchy: the space's host data, then the device form, operator and smoother
struct Level
{
   int order = 0, ndofs = 0, ne = 0, nd = 0, n_ess = 0;
   ecm2_h1space *fes = nullptr;
   std::vector<int> gmap, ess;
   std::vector<double> sigma;
   ecm2_pa_form *form = nullptr;
   ecm2_operator *A = nullptr;
   ecm2_smoother *sm = nullptr;
   double *sigma_d = nullptr;
   int *ess_d = nullptr;
};

int main(int argc, char **argv)
{
   const int n = argc > 1 ? std::atoi(argv[1]) : 8;
   const int orders[3] = {1, 2, 4};
   const double pi = M_PI, rel_tol = 1e-12;

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(n, n, n, 1.0, 1.0, 1.0, &mesh));
   int ne = 0;
   std::vector<double> enodes;
   Level lv[3];
   for (int k = 0; k < 3; k++)
   {
      Level &l = lv[k];
      l.order = orders[k];
      CHECK(ecm2_h1space_create(mesh, l.order, ECM2_NUMBERING_ENTITY, &l.fes));
      CHECK(ecm2_h1space_info(l.fes, &l.ndofs, &l.ne, &l.nd));
      ne = l.ne;
      l.gmap.resize((size_t)l.ne * l.nd);
      CHECK(ecm2_h1space_get_gather_map(l.fes, l.gmap.data()));
      CHECK(ecm2_h1space_boundary_dofs(l.fes, nullptr, &l.n_ess));
      l.ess.resize(l.n_ess);
      CHECK(ecm2_h1space_boundary_dofs(l.fes, l.ess.data(), &l.n_ess));
      // sigma = 1 + x at the level's quadrature points (the default rule, order + 2 points per direction)
      const int q1d = l.order + 2, nq = q1d * q1d * q1d;
      std::vector<double> P((size_t)l.ne * nq * 3);
      CHECK(ecm2_mesh_quadrature_points(mesh, q1d, P.data()));
      l.sigma.resize((size_t)l.ne * nq);
      for (size_t i = 0; i < l.sigma.size(); i++) { l.sigma[i] = 1.0 + P[3 * i]; }
   }
   enodes.resize((size_t)ne * 24);
   CHECK(ecm2_mesh_get_element_nodes(mesh, enodes.data()));
   Level &fine = lv[2];
   const int ndofs = fine.ndofs;
   std::vector<double> X((size_t)ndofs * 3), phi(ndofs), f(ndofs);
   CHECK(ecm2_h1space_dof_coords(fine.fes, mesh, X.data()));
   for (int i = 0; i < ndofs; i++)
   {
      const double x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
      phi[i] = std::sin(pi * x) * std::sin(pi * y) * std::sin(pi * z);
      f[i] = 3.0 * pi * pi * (1.0 + x) * phi[i] - pi * std::cos(pi * x) * std::sin(pi * y) * std::sin(pi * z);
   }
   std::printf("unit cube %d^3 elements, H1 p = 1 -> 2 -> 4, %d -> %d -> %d dofs, %d essential on the finest; sigma = 1 + x\n",
               n, lv[0].ndofs, lv[1].ndofs, lv[2].ndofs, fine.n_ess);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   for (int k = 0; k < 3; k++)
   {
      Level &l = lv[k];
      CHECK(ecm2_pa_form_create(l.ne, l.order, l.ndofs, l.gmap.data(), 0, &l.form));
      CHECK(ecm2_pa_form_set_element_nodes(l.form, enodes.data()));
      l.sigma_d = device_copy(l.sigma);
      CHECK(ecm2_pa_form_add_integrator(l.form, ECM2_DIFFUSION, ECM2_COEFF_QUAD, l.sigma_d, nullptr));
      CHECK(ecm2_pa_form_assemble(l.form, nullptr));
      CHECK(ecm2_operator_from_pa_form(l.form, &l.A));
      l.ess_d = device_copy(l.ess);
      // OperatorChebyshevSmoother(order 2) with the power method's defaults (10 steps, 1e-8), as ex26
      CHECK(ecm2_chebyshev_create_power(l.A, nullptr, l.ess_d, l.n_ess, 2, 10, 1e-8, nullptr, &l.sm, nullptr));
   }
   ecm2_transfer *tr[2] = {nullptr, nullptr};
   for (int k = 0; k < 2; k++)
   {
      CHECK(ecm2_transfer_create(ne, lv[k].order, lv[k].ndofs, lv[k].gmap.data(), lv[k + 1].order, lv[k + 1].ndofs,
                                 lv[k + 1].gmap.data(), &tr[k]));
   }
   ecm2_operator *ops[3] = {lv[0].A, lv[1].A, lv[2].A};
   ecm2_smoother *sms[3] = {lv[0].sm, lv[1].sm, lv[2].sm};
   const int *essp[3] = {lv[0].ess_d, lv[1].ess_d, lv[2].ess_d};
   const int n_ess[3] = {lv[0].n_ess, lv[1].n_ess, lv[2].n_ess};
   ecm2_multigrid *mg = nullptr;
   CHECK(ecm2_multigrid_create(3, ops, sms, tr, essp, n_ess, 1, 1, &mg));
   CHECK(ecm2_multigrid_set_coarse_pcg(mg, std::sqrt(1e-4), 200));

   // b = (f_h, v) by the device linear form, its essential rows zeroed (phi = 0 there)
   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(ne, fine.order, ndofs, fine.gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, enodes.data()));
   double *f_d = device_copy(f);
   CHECK(ecm2_linear_form_add_domain_integrator(lf, ECM2_COEFF_GRIDFUNC, f_d, nullptr, nullptr, nullptr, 0));
   double *b = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_linear_form_assemble(lf, b, nullptr));
   HIPCHECK(hipDeviceSynchronize());
   std::vector<double> bh = host_copy(b, ndofs);
   for (int i : fine.ess) { bh[i] = 0.0; }
   HIPCHECK(hipMemcpy(b, bh.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));

   double *x[3];
   int it[3] = {0, 0, 0}, conv[3] = {0, 0, 0};
   double nrm[3] = {0, 0, 0};
   for (int k = 0; k < 3; k++) { x[k] = device_copy(std::vector<double>(ndofs, 0.0)); }
   CHECK(ecm2_operator_pcg(fine.A, fine.ess_d, fine.n_ess, b, x[0], rel_tol, 0.0, 2000, 1, &it[0], &nrm[0], nullptr));
   conv[0] = ecm2_pcg_last_converged();
   CHECK(ecm2_operator_pcg_prec(fine.A, fine.sm, fine.ess_d, fine.n_ess, b, x[1], rel_tol, 0.0, 2000, &it[1], &nrm[1], nullptr));
   conv[1] = ecm2_pcg_last_converged();
   CHECK(ecm2_operator_pcg_mg(fine.A, mg, fine.ess_d, fine.n_ess, b, x[2], rel_tol, 0.0, 2000, &it[2], &nrm[2], nullptr));
   conv[2] = ecm2_pcg_last_converged();
   std::printf("Jacobi-PCG iterations: %d (converged %d)\n", it[0], conv[0]);
   std::printf("Chebyshev-PCG iterations: %d (converged %d)\n", it[1], conv[1]);
   std::printf("V-cycle-PCG iterations: %d (converged %d)\n", it[2], conv[2]);

   std::vector<double> h[3] = {host_copy(x[0], ndofs), host_copy(x[1], ndofs), host_copy(x[2], ndofs)};
   double gap = 0.0, err[3] = {0, 0, 0}, top = 0.0;
   for (int i = 0; i < ndofs; i++)
   {
      gap = std::max({gap, std::fabs(h[0][i] - h[1][i]), std::fabs(h[0][i] - h[2][i])});
      for (int k = 0; k < 3; k++) { err[k] = std::max(err[k], std::fabs(h[k][i] - phi[i])); }
      top = std::max(top, std::fabs(h[0][i]));
   }
   std::printf("largest gap between the solutions / max|phi| = %.3e, max|phi_h - phi| = %.3e, %.3e, %.3e\n", gap / top,
               err[0], err[1], err[2]);
   const bool pass = conv[0] && conv[1] && conv[2] && gap <= 1e-9 * top && err[0] <= 6e-5 && err[1] <= 6e-5 &&
                     err[2] <= 6e-5 && it[2] < it[1] && it[1] < it[0];
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_multigrid_destroy(mg);
   for (int k = 0; k < 2; k++) { ecm2_transfer_destroy(tr[k]); }
   ecm2_linear_form_destroy(lf);
   for (int k = 0; k < 3; k++)
   {
      ecm2_smoother_destroy(lv[k].sm);
      ecm2_operator_destroy(lv[k].A);
      ecm2_pa_form_destroy(lv[k].form);
      (void)hipFree(lv[k].sigma_d);
      (void)hipFree(lv[k].ess_d);
      (void)hipFree(x[k]);
      ecm2_h1space_destroy(lv[k].fes);
   }
   (void)hipFree(b);
   (void)hipFree(f_d);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
