// hmg_potential.cpp -- mg_potential.cpp's problem -div(sigma grad phi) = f at p = 2 on a Cartesian mesh refined
// twice, through the C ABI alone (include/ecm2_pa.h), solved three times: Jacobi-PCG; the PCG preconditioned by the
// p-only V-cycle 1 -> 2 on the finest mesh; and the PCG preconditioned by the V-cycle over
// (h0, 1) -> (h1, 1) -> (h2, 1) -> (h2, 2): FiniteElementSpace::RefinementOperator (fem/fespace.cpp:1833-2120, what
// TransferOperator selects between two meshes, fem/transfer.cpp:2055-) below
// TensorProductPRefinementTransferOperator (fem/transfer.cpp:2223-2592), the hierarchy a GeometricMultigrid builds
// from a mesh refined with Mesh::UniformRefinement and then raised in order (examples/ex26.cpp with geometric
// levels).  OperatorChebyshevSmoother(order 2) on every level; every coarsest level is its smoother applied once, so
// no solve synchronises inside a cycle.
//
// Unit cube, n^3 elements on h0 (64 n^3 on h2), sigma = 1 + x at every level's quadrature points, phi = 0 on the
// boundary; manufactured phi = sin(pi x) sin(pi y) sin(pi z), f interpolated at the p = 2 dofs of h2 and assembled
// by the device linear form.  Exit status 0 when the three solves converge to 1e-12, the solutions agree to 1e-9 of
// max|phi|, each meets the manufactured one to 1e-5 (4 / n)^3 (the discretisation error is 3.2e-6 at n = 4 and of
// third order), and h+p V-cycle < p V-cycle < Jacobi in iterations (the numpy restatement of the reference takes
// 8, 13 and 49 at n = 4).
//
// Usage: hmg_potential [n = 4]
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

// one level of the hierarchy: its mesh and order, the space's host data, then the device form, operator and smoother
struct Level
{
   ecm2_mesh *mesh = nullptr;
   int order = 0, ndofs = 0, ne = 0, nd = 0, n_ess = 0;
   ecm2_h1space *fes = nullptr;
   std::vector<int> gmap, ess;
   std::vector<double> sigma, enodes;
   ecm2_pa_form *form = nullptr;
   ecm2_operator *A = nullptr;
   ecm2_smoother *sm = nullptr;
   double *sigma_d = nullptr;
   int *ess_d = nullptr;
};

int main(int argc, char **argv)
{
   const int n = argc > 1 ? std::atoi(argv[1]) : 4;
   const int L = 4, orders[L] = {1, 1, 1, 2};
   const double pi = M_PI, rel_tol = 1e-12;

   // h0, and a copy refined once per h-level: the hierarchy keeps every mesh
   ecm2_mesh *mesh[3] = {nullptr, nullptr, nullptr};
   CHECK(ecm2_mesh_cartesian(n, n, n, 1.0, 1.0, 1.0, &mesh[0]));
   for (int k = 1; k < 3; k++)
   {
      CHECK(ecm2_mesh_copy(mesh[k - 1], &mesh[k]));
      CHECK(ecm2_mesh_refine_uniform(mesh[k]));
   }
   Level lv[L];
   for (int k = 0; k < L; k++)
   {
      Level &l = lv[k];
      l.mesh = mesh[std::min(k, 2)];
      l.order = orders[k];
      CHECK(ecm2_h1space_create(l.mesh, l.order, ECM2_NUMBERING_ENTITY, &l.fes));
      CHECK(ecm2_h1space_info(l.fes, &l.ndofs, &l.ne, &l.nd));
      l.gmap.resize((size_t)l.ne * l.nd);
      CHECK(ecm2_h1space_get_gather_map(l.fes, l.gmap.data()));
      CHECK(ecm2_h1space_boundary_dofs(l.fes, nullptr, &l.n_ess));
      l.ess.resize(l.n_ess);
      CHECK(ecm2_h1space_boundary_dofs(l.fes, l.ess.data(), &l.n_ess));
      // sigma = 1 + x at the level's quadrature points (the default rule, order + 2 points per direction)
      const int q1d = l.order + 2, nq = q1d * q1d * q1d;
      std::vector<double> P((size_t)l.ne * nq * 3);
      CHECK(ecm2_mesh_quadrature_points(l.mesh, q1d, P.data()));
      l.sigma.resize((size_t)l.ne * nq);
      for (size_t i = 0; i < l.sigma.size(); i++) { l.sigma[i] = 1.0 + P[3 * i]; }
      l.enodes.resize((size_t)l.ne * 24);
      CHECK(ecm2_mesh_get_element_nodes(l.mesh, l.enodes.data()));
   }
   Level &fine = lv[L - 1];
   const int ndofs = fine.ndofs;
   std::vector<double> X((size_t)ndofs * 3), phi(ndofs), f(ndofs);
   CHECK(ecm2_h1space_dof_coords(fine.fes, fine.mesh, X.data()));
   for (int i = 0; i < ndofs; i++)
   {
      const double x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
      phi[i] = std::sin(pi * x) * std::sin(pi * y) * std::sin(pi * z);
      f[i] = 3.0 * pi * pi * (1.0 + x) * phi[i] - pi * std::cos(pi * x) * std::sin(pi * y) * std::sin(pi * z);
   }
   std::printf("unit cube %d^3 -> %d^3 -> %d^3 elements, H1 (h0, 1) -> (h1, 1) -> (h2, 1) -> (h2, 2), %d -> %d -> %d -> %d dofs, "
               "%d essential on the finest; sigma = 1 + x\n",
               n, 2 * n, 4 * n, lv[0].ndofs, lv[1].ndofs, lv[2].ndofs, lv[3].ndofs, fine.n_ess);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   for (int k = 0; k < L; k++)
   {
      Level &l = lv[k];
      CHECK(ecm2_pa_form_create(l.ne, l.order, l.ndofs, l.gmap.data(), 0, &l.form));
      CHECK(ecm2_pa_form_set_element_nodes(l.form, l.enodes.data()));
      l.sigma_d = device_copy(l.sigma);
      CHECK(ecm2_pa_form_add_integrator(l.form, ECM2_DIFFUSION, ECM2_COEFF_QUAD, l.sigma_d, nullptr));
      CHECK(ecm2_pa_form_assemble(l.form, nullptr));
      CHECK(ecm2_operator_from_pa_form(l.form, &l.A));
      l.ess_d = device_copy(l.ess);
      // OperatorChebyshevSmoother(order 2) with the power method's defaults (10 steps, 1e-8), as ex26
      CHECK(ecm2_chebyshev_create_power(l.A, nullptr, l.ess_d, l.n_ess, 2, 10, 1e-8, nullptr, &l.sm, nullptr));
   }
   // the transfers: two between a mesh and its refinement at p = 1, then 1 -> 2 on the finest mesh
   ecm2_transfer *tr[L - 1] = {nullptr, nullptr, nullptr};
   for (int k = 0; k < 2; k++)
   {
      std::vector<int> parent(lv[k + 1].ne), octant(lv[k + 1].ne);
      CHECK(ecm2_mesh_refinement_embedding(mesh[k], parent.data(), octant.data()));
      CHECK(ecm2_transfer_create_h(1, lv[k].ne, lv[k].ndofs, lv[k].gmap.data(), lv[k + 1].ne, lv[k + 1].ndofs,
                                   lv[k + 1].gmap.data(), parent.data(), octant.data(), &tr[k]));
   }
   CHECK(ecm2_transfer_create(fine.ne, 1, lv[2].ndofs, lv[2].gmap.data(), 2, fine.ndofs, fine.gmap.data(), &tr[2]));
   ecm2_operator *ops[L];
   ecm2_smoother *sms[L];
   const int *essp[L];
   int n_ess[L];
   for (int k = 0; k < L; k++) { ops[k] = lv[k].A; sms[k] = lv[k].sm; essp[k] = lv[k].ess_d; n_ess[k] = lv[k].n_ess; }
   // (every coarsest level is its smoother applied once: no ecm2_multigrid_set_coarse_pcg)
   ecm2_multigrid *mg_hp = nullptr, *mg_p = nullptr;
   CHECK(ecm2_multigrid_create(L, ops, sms, tr, essp, n_ess, 1, 1, &mg_hp));
   CHECK(ecm2_multigrid_create(2, ops + 2, sms + 2, tr + 2, essp + 2, n_ess + 2, 1, 1, &mg_p));

   // b = (f_h, v) by the device linear form, its essential rows zeroed (phi = 0 there)
   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(fine.ne, fine.order, ndofs, fine.gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, fine.enodes.data()));
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
   CHECK(ecm2_operator_pcg_mg(fine.A, mg_p, fine.ess_d, fine.n_ess, b, x[1], rel_tol, 0.0, 2000, &it[1], &nrm[1], nullptr));
   conv[1] = ecm2_pcg_last_converged();
   CHECK(ecm2_operator_pcg_mg(fine.A, mg_hp, fine.ess_d, fine.n_ess, b, x[2], rel_tol, 0.0, 2000, &it[2], &nrm[2], nullptr));
   conv[2] = ecm2_pcg_last_converged();
   std::printf("Jacobi-PCG iterations: %d (converged %d)\n", it[0], conv[0]);
   std::printf("p V-cycle-PCG iterations: %d (converged %d)\n", it[1], conv[1]);
   std::printf("h+p V-cycle-PCG iterations: %d (converged %d)\n", it[2], conv[2]);

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
   const double bound = 1e-5 * std::pow(4.0 / n, 3);
   const bool pass = conv[0] && conv[1] && conv[2] && gap <= 1e-9 * top && err[0] <= bound && err[1] <= bound &&
                     err[2] <= bound && it[2] < it[1] && it[1] < it[0];
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_multigrid_destroy(mg_hp);
   ecm2_multigrid_destroy(mg_p);
   for (int k = 0; k < L - 1; k++) { ecm2_transfer_destroy(tr[k]); }
   ecm2_linear_form_destroy(lf);
   for (int k = 0; k < L; k++)
   {
      ecm2_smoother_destroy(lv[k].sm);
      ecm2_operator_destroy(lv[k].A);
      ecm2_pa_form_destroy(lv[k].form);
      (void)hipFree(lv[k].sigma_d);
      (void)hipFree(lv[k].ess_d);
      ecm2_h1space_destroy(lv[k].fes);
   }
   for (int k = 0; k < 3; k++) { (void)hipFree(x[k]); ecm2_mesh_destroy(mesh[k]); }
   (void)hipFree(b);
   (void)hipFree(f_d);
   return pass ? 0 : 1;
}
