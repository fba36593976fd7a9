// rf_potential.cpp -- the RF potential problem -div(sigma grad phi) = f through the C ABI alone
// (include/ecm2_pa.h): a diffusion-only form with no mass to bound its condition number, solved once with
// Jacobi-PCG and once with the PCG preconditioned by OperatorChebyshevSmoother (linalg/solvers.cpp:455-658;
// order 2, the power method's eigenvalue estimate with the reference's default parameters).
//
// Unit cube, n^3 elements, p = 2, sigma = 1 + x at the quadrature points, phi = 0 on the boundary.
// Manufactured phi = sin(pi x) sin(pi y) sin(pi z), so f = 3 pi^2 sigma phi - pi cos(pi x) sin(pi y) sin(pi z);
// f is interpolated at the dofs and assembled by the device linear form as a grid-function source.
// Exit status 0 when
//   both solves converge to 1e-12,
//   the two solutions agree to 1e-9 of max|phi|,
//   max_i |phi_i - phi(x_i)| <= 6e-5 (the discrete solution's own error at n = 8 is 4.78e-5; + 25 %),
//   and the Chebyshev solve needs <= 0.75 of Jacobi's iterations.
//
// Usage: rf_potential [n = 8]
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

int main(int argc, char **argv)
{
   const int n = argc > 1 ? std::atoi(argv[1]) : 8;
   const int order = 2;
   const double pi = M_PI, rel_tol = 1e-12;

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(n, n, n, 1.0, 1.0, 1.0, &mesh));
   ecm2_h1space *fes = nullptr;
   CHECK(ecm2_h1space_create(mesh, order, ECM2_NUMBERING_ENTITY, &fes));
   int ndofs = 0, ne = 0, nd = 0;
   CHECK(ecm2_h1space_info(fes, &ndofs, &ne, &nd));
   std::vector<int> gmap((size_t)ne * nd);
   CHECK(ecm2_h1space_get_gather_map(fes, gmap.data()));
   std::vector<double> enodes((size_t)ne * 24), X((size_t)ndofs * 3);
   CHECK(ecm2_mesh_get_element_nodes(mesh, enodes.data()));
   CHECK(ecm2_h1space_dof_coords(fes, mesh, X.data()));
   int n_ess = 0;
   CHECK(ecm2_h1space_boundary_dofs(fes, nullptr, &n_ess));
   std::vector<int> ess(n_ess);
   CHECK(ecm2_h1space_boundary_dofs(fes, ess.data(), &n_ess));
   // sigma = 1 + x at the form's quadrature points (the default rule, order + 2 points per direction)
   const int q1d = order + 2, nq = q1d * q1d * q1d;
   std::vector<double> P((size_t)ne * nq * 3), sigma((size_t)ne * nq);
   CHECK(ecm2_mesh_quadrature_points(mesh, q1d, P.data()));
   for (size_t i = 0; i < sigma.size(); i++) { sigma[i] = 1.0 + P[3 * i]; }
   // the exact potential and the source at the dofs
   std::vector<double> phi(ndofs), f(ndofs);
   for (int i = 0; i < ndofs; i++)
   {
      const double x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
      phi[i] = std::sin(pi * x) * std::sin(pi * y) * std::sin(pi * z);
      f[i] = 3.0 * pi * pi * (1.0 + x) * phi[i] - pi * std::cos(pi * x) * std::sin(pi * y) * std::sin(pi * z);
   }
   std::printf("unit cube %d^3 elements, H1 p=%d, %d dofs, %d essential; sigma = 1 + x\n", n, order, ndofs, n_ess);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   ecm2_pa_form *Af = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), 0, &Af));
   CHECK(ecm2_pa_form_set_element_nodes(Af, enodes.data()));
   double *sigma_d = device_copy(sigma);
   CHECK(ecm2_pa_form_add_integrator(Af, ECM2_DIFFUSION, ECM2_COEFF_QUAD, sigma_d, nullptr));
   CHECK(ecm2_pa_form_assemble(Af, nullptr));
   ecm2_operator *A = nullptr;
   CHECK(ecm2_operator_from_pa_form(Af, &A));

   // b = (f_h, v) by the device linear form, its essential rows zeroed (phi = 0 there)
   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, enodes.data()));
   double *f_d = device_copy(f);
   CHECK(ecm2_linear_form_add_domain_integrator(lf, ECM2_COEFF_GRIDFUNC, f_d, nullptr, nullptr, nullptr, 0));
   double *b = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_linear_form_assemble(lf, b, nullptr));
   HIPCHECK(hipDeviceSynchronize());
   std::vector<double> bh = host_copy(b, ndofs);
   for (int i : ess) { bh[i] = 0.0; }
   HIPCHECK(hipMemcpy(b, bh.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));
   int *ess_d = device_copy(ess);

   // Jacobi-PCG
   double *xj = device_copy(std::vector<double>(ndofs, 0.0)), *xc = device_copy(std::vector<double>(ndofs, 0.0));
   int it_j = 0, it_c = 0;
   double nrm_j = 0.0, nrm_c = 0.0;
   CHECK(ecm2_operator_pcg(A, ess_d, n_ess, b, xj, rel_tol, 0.0, 2000, 1, &it_j, &nrm_j, nullptr));
   const int conv_j = ecm2_pcg_last_converged();
   // Chebyshev-PCG: order 2, the power method with the reference's defaults (10 steps, 1e-8)
   ecm2_smoother *sm = nullptr;
   CHECK(ecm2_chebyshev_create_power(A, nullptr, ess_d, n_ess, 2, 10, 1e-8, nullptr, &sm, nullptr));
   int cheb_order = 0, power_steps = 0;
   double max_eig = 0.0, coeffs[5];
   CHECK(ecm2_chebyshev_info(sm, &cheb_order, &max_eig, &power_steps, coeffs));
   CHECK(ecm2_operator_pcg_prec(A, sm, ess_d, n_ess, b, xc, rel_tol, 0.0, 2000, &it_c, &nrm_c, nullptr));
   const int conv_c = ecm2_pcg_last_converged();
   std::printf("Chebyshev smoother: order %d, max_eig %.6f after %d power steps, c = (%.6f, %.6f)\n", cheb_order, max_eig,
               power_steps, coeffs[0], coeffs[1]);
   std::printf("Jacobi-PCG iterations: %d (converged %d)\n", it_j, conv_j);
   std::printf("Chebyshev-PCG iterations: %d (converged %d)\n", it_c, conv_c);

   const std::vector<double> hj = host_copy(xj, ndofs), hc = host_copy(xc, ndofs);
   double gap = 0.0, err = 0.0, top = 0.0;
   for (int i = 0; i < ndofs; i++)
   {
      gap = std::max(gap, std::fabs(hj[i] - hc[i]));
      err = std::max(err, std::fabs(hc[i] - phi[i]));
      top = std::max(top, std::fabs(hj[i]));
   }
   std::printf("max|phi_jacobi - phi_chebyshev| / max|phi| = %.3e, max|phi_h - phi| = %.3e\n", gap / top, err);

   const bool pass = conv_j != 0 && conv_c != 0 && gap <= 1e-9 * top && err <= 6e-5 && it_c <= 0.75 * it_j;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_smoother_destroy(sm);
   ecm2_operator_destroy(A);
   ecm2_pa_form_destroy(Af);
   ecm2_linear_form_destroy(lf);
   (void)hipFree(xj);
   (void)hipFree(xc);
   (void)hipFree(b);
   (void)hipFree(f_d);
   (void)hipFree(sigma_d);
   (void)hipFree(ess_d);
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
