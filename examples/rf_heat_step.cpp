// rf_heat_step.cpp -- one RF-heated time step through the C ABI alone (include/ecm2_pa.h): the
// right-hand side of Pennes' equation  rho c dT/dt = div(k grad T) + Q  with the Joule heat
// Q = sigma |grad phi|^2 assembled by the device linear form (LinearForm + DomainLFIntegrator,
// fem/linearform_ext.cpp:20-68) and taken by the sourced implicit step (ecm2_ode_step_source).
//
// Unit cube, n^3 elements, order p; phi = the interpolant of a . x (exact in the space), sigma and
// rho c constant, no essential dofs, u0 uniform.  Two exact answers are checked:
//   sum_i b_i = sigma |a|^2          (partition of unity; the cube's volume is 1)
//   u1 = u0 + dt sigma |a|^2 / rho c at every dof  (K u0 = 0 and b = sigma |a|^2 M_1 1, so every
//                                                   SDIRK33 stage slope is the constant vector)
// Exit status 0 = pass.
//
// Usage: rf_heat_step [n = 4] [order = 2]
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

static double *device_copy(const std::vector<double> &h)
{
   double *d = nullptr;
   HIPCHECK(hipMalloc(&d, std::max<size_t>(1, h.size()) * sizeof(double)));
   if (!h.empty()) { HIPCHECK(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice)); }
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
   const int n = argc > 1 ? std::atoi(argv[1]) : 4;
   const int order = argc > 2 ? std::atoi(argv[2]) : 2;
   const double a[3] = {1.5, -0.7, 0.4};          // phi = a . x
   const double sigma = 0.6, rho_c = 3.6, k = 0.5; // (scaled units)
   const double u_init = 37.0, dt = 0.25;
   const int type = 23;                            // SDIRK33
   const double c = ecm2_ode_implicit_coeff(type);

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
   std::printf("unit cube %d^3 elements, H1 p=%d, %d dofs; linear form rule %d points per direction\n", n, order, ndofs,
               ecm2_linear_form_default_q1d(order));

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, enodes.data()));

   std::vector<double> phi(ndofs);
   for (int i = 0; i < ndofs; i++) { phi[i] = a[0] * X[3 * i] + a[1] * X[3 * i + 1] + a[2] * X[3 * i + 2]; }
   double *phi_d = device_copy(phi);
   const double joule[3] = {sigma, 0.0, 0.0};
   CHECK(ecm2_linear_form_add_domain_integrator(lf, ECM2_COEFF_JOULE, phi_d, nullptr, joule, nullptr, 0));
   double *b = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_linear_form_assemble(lf, b, nullptr));
   HIPCHECK(hipDeviceSynchronize());

   const double a2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
   double sum_b = 0.0;
   for (double v : host_copy(b, ndofs)) { sum_b += v; }
   const double err_b = std::fabs(sum_b - sigma * a2) / (sigma * a2);
   std::printf("sum b = %.15f, sigma |a|^2 = %.15f, relative error %.3e\n", sum_b, sigma * a2, err_b);

   // T = M(rho c) + c dt K(k), K = Diffusion(k); no essential dofs
   const double cdtk = c * dt * k;
   ecm2_pa_form *Tf = nullptr, *Kf = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), 0, &Tf));
   CHECK(ecm2_pa_form_set_element_nodes(Tf, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(Tf, ECM2_MASS, ECM2_COEFF_CONSTANT, &rho_c, nullptr));
   CHECK(ecm2_pa_form_add_integrator(Tf, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &cdtk, nullptr));
   CHECK(ecm2_pa_form_assemble(Tf, nullptr));
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), 0, &Kf));
   CHECK(ecm2_pa_form_set_element_nodes(Kf, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(Kf, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &k, nullptr));
   CHECK(ecm2_pa_form_assemble(Kf, nullptr));
   ecm2_operator *Top = nullptr, *Kop = nullptr;
   CHECK(ecm2_operator_from_pa_form(Tf, &Top));
   CHECK(ecm2_operator_from_pa_form(Kf, &Kop));

   double *u = device_copy(std::vector<double>(ndofs, u_init));
   int solves = 0, iters = 0, conv = 0;
   CHECK(ecm2_ode_step_source(type, Top, Kop, b, dt, u, nullptr, 0, 1e-13, 2000, 1, &solves, &iters, &conv, nullptr));
   const double rise = dt * sigma * a2 / rho_c;
   double err_u = 0.0;
   for (double v : host_copy(u, ndofs)) { err_u = std::max(err_u, std::fabs((v - u_init) - rise)); }
   err_u /= rise;
   std::printf("SDIRK33 step: %d stage solves, %d PCG iterations, converged %d\n", solves, iters, conv);
   std::printf("u1 - u0 = dt sigma |a|^2 / rho c = %.15f, max relative error %.3e\n", rise, err_u);

   const bool pass = err_b < 1e-12 && err_u < 1e-9 && conv != 0 && solves == 3;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_operator_destroy(Top);
   ecm2_operator_destroy(Kop);
   ecm2_pa_form_destroy(Tf);
   ecm2_pa_form_destroy(Kf);
   ecm2_linear_form_destroy(lf);
   (void)hipFree(u);
   (void)hipFree(b);
   (void)hipFree(phi_d);
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
