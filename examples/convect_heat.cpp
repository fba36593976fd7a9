// convect_heat.cpp -- heat conduction with advection by a uniform flow through the C ABI alone
// (include/ecm2_pa.h): the blood-flow line of an ablation model,
//   k.AddDomainIntegrator(new ConvectionIntegrator(vel, alpha), fluid_marker)
// (ConvectionIntegrator::AssemblePA / AddMultPA, fem/integ/bilininteg_convection_pa.cpp; the multidomain
// miniapp uses it this way, miniapps/multidomain/multidomain.cpp:121), on the device.
//
// Slab [0, 1] x [0, .5]^2, 8 x 4 x 4 elements, order p.  u = x on the two x faces (boundary attributes
// 5 and 3), the other sides insulated; k = 1, rho c = 1, v = (Pe, 0, 0), Pe = 1:
//   M du/dt = -K u + b,  K = Diffusion(1) + Convection(v),  b = (Pe, phi_i) (the linear form of Pe).
// u = x solves it: K u = b at every free dof up to rounding (the diffusion part integrates to a boundary
// term that vanishes there, the convection part is Pe (1, phi_i)).  The step (ecm2_ode_step_source, type
// 21 = backward Euler) has T = M + c dt Diffusion(1), symmetric: the advection is explicit per stage, the
// diffusion implicit, the solver Jacobi-PCG.  Checked:
//   1. C (g . p) against (v . g) b_1, b_1 the linear form of 1: two independent kernels, the same
//      quadrature sums term by term: <= 1e-12 in max norm / max norm;
//   2. five steps (dt = 0.02, rel_tol 1e-12) from u = x stay there: max |u - x| <= 1e-10;
//   3. from u0 = x + 0.1 sin(pi x), thirty steps: max |u - x| falls at every step and ends at <= 2% of its
//      start (the slowest mode of the continuous problem under backward Euler gives
//      (1 + dt (pi^2 + Pe^2 / 4))^-30 = 0.4%; five times that covers the stage-explicit advection and
//      the non-modal start).
// Exit status 0 = pass.
//
// Usage: convect_heat [order = 2] [q1d = order + 2]
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
   HIPCHECK(hipDeviceSynchronize());
   HIPCHECK(hipMemcpy(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost));
   return h;
}

int main(int argc, char **argv)
{
   const int order = argc > 1 ? std::atoi(argv[1]) : 2;
   const int q1d = argc > 2 ? std::atoi(argv[2]) : order + 2;
   const int nx = 8, n = 4;
   const double Pe = 1.0, one = 1.0, dt = 0.02, pi = 3.14159265358979323846;
   const double vel[3] = {Pe, 0.0, 0.0};
   const int type = 21;  // backward Euler

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(nx, n, n, 1.0, 0.5, 0.5, &mesh));
   ecm2_h1space *fes = nullptr;
   CHECK(ecm2_h1space_create(mesh, order, ECM2_NUMBERING_ENTITY, &fes));
   int ndofs = 0, ne = 0, nd = 0, nbe = 0;
   CHECK(ecm2_h1space_info(fes, &ndofs, &ne, &nd));
   CHECK(ecm2_mesh_boundary_info(mesh, &nbe));
   const int dd = (order + 1) * (order + 1);
   std::vector<int> gmap((size_t)ne * nd), bmap((size_t)nbe * dd), battr(nbe);
   std::vector<double> enodes((size_t)ne * 24), X((size_t)ndofs * 3);
   CHECK(ecm2_h1space_get_gather_map(fes, gmap.data()));
   CHECK(ecm2_h1space_get_boundary_map(fes, bmap.data()));
   CHECK(ecm2_mesh_get_boundary(mesh, nullptr, battr.data()));
   CHECK(ecm2_mesh_get_element_nodes(mesh, enodes.data()));
   CHECK(ecm2_h1space_dof_coords(fes, mesh, X.data()));
   // essential dofs: the two x faces (Mesh::Make3D: attribute 5 left, 3 right)
   std::vector<int> ess;
   for (int b = 0; b < nbe; b++)
   {
      if (battr[b] != 5 && battr[b] != 3) { continue; }
      ess.insert(ess.end(), &bmap[(size_t)b * dd], &bmap[(size_t)b * dd] + dd);
   }
   std::sort(ess.begin(), ess.end());
   ess.erase(std::unique(ess.begin(), ess.end()), ess.end());
   const int n_ess = (int)ess.size();
   std::printf("slab %d x %d x %d elements, H1 p=%d, %d points per direction, %d dofs, %d essential dofs, Pe = %g\n", nx, n,
               n, order, q1d, ndofs, n_ess, Pe);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   ecm2_pa_form *C = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), q1d, &C));
   CHECK(ecm2_pa_form_set_element_nodes(C, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(C, ECM2_CONVECTION, ECM2_COEFF_CONST_VECTOR, vel, nullptr));
   CHECK(ecm2_pa_form_assemble(C, nullptr));
   int present = 0, n_active = 0, distinct = 0;
   CHECK(ecm2_pa_form_convection_info(C, &present, &n_active, &distinct));

   // b_1 = (1, phi_i) and b = Pe b_1, at the forms' rule
   ecm2_linear_form *lf1 = nullptr, *lfb = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), q1d, &lf1));
   CHECK(ecm2_linear_form_set_element_nodes(lf1, enodes.data()));
   CHECK(ecm2_linear_form_add_domain_integrator(lf1, ECM2_COEFF_CONSTANT, &one, nullptr, nullptr, nullptr, 0));
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), q1d, &lfb));
   CHECK(ecm2_linear_form_set_element_nodes(lfb, enodes.data()));
   CHECK(ecm2_linear_form_add_domain_integrator(lfb, ECM2_COEFF_CONSTANT, &Pe, nullptr, nullptr, nullptr, 0));
   double *b1 = device_copy(std::vector<double>(ndofs, 0.0)), *b = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_linear_form_assemble(lf1, b1, nullptr));
   CHECK(ecm2_linear_form_assemble(lfb, b, nullptr));

   // check 1: C (g . p) = (v . g) b_1
   const double g[3] = {0.4, -1.1, 0.7};
   std::vector<double> gp(ndofs), ux(ndofs);
   for (int i = 0; i < ndofs; i++)
   {
      gp[i] = g[0] * X[3 * (size_t)i] + g[1] * X[3 * (size_t)i + 1] + g[2] * X[3 * (size_t)i + 2];
      ux[i] = X[3 * (size_t)i];
   }
   double *gp_d = device_copy(gp), *cgp = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_pa_form_mult(C, gp_d, cgp, nullptr));
   const std::vector<double> cgp_h = host_copy(cgp, ndofs), b1_h = host_copy(b1, ndofs);
   const double vg = vel[0] * g[0] + vel[1] * g[1] + vel[2] * g[2];
   double err1 = 0.0, max1 = 0.0;
   for (int i = 0; i < ndofs; i++)
   {
      err1 = std::max(err1, std::fabs(cgp_h[i] - vg * b1_h[i]));
      max1 = std::max(max1, std::fabs(vg * b1_h[i]));
   }
   err1 /= max1;
   std::printf("convection on %d of %d elements; C (g . p) against (v . g) b_1: %.3e relative\n", n_active, ne, err1);

   // K = Diffusion(1) + Convection(v), T = Mass(1) + c dt Diffusion(1)
   const double cdt = ecm2_ode_implicit_coeff(type) * dt;
   ecm2_pa_form *K = nullptr, *T = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), q1d, &K));
   CHECK(ecm2_pa_form_set_element_nodes(K, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(K, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &one, nullptr));
   CHECK(ecm2_pa_form_add_integrator(K, ECM2_CONVECTION, ECM2_COEFF_CONST_VECTOR, vel, nullptr));
   CHECK(ecm2_pa_form_assemble(K, nullptr));
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), q1d, &T));
   CHECK(ecm2_pa_form_set_element_nodes(T, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(T, ECM2_MASS, ECM2_COEFF_CONSTANT, &one, nullptr));
   CHECK(ecm2_pa_form_add_integrator(T, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &cdt, nullptr));
   CHECK(ecm2_pa_form_assemble(T, nullptr));
   ecm2_operator *Top = nullptr, *Kop = nullptr;
   CHECK(ecm2_operator_from_pa_form(T, &Top));
   CHECK(ecm2_operator_from_pa_form(K, &Kop));
   int *ess_d = device_copy(ess);

   auto distance = [&](const double *u) {
      const std::vector<double> uh = host_copy(u, ndofs);
      double e = 0.0;
      for (int i = 0; i < ndofs; i++) { e = std::max(e, std::fabs(uh[i] - ux[i])); }
      return e;
   };
   int all_conv = 1, total_iters = 0;
   auto step = [&](double *u) {
      int solves = 0, iters = 0, conv = 0;
      CHECK(ecm2_ode_step_source(type, Top, Kop, b, dt, u, ess_d, n_ess, 1e-12, 2000, 1, &solves, &iters, &conv, nullptr));
      all_conv = all_conv && conv;
      total_iters += iters;
   };

   // check 2: the fixed point
   double *u = device_copy(ux);
   for (int s = 0; s < 5; s++) { step(u); }
   const double err2 = distance(u);
   std::printf("five steps from u = x: max |u - x| = %.3e\n", err2);

   // check 3: relaxation
   std::vector<double> u0(ndofs);
   for (int i = 0; i < ndofs; i++) { u0[i] = ux[i] + 0.1 * std::sin(pi * ux[i]); }
   HIPCHECK(hipMemcpy(u, u0.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));
   const double d0 = distance(u);
   double dprev = d0;
   bool falls = true;
   for (int s = 0; s < 30; s++)
   {
      step(u);
      const double d = distance(u);
      falls = falls && d < dprev;
      dprev = d;
   }
   const double ratio = dprev / d0;
   std::printf("thirty steps from x + 0.1 sin(pi x): max |u - x| %.3e -> %.3e, ratio %.4f%% (bound 2%%), monotone %d\n", d0,
               dprev, 100.0 * ratio, falls ? 1 : 0);
   std::printf("Jacobi-PCG: %d iterations in all, converged %d\n", total_iters, all_conv);

   const bool pass = present == 1 && n_active == ne && distinct == 1 && err1 <= 1e-12 && err2 <= 1e-10 && falls &&
                     ratio <= 0.02 && all_conv != 0;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_operator_destroy(Top);
   ecm2_operator_destroy(Kop);
   ecm2_pa_form_destroy(C);
   ecm2_pa_form_destroy(K);
   ecm2_pa_form_destroy(T);
   ecm2_linear_form_destroy(lf1);
   ecm2_linear_form_destroy(lfb);
   (void)hipFree(u);
   (void)hipFree(b);
   (void)hipFree(b1);
   (void)hipFree(gp_d);
   (void)hipFree(cgp);
   (void)hipFree(ess_d);
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
