// implicit_convect_heat.cpp -- convection-dominated heat conduction with the advection inside the implicit
// operator, through the C ABI alone (include/ecm2_pa.h): the blood pool beside the tissue, where the time
// step must be set by accuracy and not by the flow.  The stage solver is BiCGSTABSolver (linalg/solvers.cpp:
// 1579-1805) with OperatorJacobiSmoother built from the symmetric form, as an MFEM user pairs them for a
// form that carries a ConvectionIntegrator.
//
// Slab [0, 1] x [0, .25]^2, 8 x 2 x 2 elements, p = 2.  u = 0 / 1 on the two x faces (boundary attributes 5
// and 3), the other sides insulated; rho c = 1, k = 1, v = (Pe, 0, 0), Pe = 10; start u = x; forty backward
// Euler steps of dt = 0.1 -- eight times h / Pe, beyond what the explicit treatment of the advection bears:
//   T = Mass(1) + c dt (Diffusion(1) + Convection(v)),  K = Diffusion(1) + Convection(v),
//   jacobi_of = Mass(1) + c dt Diffusion(1),            ecm2_ode_step_bicgstab.
// Checked:
//   1. the state stops moving: the last step's increment is <= 1e-10 of max |u|;
//   2. it is the steady state: max |u - (e^{Pe x} - 1) / (e^{Pe} - 1)| <= 5.3e-3, twice the discrete steady
//      state's own distance from the closed form on this mesh (2.62e-3, tests/test_bicgstab_reference.py);
//   3. the essential values are bitwise unchanged;
//   4. the explicit treatment at the same dt (the convection in K only, T = Mass + c dt Diffusion symmetric,
//      ecm2_ode_step_source with Jacobi-PCG) moves away from the steady state: its error after forty steps
//      is larger than at the start.
// Exit status 0 = pass.
//
// Usage: implicit_convect_heat [q1d = 4]
#include "ecm2_pa.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
   const int order = 2;
   const int q1d = argc > 1 ? std::atoi(argv[1]) : 4;
   const int nx = 8, n = 2, steps = 40;
   const double Pe = 10.0, one = 1.0, dt = 0.1;
   const double vel[3] = {Pe, 0.0, 0.0};
   const int type = 21;  // backward Euler

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(nx, n, n, 1.0, 0.25, 0.25, &mesh));
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
   std::printf("slab %d x %d x %d elements, H1 p=%d, %d points per direction, %d dofs, %d essential dofs, Pe = %g, dt = %g\n",
               nx, n, n, order, q1d, ndofs, n_ess, Pe, dt);

   // the start u = x (0 and 1 on the two faces) and the closed-form steady state
   std::vector<double> u0(ndofs), exact(ndofs);
   for (int i = 0; i < ndofs; i++)
   {
      u0[i] = X[3 * (size_t)i];
      exact[i] = std::expm1(Pe * u0[i]) / std::expm1(Pe);
   }

   const double cdt = ecm2_ode_implicit_coeff(type) * dt;
   const double cvel[3] = {cdt * Pe, 0.0, 0.0};
   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   // T = Mass + c dt (Diffusion + Convection): nonsymmetric
   ecm2_pa_form *T = nullptr, *Ts = nullptr, *K = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), q1d, &T));
   CHECK(ecm2_pa_form_set_element_nodes(T, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(T, ECM2_MASS, ECM2_COEFF_CONSTANT, &one, nullptr));
   CHECK(ecm2_pa_form_add_integrator(T, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &cdt, nullptr));
   CHECK(ecm2_pa_form_add_integrator(T, ECM2_CONVECTION, ECM2_COEFF_CONST_VECTOR, cvel, nullptr));
   CHECK(ecm2_pa_form_assemble(T, nullptr));
   // its symmetric part: the preconditioner's operator, and the explicit treatment's T
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), q1d, &Ts));
   CHECK(ecm2_pa_form_set_element_nodes(Ts, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(Ts, ECM2_MASS, ECM2_COEFF_CONSTANT, &one, nullptr));
   CHECK(ecm2_pa_form_add_integrator(Ts, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &cdt, nullptr));
   CHECK(ecm2_pa_form_assemble(Ts, nullptr));
   // K = Diffusion + Convection
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), q1d, &K));
   CHECK(ecm2_pa_form_set_element_nodes(K, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(K, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &one, nullptr));
   CHECK(ecm2_pa_form_add_integrator(K, ECM2_CONVECTION, ECM2_COEFF_CONST_VECTOR, vel, nullptr));
   CHECK(ecm2_pa_form_assemble(K, nullptr));
   ecm2_operator *Top = nullptr, *Tsop = nullptr, *Kop = nullptr;
   CHECK(ecm2_operator_from_pa_form(T, &Top));
   CHECK(ecm2_operator_from_pa_form(Ts, &Tsop));
   CHECK(ecm2_operator_from_pa_form(K, &Kop));
   int *ess_d = device_copy(ess);

   auto distance = [&](const std::vector<double> &a, const std::vector<double> &b) {
      double e = 0.0;
      for (int i = 0; i < ndofs; i++) { e = std::max(e, std::fabs(a[i] - b[i])); }
      return e;
   };
   const double err0 = distance(u0, exact);

   // the advection implicit: BiCGSTAB stage solves
   double *u = device_copy(u0);
   int all_conv = 1, total_iters = 0;
   std::vector<double> prev = u0, cur = u0;
   for (int s = 0; s < steps; s++)
   {
      int solves = 0, iters = 0, conv = 0;
      CHECK(ecm2_ode_step_bicgstab(type, Top, Tsop, Kop, nullptr, dt, u, ess_d, n_ess, 1e-12, 2000, &solves, &iters, &conv,
                                   nullptr));
      all_conv = all_conv && conv;
      total_iters += iters;
      if (s >= steps - 2)
      {
         prev = cur;
         cur = host_copy(u, ndofs);
      }
   }
   double umax = 0.0;
   for (int i = 0; i < ndofs; i++) { umax = std::max(umax, std::fabs(cur[i])); }
   const double incr = distance(cur, prev) / umax, err = distance(cur, exact);
   bool ess_same = true;
   for (int i : ess) { ess_same = ess_same && std::memcmp(&cur[i], &u0[i], sizeof(double)) == 0; }
   std::printf("implicit advection, %d steps: last increment %.3e of max |u| (bound 1e-10), max |u - closed form| %.3e -> %.3e "
               "(bound 5.3e-3), essential values unchanged %d\n",
               steps, incr, err0, err, ess_same ? 1 : 0);
   std::printf("BiCGSTAB: %d iterations in all, converged %d\n", total_iters, all_conv);

   // the explicit treatment at the same dt: T symmetric, the convection in K only
   HIPCHECK(hipMemcpy(u, u0.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));
   int pcg_conv = 1;
   for (int s = 0; s < steps; s++)
   {
      int solves = 0, iters = 0, conv = 0;
      CHECK(ecm2_ode_step_source(type, Tsop, Kop, nullptr, dt, u, ess_d, n_ess, 1e-12, 2000, 1, &solves, &iters, &conv, nullptr));
      pcg_conv = pcg_conv && conv;
   }
   const std::vector<double> uex = host_copy(u, ndofs);
   double err_ex = distance(uex, exact);
   if (!(err_ex == err_ex)) { err_ex = HUGE_VAL; }  // (a NaN state has left the steady state too)
   std::printf("explicit advection at the same dt: max |u - closed form| %.3e -> %.3e (moves away: %d), PCG converged %d\n", err0,
               err_ex, err_ex > err0 ? 1 : 0, pcg_conv);

   const bool pass = all_conv != 0 && incr <= 1e-10 && err <= 5.3e-3 && ess_same && err_ex > err0;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_operator_destroy(Top);
   ecm2_operator_destroy(Tsop);
   ecm2_operator_destroy(Kop);
   ecm2_pa_form_destroy(T);
   ecm2_pa_form_destroy(Ts);
   ecm2_pa_form_destroy(K);
   (void)hipFree(u);
   (void)hipFree(ess_d);
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
