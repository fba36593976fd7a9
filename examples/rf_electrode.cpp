// rf_electrode.cpp -- the electrode problem of RF ablation and its Joule power through the C ABI alone
// (include/ecm2_pa.h): -div(sigma grad phi) = 0 with phi = V0 on the electrode, phi = 0 on the dispersive ground
// and natural conditions elsewhere -- inhomogeneous essential data on two boundary attributes.  The essential
// list comes from ecm2_h1space_essential_dofs (FiniteElementSpace::GetEssentialTrueDofs with a marker), the data
// are eliminated on the device by ecm2_operator_form_linear_system (Operator::FormLinearSystem) and the PCG starts
// from the lifted data (iterative_mode = 1, the reference's IterativeSolver default).
//
// Unit cube, n^3 elements, p = 2, sigma = 1 + x at the form's quadrature points; the boundary attributes are read
// from ecm2_mesh_get_boundary: the electrode is the face x = 0 (phi = V0 = 30), the ground the face x = 1.  The exact
// potential is phi = V0 (1 - ln(1 + x) / ln 2) and the dissipated power int sigma |grad phi|^2 = V0^2 / ln 2.
// The Joule source is the device linear form of ECM2_COEFF_JOULE with sigma(T) = 1 (1 + 1 (T - 0)) and T := the
// dofs' x-coordinate; its entries sum to the power (the shape functions sum to one).
// Exit status 0 when
//   the solve converges to rel_tol = 1e-13,
//   phi on the essential dofs is bitwise the prescribed data,
//   max_i |phi_i - phi(x_i)| / V0 <= 1.9e-6,
//   sum_i b_i lies within (0, 5.7e-7] relative above V0^2 / ln 2 (the discrete energy is an upper bound),
//   |sum_i b_i - phi^T (K phi)| <= 1e-12 sum_i b_i (both rules integrate the degree-5 integrand exactly),
//   and a second solve with sigma = 1 meets the linear potential V0 (1 - x) to 1e-9 of V0.
// The two discretisation bounds are the CPU oracle's own values for this problem at n = 8, 1.497e-6 and +4.539e-7,
// plus 25 %; tests/test_ess_reference.py::test_rf_electrode_discretisation_values derives them again.  They are
// not device figures.
//
// Usage: rf_electrode [n = 8]   (the bounds above are those of n = 8)
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
   HIPCHECK(hipMemcpy(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost));
   return h;
}

struct Solve
{
   std::vector<double> phi;
   int iterations = 0, converged = 0;
   bool data_kept = false;
};

// FormLinearSystem + Jacobi-PCG from the lifted data; b = 0 (no source)
static Solve solve_potential(ecm2_operator *A, const int *ess_d, const std::vector<int> &ess,
                             const std::vector<double> &data, int ndofs, double rel_tol)
{
   std::vector<double> x0(ndofs, 0.0);
   for (size_t k = 0; k < ess.size(); k++) { x0[ess[k]] = data[k]; }
   double *x = device_copy(x0), *b = device_copy(std::vector<double>(ndofs, 0.0));
   const int n_ess = (int)ess.size();
   CHECK(ecm2_operator_form_linear_system(A, ess_d, n_ess, x, b, 0, nullptr));
   Solve s;
   double nrm = 0.0;
   CHECK(ecm2_operator_pcg_ex(A, ess_d, n_ess, b, x, rel_tol, 0.0, 2000, 1, &s.iterations, &nrm, nullptr, 1));
   s.converged = ecm2_pcg_last_converged();
   s.phi = host_copy(x, ndofs);
   s.data_kept = true;
   for (size_t k = 0; k < ess.size(); k++)
   {
      s.data_kept = s.data_kept && std::memcmp(&s.phi[ess[k]], &data[k], sizeof(double)) == 0;
   }
   (void)hipFree(x);
   (void)hipFree(b);
   return s;
}

int main(int argc, char **argv)
{
   const int n = argc > 1 ? std::atoi(argv[1]) : 8;
   const int order = 2;
   const double V0 = 30.0, rel_tol = 1e-13;

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(n, n, n, 1.0, 1.0, 1.0, &mesh));
   ecm2_h1space *fes = nullptr;
   CHECK(ecm2_h1space_create(mesh, order, ECM2_NUMBERING_ENTITY, &fes));
   int ndofs = 0, ne = 0, nd = 0, nv = 0, nbe = 0;
   CHECK(ecm2_h1space_info(fes, &ndofs, &ne, &nd));
   CHECK(ecm2_mesh_info(mesh, &nv, nullptr));
   std::vector<int> gmap((size_t)ne * nd);
   CHECK(ecm2_h1space_get_gather_map(fes, gmap.data()));
   std::vector<double> enodes((size_t)ne * 24), X((size_t)ndofs * 3), V((size_t)nv * 3);
   CHECK(ecm2_mesh_get_element_nodes(mesh, enodes.data()));
   CHECK(ecm2_h1space_dof_coords(fes, mesh, X.data()));
   CHECK(ecm2_mesh_get_vertices(mesh, V.data()));
   // the attributes of the faces x = 0 (electrode) and x = 1 (ground), from the boundary elements themselves
   CHECK(ecm2_mesh_boundary_info(mesh, &nbe));
   std::vector<int> bverts((size_t)nbe * 4), battr(nbe);
   CHECK(ecm2_mesh_get_boundary(mesh, bverts.data(), battr.data()));
   const int n_marker = *std::max_element(battr.begin(), battr.end());
   std::vector<int> marker(n_marker, 0);
   int electrode = 0, ground = 0;
   for (int b = 0; b < nbe; b++)
   {
      double lo = 1.0, hi = 0.0;
      for (int k = 0; k < 4; k++)
      {
         lo = std::min(lo, V[3 * (size_t)bverts[4 * b + k]]);
         hi = std::max(hi, V[3 * (size_t)bverts[4 * b + k]]);
      }
      if (hi == 0.0) { electrode = battr[b]; }
      if (lo == 1.0) { ground = battr[b]; }
   }
   if (electrode == 0 || ground == 0 || electrode == ground)
   {
      std::fprintf(stderr, "no boundary attribute of its own on x = 0 or x = 1\n");
      return 2;
   }
   marker[electrode - 1] = marker[ground - 1] = 1;
   int n_ess = 0;
   CHECK(ecm2_h1space_essential_dofs(fes, marker.data(), n_marker, nullptr, &n_ess));
   std::vector<int> ess(n_ess);
   CHECK(ecm2_h1space_essential_dofs(fes, marker.data(), n_marker, ess.data(), &n_ess));
   std::vector<double> data(n_ess);
   for (int k = 0; k < n_ess; k++) { data[k] = X[3 * (size_t)ess[k]] < 0.5 ? V0 : 0.0; }
   // sigma = 1 + x at the form's quadrature points (the default rule, order + 2 points per direction)
   const int q1d = order + 2, nq = q1d * q1d * q1d;
   std::vector<double> P((size_t)ne * nq * 3), sigma((size_t)ne * nq);
   CHECK(ecm2_mesh_quadrature_points(mesh, q1d, P.data()));
   for (size_t i = 0; i < sigma.size(); i++) { sigma[i] = 1.0 + P[3 * i]; }
   std::printf("unit cube %d^3 elements, H1 p=%d, %d dofs, %d essential (attributes %d: phi = %g, %d: phi = 0); "
               "sigma = 1 + x\n", n, order, ndofs, n_ess, electrode, V0, ground);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   ecm2_pa_form *Kf = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), 0, &Kf));
   CHECK(ecm2_pa_form_set_element_nodes(Kf, enodes.data()));
   double *sigma_d = device_copy(sigma);
   CHECK(ecm2_pa_form_add_integrator(Kf, ECM2_DIFFUSION, ECM2_COEFF_QUAD, sigma_d, nullptr));
   CHECK(ecm2_pa_form_assemble(Kf, nullptr));
   ecm2_operator *K = nullptr;
   CHECK(ecm2_operator_from_pa_form(Kf, &K));
   int *ess_d = device_copy(ess);

   const Solve s = solve_potential(K, ess_d, ess, data, ndofs, rel_tol);
   double err = 0.0;
   for (int i = 0; i < ndofs; i++)
   {
      err = std::max(err, std::fabs(s.phi[i] - V0 * (1.0 - std::log1p(X[3 * (size_t)i]) / std::log(2.0))));
   }
   std::printf("Jacobi-PCG from the lifted data: %d iterations (converged %d), essential data kept bitwise %d\n",
               s.iterations, s.converged, (int)s.data_kept);
   std::printf("max|phi_h - phi| / V0 = %.3e\n", err / V0);

   // the Joule source b_i = int sigma(T) |grad phi_h|^2 v_i, sigma(T) = 1 + T, T = x at the dofs
   std::vector<double> T(ndofs);
   for (int i = 0; i < ndofs; i++) { T[i] = X[3 * (size_t)i]; }
   double *phi_d = device_copy(s.phi), *T_d = device_copy(T), *b = device_copy(std::vector<double>(ndofs, 0.0));
   double *y = device_copy(std::vector<double>(ndofs, 0.0));
   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, enodes.data()));
   const double joule[3] = {1.0, 1.0, 0.0};
   CHECK(ecm2_linear_form_add_domain_integrator(lf, ECM2_COEFF_JOULE, phi_d, T_d, joule, nullptr, 0));
   CHECK(ecm2_linear_form_assemble(lf, b, nullptr));
   CHECK(ecm2_operator_mult(K, phi_d, y, nullptr));
   HIPCHECK(hipDeviceSynchronize());
   const std::vector<double> bh = host_copy(b, ndofs), yh = host_copy(y, ndofs);
   long double power_l = 0.0L, energy_l = 0.0L;
   for (int i = 0; i < ndofs; i++)
   {
      power_l += bh[i];
      energy_l += (long double)s.phi[i] * yh[i];
   }
   const double power = (double)power_l, exact = V0 * V0 / std::log(2.0);
   const double excess = (power - exact) / exact, gap = std::fabs((double)(power_l - energy_l));
   std::printf("Joule power sum b = %.12e, V0^2 / ln 2 = %.12e, relative excess %+.3e\n", power, exact, excess);
   std::printf("|sum b - phi^T K phi| / sum b = %.3e\n", gap / power);

   // sigma = 1: the linear potential is in the space
   ecm2_pa_form *Lf = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), 0, &Lf));
   CHECK(ecm2_pa_form_set_element_nodes(Lf, enodes.data()));
   const double one = 1.0;
   CHECK(ecm2_pa_form_add_integrator(Lf, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &one, nullptr));
   CHECK(ecm2_pa_form_assemble(Lf, nullptr));
   ecm2_operator *L = nullptr;
   CHECK(ecm2_operator_from_pa_form(Lf, &L));
   const Solve s1 = solve_potential(L, ess_d, ess, data, ndofs, rel_tol);
   double err1 = 0.0;
   for (int i = 0; i < ndofs; i++) { err1 = std::max(err1, std::fabs(s1.phi[i] - V0 * (1.0 - X[3 * (size_t)i]))); }
   std::printf("sigma = 1: %d iterations (converged %d), max|phi_h - V0 (1 - x)| / V0 = %.3e\n", s1.iterations,
               s1.converged, err1 / V0);

   const bool pass = s.converged != 0 && s.data_kept && err <= 1.9e-6 * V0 && excess > 0.0 && excess <= 5.7e-7
                     && gap <= 1e-12 * power && s1.converged != 0 && s1.data_kept && err1 <= 1e-9 * V0;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_linear_form_destroy(lf);
   ecm2_operator_destroy(L);
   ecm2_pa_form_destroy(Lf);
   ecm2_operator_destroy(K);
   ecm2_pa_form_destroy(Kf);
   (void)hipFree(y);
   (void)hipFree(b);
   (void)hipFree(T_d);
   (void)hipFree(phi_d);
   (void)hipFree(sigma_d);
   (void)hipFree(ess_d);
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
