// robin_heat.cpp -- a steady heat problem with a convective (Robin) wall through the C ABI alone
// (include/ecm2_pa.h): the two boundary lines of an ablation model,
//   a.AddBoundaryIntegrator(new MassIntegrator(h), robin_marker)
//   b.AddBoundaryIntegrator(new BoundaryLFIntegrator(h T_b), robin_marker)
// (PABilinearFormExtension's boundary blocks, fem/bilinearform_ext.cpp:625-675, :441-452;
// LinearFormExtension::Assemble's boundary loop, fem/linearform_ext.cpp:70-111), on the device.
//
// Slab [0, L] x [0, 1]^2, nx x n x n elements, order p.  T = T0 on x = 0 (boundary attribute 5),
// -k dT/dn = h (T - T_b) on x = L (attribute 3), the other four sides insulated:
//   (K_k + H_h) u = b_{h T_b},  solved by constrained Jacobi-PCG at rel_tol 1e-13.
// The solution u = T0 - h (T0 - T_b) x / (k + h L) is linear, so it lies in the space for every p and
// the error is the solver's only.  Checked: max |u - u_exact| / max |u_exact| < 1e-9, and
// sum_i b_i = h T_b (the Robin face has area 1).  Exit status 0 = pass.
//
// Usage: robin_heat [n = 4] [order = 2] [nx = 2 n]
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
   const int n = argc > 1 ? std::atoi(argv[1]) : 4;
   const int order = argc > 2 ? std::atoi(argv[2]) : 2;
   const int nx = argc > 3 ? std::atoi(argv[3]) : 2 * n;
   const double L = 2.0, k = 0.5, h = 25.0, T0 = 37.0, Tb = 20.0;  // (scaled units)
   const int attr_dirichlet = 5, attr_robin = 3;                   // Mesh::Make3D: left, right

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(nx, n, n, L, 1.0, 1.0, &mesh));
   ecm2_h1space *fes = nullptr;
   CHECK(ecm2_h1space_create(mesh, order, ECM2_NUMBERING_ENTITY, &fes));
   int ndofs = 0, ne = 0, nd = 0, nbe = 0;
   CHECK(ecm2_h1space_info(fes, &ndofs, &ne, &nd));
   CHECK(ecm2_mesh_boundary_info(mesh, &nbe));
   const int dd = (order + 1) * (order + 1);
   std::vector<int> gmap((size_t)ne * nd), bmap((size_t)nbe * dd), battr(nbe);
   std::vector<double> enodes((size_t)ne * 24), bnodes((size_t)nbe * 12), X((size_t)ndofs * 3);
   CHECK(ecm2_h1space_get_gather_map(fes, gmap.data()));
   CHECK(ecm2_h1space_get_boundary_map(fes, bmap.data()));
   CHECK(ecm2_mesh_get_boundary(mesh, nullptr, battr.data()));
   CHECK(ecm2_mesh_get_element_nodes(mesh, enodes.data()));
   CHECK(ecm2_mesh_get_boundary_nodes(mesh, bnodes.data()));
   CHECK(ecm2_h1space_dof_coords(fes, mesh, X.data()));
   // essential dofs: the dofs of the boundary elements with the Dirichlet attribute
   std::vector<int> ess;
   int n_robin = 0;
   for (int b = 0; b < nbe; b++)
   {
      n_robin += battr[b] == attr_robin;
      if (battr[b] != attr_dirichlet) { continue; }
      ess.insert(ess.end(), &bmap[(size_t)b * dd], &bmap[(size_t)b * dd] + dd);
   }
   std::sort(ess.begin(), ess.end());
   ess.erase(std::unique(ess.begin(), ess.end()), ess.end());
   const int n_ess = (int)ess.size();
   std::printf("slab %d x %d x %d elements, H1 p=%d, %d dofs, %d boundary faces (%d Robin), %d essential dofs\n", nx, n, n,
               order, ndofs, nbe, n_robin, n_ess);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   ecm2_pa_form *A = nullptr;
   CHECK(ecm2_pa_form_create(ne, order, ndofs, gmap.data(), 0, &A));
   CHECK(ecm2_pa_form_set_element_nodes(A, enodes.data()));
   CHECK(ecm2_pa_form_add_integrator(A, ECM2_DIFFUSION, ECM2_COEFF_CONSTANT, &k, nullptr));
   const int marker[6] = {0, 0, 1, 0, 0, 0};  // attribute 3
   CHECK(ecm2_pa_form_set_boundary(A, nbe, bmap.data(), battr.data(), bnodes.data(), 0));
   CHECK(ecm2_pa_form_add_boundary_integrator(A, ECM2_MASS, ECM2_COEFF_CONSTANT, &h, marker, 6));
   CHECK(ecm2_pa_form_assemble(A, nullptr));
   int n_active = 0, bq = 0;
   CHECK(ecm2_pa_form_boundary_info(A, nullptr, nullptr, &n_active, &bq));

   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, enodes.data()));
   CHECK(ecm2_linear_form_set_boundary(lf, nbe, bmap.data(), battr.data(), bnodes.data(), 0));
   const double hTb = h * Tb;
   CHECK(ecm2_linear_form_add_boundary_integrator(lf, ECM2_COEFF_CONSTANT, &hTb, marker, 6));
   double *b = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_linear_form_assemble(lf, b, nullptr));
   HIPCHECK(hipDeviceSynchronize());
   std::vector<double> bh = host_copy(b, ndofs);
   double sum_b = 0.0;
   for (double v : bh) { sum_b += v; }
   const double err_b = std::fabs(sum_b - hTb) / hTb;
   std::printf("face rule %d points per direction, %d active faces; sum b = %.15f, h T_b = %.15f, relative error %.3e\n",
               bq, n_active, sum_b, hTb, err_b);

   // eliminate the Dirichlet values: b <- b - A u_D on the free dofs, b = T0 on the essential ones
   std::vector<double> uD(ndofs, 0.0);
   for (int i : ess) { uD[i] = T0; }
   double *uD_d = device_copy(uD), *AuD = device_copy(std::vector<double>(ndofs, 0.0));
   CHECK(ecm2_pa_form_mult(A, uD_d, AuD, nullptr));
   HIPCHECK(hipDeviceSynchronize());
   const std::vector<double> AuDh = host_copy(AuD, ndofs);
   for (int i = 0; i < ndofs; i++) { bh[i] -= AuDh[i]; }
   for (int i : ess) { bh[i] = T0; }
   HIPCHECK(hipMemcpy(b, bh.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));

   int *ess_d = device_copy(ess);
   double *u = device_copy(std::vector<double>(ndofs, 0.0));
   int iters = 0;
   double final_norm = 0.0;
   CHECK(ecm2_pcg_solve(A, ess_d, n_ess, b, u, 1e-13, 0.0, 5000, 1, &iters, &final_norm, nullptr));
   const int conv = ecm2_pcg_last_converged();
   const std::vector<double> uh = host_copy(u, ndofs);
   double err_u = 0.0, umax = 0.0, u_wall = 0.0;
   for (int i = 0; i < ndofs; i++)
   {
      const double ue = T0 - h * (T0 - Tb) * X[3 * (size_t)i] / (k + h * L);
      if (X[3 * (size_t)i] == L) { u_wall = uh[i]; }
      err_u = std::max(err_u, std::fabs(uh[i] - ue));
      umax = std::max(umax, std::fabs(ue));
   }
   err_u /= umax;
   std::printf("Jacobi-PCG: %d iterations, converged %d; wall temperature %.12f (exact %.12f)\n", iters, conv,
               u_wall, T0 - h * (T0 - Tb) * L / (k + h * L));
   std::printf("max |u - u_exact| / max |u_exact| = %.3e\n", err_u);

   const bool pass = err_b < 1e-12 && err_u < 1e-9 && conv != 0 && n_active == n_robin;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_pa_form_destroy(A);
   ecm2_linear_form_destroy(lf);
   (void)hipFree(u);
   (void)hipFree(b);
   (void)hipFree(uD_d);
   (void)hipFree(AuD);
   (void)hipFree(ess_d);
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
