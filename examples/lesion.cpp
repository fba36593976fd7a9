// lesion.cpp -- the cell-death state through the C ABI alone (include/ecm2_pa.h, "Cell death"): which tissue died.
//
// Slab [0, 1] x [0, 0.5]^2, 8 x 4 x 4 elements, order 2; three-state kinetics with Arrhenius rates (a liver
// unfolding fit, a refolding rate, the Henriques-Moritz death fit), temperatures in degrees Celsius.
//  (a) a frozen field T(x) = 37 + 58 x: 60 steps of 1 s against one step of 60 s (the update is the exact
//      propagator, so they agree to rounding) and against the closed form -- the spectral form of exp(A t) with D
//      by conservation -- evaluated in long double on the host, per dof; then the lesion volume at theta = 0.8 from
//      ecm2_celldeath_measure (w = the linear form of the constant 1) against the host's sum.
//  (b) composition with the heat solver: ten sourced SDIRK33 steps (ecm2_ode_step_source) of the slab heated
//      towards its x = 1 end, each followed by ecm2_celldeath_step(T0 = u_old, T1 = u_new, nsub = 4); at every step
//      D is non-decreasing, all fractions lie in [0, 1] and |N + U + D - 1| <= 1e-12.
// Exit status 0 = pass (prints PASS); 2 = a library call failed (no device: ecm2_celldeath_create, no fallback).
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

typedef long double ld;
static const double kR = 8.31446261815324;

// exp(M t) (1, 0, 0) at T degrees Celsius in long double: the spectral form of the (N, U) block, D by conservation
static void closed_form(const double *par, double T, double t, ld out[3])
{
   const ld TK = (ld)T + (ld)273.15;
   ld k[3];
   for (int i = 0; i < 3; i++) { k[i] = (ld)par[2 * i] * expl(-(ld)par[2 * i + 1] / ((ld)kR * TK)); }
   const ld a = k[0], b = k[1], c = k[2];
   const ld two_delta = sqrtl((a - c) * (a - c) + b * b + 2 * b * (a + c));
   const ld lm = -((a + b + c) + two_delta) / 2, lp = lm != 0 ? a * c / lm : 0;
   const ld ep = expl(lp * t), em = expl(lm * t);
   const ld h = ((b + c) - a) / 2, big = fabsl(h) + two_delta / 2, little = big != 0 ? a * b / big : 0;
   const ld p = h >= 0 ? big : little, q = h >= 0 ? little : big;   // A - lm I = [[p, b], [a, q]]
   // exp(A t) = em I + g (A - lm I), g = (ep - em) / (2 delta) through expm1l (exact near a double eigenvalue too)
   const ld g = two_delta != 0 ? ep * (-expm1l(-two_delta * t)) / two_delta : ep * t;
   const ld N = em + g * p, U = g * a;
   out[0] = N;
   out[1] = U;
   out[2] = (1 - N) - U;
}

int main()
{
   const int nx = 8, ny = 4, nz = 4, order = 2;
   // A1, dE1, A2, dE2, A3, dE3 [1/s, J/mol]
   const double par[6] = {7.39e39, 2.577e5, 1.0e25, 1.6e5, 3.1e98, 6.28e5};
   const double theta = 0.8;

   ecm2_mesh *mesh = nullptr;
   CHECK(ecm2_mesh_cartesian(nx, ny, nz, 1.0, 0.5, 0.5, &mesh));
   ecm2_h1space *fes = nullptr;
   CHECK(ecm2_h1space_create(mesh, order, ECM2_NUMBERING_ENTITY, &fes));
   int ndofs = 0, ne = 0, nd = 0;
   CHECK(ecm2_h1space_info(fes, &ndofs, &ne, &nd));
   std::vector<int> gmap((size_t)ne * nd);
   CHECK(ecm2_h1space_get_gather_map(fes, gmap.data()));
   std::vector<double> enodes((size_t)ne * 24), X((size_t)ndofs * 3);
   CHECK(ecm2_mesh_get_element_nodes(mesh, enodes.data()));
   CHECK(ecm2_h1space_dof_coords(fes, mesh, X.data()));
   std::printf("slab %d x %d x %d elements, H1 p=%d, %d dofs; three-state cell death\n", nx, ny, nz, order, ndofs);

   // the first compute entry point: with no HIP device it fails here (ECM2_ERR_HIP), no fallback
   ecm2_celldeath *cd = nullptr;
   CHECK(ecm2_celldeath_create(ECM2_CELLDEATH_THREE_STATE, par, 273.15, ndofs, &cd));

   // ---- (a) the frozen slab ----
   std::vector<double> T(ndofs);
   for (int i = 0; i < ndofs; i++) { T[i] = 37.0 + 58.0 * X[3 * i]; }
   double *Td = device_copy(T);
   const std::vector<double> ones(ndofs, 1.0), zeros(ndofs, 0.0);
   double *N = device_copy(ones), *U = device_copy(zeros), *D = device_copy(zeros);
   double *N1 = device_copy(ones), *U1 = device_copy(zeros), *D1 = device_copy(zeros);
   int invalid = -1, invalid_total = 0;
   for (int s = 0; s < 60; s++)
   {
      CHECK(ecm2_celldeath_step(cd, Td, nullptr, 1.0, 1, N, U, D, &invalid, nullptr));
      invalid_total += invalid;
   }
   CHECK(ecm2_celldeath_step(cd, Td, nullptr, 60.0, 1, N1, U1, D1, &invalid, nullptr));
   invalid_total += invalid;
   const std::vector<double> hN = host_copy(N, ndofs), hU = host_copy(U, ndofs), hD = host_copy(D, ndofs);
   const std::vector<double> gN = host_copy(N1, ndofs), gU = host_copy(U1, ndofs), gD = host_copy(D1, ndofs);
   // the bound of the device update, 16 u (1 + x_max) per step with x_max = dE3 / (R 310.15 K)
   const double tol = 16.0 * std::ldexp(1.0, -53) * (1.0 + par[5] / (kR * 310.15));
   double err60 = 0.0, err1 = 0.0;
   for (int i = 0; i < ndofs; i++)
   {
      ld ref[3];
      closed_form(par, T[i], 60.0, ref);
      const double s[3] = {hN[i], hU[i], hD[i]}, g[3] = {gN[i], gU[i], gD[i]};
      for (int k = 0; k < 3; k++)
      {
         err60 = std::max(err60, (double)fabsl(s[k] - ref[k]));
         err1 = std::max(err1, (double)fabsl(g[k] - ref[k]));
      }
   }
   std::printf("(a) 60 steps of 1 s: max error %.3e (bound %.3e); one step of 60 s: %.3e (bound %.3e); invalid %d\n",
               err60, 60.0 * tol, err1, tol, invalid_total);

   // w = the linear form of the constant 1: sum w D, sum w [D >= theta], sum w = dead volume, lesion, |Omega|
   ecm2_linear_form *lf = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), 0, &lf));
   CHECK(ecm2_linear_form_set_element_nodes(lf, enodes.data()));
   const double one = 1.0;
   CHECK(ecm2_linear_form_add_domain_integrator(lf, ECM2_COEFF_CONSTANT, &one, nullptr, nullptr, nullptr, 0));
   double *w = device_copy(zeros);
   CHECK(ecm2_linear_form_assemble(lf, w, nullptr));
   double vol[3] = {0, 0, 0};
   CHECK(ecm2_celldeath_measure(cd, D, w, theta, vol, nullptr));
   const std::vector<double> hw = host_copy(w, ndofs);
   ld dead = 0, lesion = 0, all = 0;
   for (int i = 0; i < ndofs; i++)
   {
      dead += (ld)hw[i] * hD[i];
      lesion += hD[i] >= theta ? (ld)hw[i] : 0.0L;
      all += hw[i];
   }
   const double err_v = std::max({std::fabs(vol[0] - (double)dead) / (double)all, std::fabs(vol[1] - (double)lesion) / (double)all,
                                  std::fabs(vol[2] - (double)all) / (double)all, std::fabs(vol[2] - 0.25) / 0.25});
   std::printf("    dead volume %.6e, lesion (D >= %.1f) %.6e of |Omega| = %.15f; max relative error %.3e\n", vol[0], theta,
               vol[1], vol[2], err_v);
   const bool pass_a = err60 <= 60.0 * tol && err1 <= tol && invalid_total == 0 && err_v <= 1e-13 && vol[1] > 0.0 &&
                       vol[1] < vol[2];

   // ---- (b) composition with the sourced implicit step ----
   const int type = 23;                                  // SDIRK33
   const double c = ecm2_ode_implicit_coeff(type);
   const double rho_c = 3.6, k = 0.02, dt = 1.0, q0 = 21.0;   // (scaled units: the x = 1 end gains ~5.8 K a step)
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
   // the source q(x) = q0 x as a grid function
   std::vector<double> q(ndofs);
   for (int i = 0; i < ndofs; i++) { q[i] = q0 * X[3 * i]; }
   double *qd = device_copy(q);
   ecm2_linear_form *src = nullptr;
   CHECK(ecm2_linear_form_create(ne, order, ndofs, gmap.data(), 0, &src));
   CHECK(ecm2_linear_form_set_element_nodes(src, enodes.data()));
   CHECK(ecm2_linear_form_add_domain_integrator(src, ECM2_COEFF_GRIDFUNC, qd, nullptr, nullptr, nullptr, 0));
   double *b = device_copy(zeros);
   CHECK(ecm2_linear_form_assemble(src, b, nullptr));

   double *u = device_copy(std::vector<double>(ndofs, 37.0)), *u_old = device_copy(zeros);
   HIPCHECK(hipMemcpy(N, ones.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));
   HIPCHECK(hipMemcpy(U, zeros.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));
   HIPCHECK(hipMemcpy(D, zeros.data(), ndofs * sizeof(double), hipMemcpyHostToDevice));
   std::vector<double> Dprev(ndofs, 0.0);
   bool pass_b = true;
   double worst_sum = 0.0;
   for (int s = 1; s <= 10; s++)
   {
      HIPCHECK(hipMemcpy(u_old, u, ndofs * sizeof(double), hipMemcpyDeviceToDevice));
      int solves = 0, iters = 0, conv = 0;
      CHECK(ecm2_ode_step_source(type, Top, Kop, b, dt, u, nullptr, 0, 1e-12, 2000, 1, &solves, &iters, &conv, nullptr));
      CHECK(ecm2_celldeath_step(cd, u_old, u, dt, 4, N, U, D, &invalid, nullptr));
      const std::vector<double> n = host_copy(N, ndofs), uu = host_copy(U, ndofs), d = host_copy(D, ndofs);
      const std::vector<double> Tn = host_copy(u, ndofs);
      bool ok = conv != 0 && invalid == 0;
      for (int i = 0; i < ndofs; i++)
      {
         ok = ok && d[i] >= Dprev[i] && n[i] >= 0.0 && n[i] <= 1.0 && uu[i] >= 0.0 && uu[i] <= 1.0 && d[i] <= 1.0;
         worst_sum = std::max(worst_sum, std::fabs((n[i] + uu[i] + d[i]) - 1.0));
      }
      ok = ok && worst_sum <= 1e-12;
      CHECK(ecm2_celldeath_measure(cd, D, w, theta, vol, nullptr));
      std::printf("(b) step %2d: T max %.2f C, dead volume %.6e, lesion %.6e, max |N + U + D - 1| %.2e%s\n", s,
                  *std::max_element(Tn.begin(), Tn.end()), vol[0], vol[1], worst_sum, ok ? "" : "  <-- FAILED");
      pass_b = pass_b && ok;
      Dprev = d;
   }
   pass_b = pass_b && vol[1] > 0.0;   // the hot end died

   const bool pass = pass_a && pass_b;
   std::printf("%s\n", pass ? "PASS" : "FAIL");

   ecm2_operator_destroy(Top);
   ecm2_operator_destroy(Kop);
   ecm2_pa_form_destroy(Tf);
   ecm2_pa_form_destroy(Kf);
   ecm2_linear_form_destroy(lf);
   ecm2_linear_form_destroy(src);
   ecm2_celldeath_destroy(cd);
   for (double *p : {Td, N, U, D, N1, U1, D1, w, qd, b, u, u_old}) { (void)hipFree(p); }
   ecm2_h1space_destroy(fes);
   ecm2_mesh_destroy(mesh);
   return pass ? 0 : 1;
}
