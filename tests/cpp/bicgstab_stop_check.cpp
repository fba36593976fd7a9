// bicgstab_stop_check.cpp -- CPU check of the BiCGSTAB loop's stopping decision (csrc/bicgstab_stop.hpp:
// the function the device's final-pass kernels call), run by tests/test_bicgstab_host.py under ASan + UBSan.
// Reads cases "test value tol_goal it max_iter" (values as C99 hex floats, inf or nan) from stdin and prints
// one status per line; the test compares them with the table tests/bicgstab_ref.py's stop_decision produces.
// Then it walks one iteration's tests in the kernels' order for a few scripted runs and prints the stop
// and final_iter of each, the sequence k_bcg_final follows.
#include "bicgstab_stop.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ecm2;

// the order of the tests in iteration `it` (k_bcg_final: BCG_FINAL_S, then BCG_FINAL_R with the next rho_1)
static int iteration(double snorm, double rnorm, double omega, double rho_next, double tol, int it, int max_iter,
                     int *final_iter)
{
   *final_iter = it;
   int done = bcg_stop(BCG_TEST_S, snorm, tol, it, max_iter);
   if (done) { return done; }
   done = bcg_stop(BCG_TEST_R, rnorm, tol, it, max_iter);
   if (!done) { done = bcg_stop(BCG_TEST_OMEGA, omega, tol, it, max_iter); }
   if (done == BCG_MAX_ITER) { *final_iter = max_iter; }
   if (!done)
   {
      done = bcg_stop(BCG_TEST_RHO, rho_next, tol, it + 1, max_iter);
      if (done) { *final_iter = it + 1; }
   }
   return done;
}

int main()
{
   char line[256];
   int ncase = 0;
   while (std::fgets(line, sizeof line, stdin))
   {
      if (std::strncmp(line, "end", 3) == 0) { break; }
      char vs[64], ts[64];
      int test = 0, it = 0, max_iter = 0;
      if (std::sscanf(line, "%d %63s %63s %d %d", &test, vs, ts, &it, &max_iter) != 5)
      {
         std::fprintf(stderr, "bad case line: %s", line);
         return 1;
      }
      const double value = std::strtod(vs, nullptr), tol = std::strtod(ts, nullptr);
      std::printf("%d\n", bcg_stop(test, value, tol, it, max_iter));
      ncase++;
   }
   // scripted iterations: (||s||, ||r||, omega, next rho_1, tol_goal, it, max_iter)
   const double inf = __builtin_inf(), nan = __builtin_nan("");
   const struct { double s, r, om, rho, tol; int it, mx; } runs[] = {
      {1.0, 0.5, 0.3, 2.0, 1e-3, 1, 10},    // running
      {1e-4, 0.5, 0.3, 2.0, 1e-3, 2, 10},   // ||s|| stop
      {1.0, 1e-4, 0.3, 2.0, 1e-3, 3, 10},   // ||r|| stop
      {1.0, 1e-4, 0.0, 0.0, 1e-3, 3, 3},    // ||r|| stop wins over omega == 0, max_iter and rho == 0
      {1.0, 0.5, 0.0, 2.0, 1e-3, 4, 4},     // omega == 0 wins over max_iter
      {1.0, 0.5, 0.3, 0.0, 1e-3, 5, 5},     // max_iter wins over the next rho_1
      {1.0, 0.5, 0.3, 0.0, 1e-3, 5, 10},    // rho_1 == 0: final_iter = it + 1
      {nan, 0.5, 0.3, 2.0, 1e-3, 6, 10},    // non-finite ||s||
      {1.0, inf, 0.3, 2.0, 1e-3, 6, 10},    // non-finite ||r||
      {1.0, nan, nan, nan, 1e-3, 6, 10},    // non-finite ||r|| (omega = 0 / 0)
      {1e-3, 1e-3, 0.3, 2.0, 1e-3, 7, 10},  // == tol_goal is not < tol_goal
   };
   for (const auto &q : runs)
   {
      int fi = 0;
      const int done = iteration(q.s, q.r, q.om, q.rho, q.tol, q.it, q.mx, &fi);
      std::printf("run %d %d %d\n", done, fi, bcg_converged(done) ? 1 : 0);
   }
   std::printf("cases %d\n", ncase);
   return 0;
}
