// bicgstab_stop.hpp -- the stopping decisions of BiCGSTABSolver::Mult (linalg/solvers.cpp:1579-1805)
// as one function the device loop's final-pass kernels (k_bicgstab.hip), the host's start of the solve
// (solvers.cpp) and a CPU program (tests/cpp/bicgstab_stop_check.cpp) share.  The tests work on
// norms ||.||_2, not on their squares, against tol_goal = max(||r_0|| rel_tol, abs_tol).
#pragma once

#include "common.hpp"

namespace ecm2
{

// The tests of one iteration i, in the reference's order.
enum BcgTest : int
{
   BCG_TEST_R0 = 0,     // before the loop, value = ||r_0||: not finite -> abort; <= tol_goal -> converged (:1630-1648)
   BCG_TEST_RHO = 1,    // value = rho_1 = (r~, r) at the start of iteration `it`: == 0 -> stopped (:1652-1675)
   BCG_TEST_S = 2,      // value = ||s||: not finite -> abort; < tol_goal -> converged after x += alpha phat (:1697-1717)
   BCG_TEST_R = 3,      // value = ||r||: not finite -> abort; < tol_goal -> converged (:1738-1761)
   BCG_TEST_OMEGA = 4   // value = omega, after the ||r|| test: == 0 -> stopped (:1762-1783); else the loop's
                        // bound: it >= max_iter -> stopped with final_iter = max_iter (:1650, 1786-1788)
};

// BCG_RUNNING, or why the loop ended.  Converged: BCG_CONVERGED (||r_0|| or ||r||) and BCG_CONVERGED_S
// (||s||: x still lacks alpha phat); not converged: BCG_MAX_ITER, BCG_RHO_ZERO, BCG_OMEGA_ZERO;
// BCG_NONFINITE: the reference's MFEM_VERIFY(IsFinite(resid)) aborts (ECM2_ERR_NUMERIC).
enum BcgDone : int
{
   BCG_RUNNING = 0,
   BCG_CONVERGED = 1,
   BCG_CONVERGED_S = 2,
   BCG_MAX_ITER = 3,
   BCG_RHO_ZERO = 4,
   BCG_OMEGA_ZERO = 5,
   BCG_NONFINITE = 6
};

__host__ __device__ inline bool bcg_finite(double v) { return v - v == 0.0; }  // (false for NaN and +-inf)

__host__ __device__ inline int bcg_stop(int test, double value, double tol_goal, int it, int max_iter)
{
   switch (test)
   {
      case BCG_TEST_R0:
         return !bcg_finite(value) ? BCG_NONFINITE : (value <= tol_goal ? BCG_CONVERGED : BCG_RUNNING);
      case BCG_TEST_RHO:
         return value == 0.0 ? BCG_RHO_ZERO : BCG_RUNNING;
      case BCG_TEST_S:
         return !bcg_finite(value) ? BCG_NONFINITE : (value < tol_goal ? BCG_CONVERGED_S : BCG_RUNNING);
      case BCG_TEST_R:
         return !bcg_finite(value) ? BCG_NONFINITE : (value < tol_goal ? BCG_CONVERGED : BCG_RUNNING);
      case BCG_TEST_OMEGA:
         return value == 0.0 ? BCG_OMEGA_ZERO : (it >= max_iter ? BCG_MAX_ITER : BCG_RUNNING);
      default: break;
   }
   return BCG_RUNNING;
}

__host__ __device__ inline bool bcg_converged(int done) { return done == BCG_CONVERGED || done == BCG_CONVERGED_S; }

} // namespace ecm2
