// cheb_coeffs.hpp -- the polynomial coefficients of OperatorChebyshevSmoother::Setup (linalg/solvers.cpp:
// 538-617) as one plain C++ function (no HIP in it) that the smoother's constructor (solvers.cpp) and a
// CPU program (tests/cpp/cheb_coeffs_check.cpp) share.  The smoother is y = sum_k c_k (D^-1 A)^k D^-1 x,
// its residual polynomial 1 - lambda p(lambda) = T_order((theta - lambda) / delta) / T_order(theta / delta)
// on the interval [0.3, 1.2] max_eig (Adams et al., Parallel multigrid smoothing: polynomial versus
// Gauss-Seidel): theta and delta are the interval's centre and half width.
#pragma once

#include <cmath>

namespace ecm2
{

constexpr int kChebMaxOrder = 5;
constexpr int kChebOk = 0, kChebErrArg = 1;  // (Status::OK, Status::ERR_ARG of common.hpp)

// c[0 .. order) = the coefficients in the reference's closed forms (the powers through pow, as there), the
// rest 0.  Returns kChebOk, or kChebErrArg for an order outside 1..5, where the reference aborts.
inline int cheb_coeffs(int order, double max_eig, double c[5])
{
   for (int k = 0; k < kChebMaxOrder; k++) { c[k] = 0.0; }
   const double hi = 1.2 * max_eig, lo = 0.3 * max_eig;
   const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo);
   const double d2 = std::pow(delta, 2), t2 = std::pow(theta, 2);
   if (order == 1) { c[0] = 1.0 / theta; }
   else if (order == 2)
   {
      const double w = 1.0 / (d2 - 2 * t2);
      c[0] = -4 * theta * w;
      c[1] = 2 * w;
   }
   else if (order == 3)
   {
      const double d3 = 3 * d2;
      const double w = 1.0 / (-4 * std::pow(theta, 3) + theta * d3);
      c[0] = w * (d3 - 12 * t2);
      c[1] = 12 / (d3 - 4 * t2);
      c[2] = -4 * w;
   }
   else if (order == 4)
   {
      const double d8 = 8 * d2;
      const double w = 1.0 / (std::pow(delta, 4) + 8 * std::pow(theta, 4) - t2 * d8);
      c[0] = w * (32 * std::pow(theta, 3) - 16 * theta * d2);
      c[1] = w * (-48 * t2 + d8);
      c[2] = 32 * theta * w;
      c[3] = -8 * w;
   }
   else if (order == 5)
   {
      const double d45 = 5 * std::pow(delta, 4), t4 = std::pow(theta, 4);
      const double d60 = 60 * d2, d20 = 20 * d2, t160 = 160 * t2;
      const double wo = 1.0 / (16 * std::pow(theta, 5) - std::pow(theta, 3) * d20 + theta * d45);  // odd powers
      const double we = 1.0 / (d45 + 16 * t4 - t2 * d20);                                          // even powers
      c[0] = wo * (d45 + 80 * t4 - t2 * d60);
      c[1] = we * (d60 - t160);
      c[2] = wo * (-d20 + t160);
      c[3] = -80 * we;
      c[4] = 16 * wo;
   }
   else { return kChebErrArg; }
   return kChebOk;
}

} // namespace ecm2
