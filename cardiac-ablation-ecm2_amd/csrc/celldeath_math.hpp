// celldeath_math.hpp -- one entry's update of the cell-death state (include/ecm2_pa.h, "Cell death"), stated
// once as a function of scalars that the device kernel (k_celldeath.hip) and a CPU program
// (tests/cpp/celldeath_check.cpp) share; tests/celldeath_ref.py restates it in extended precision.  Plain C++,
// no HIP types.
//
// Three-state model, rates a, b, c = k1, k2, k3 frozen over a substep of length dt: (N, U) obey the 2 x 2
// system with matrix A = [[-a, b], [a, -(b + c)]], trace -sigma (sigma = a + b + c), determinant a c, real
// eigenvalues lm = -(sigma / 2 + delta) <= lp = a c / lm <= 0 with (2 delta)^2 = (a - c)^2 + b^2 + 2 b (a + c).
//   exp(A dt)        = em I + g (A - lm I),    em = e^{lm dt},  g = e^{lp dt} (-expm1(-2 delta dt)) / (2 delta)
//   int_0^dt exp(A s) = psi(lm) I + G (A - lm I),  psi(l) = expm1(l dt) / l,  G = (psi(lp) - psi(lm)) / (2 delta)
//                                                                        = (g - psi(lm)) / lp
// and D advances by dD = c int U ds >= 0.  The three hazards of the formulation:
//   overflow     g is the product of two factors <= 1 and dt-sized; no sinh, nothing grows with delta dt.
//   degeneracy   every quotient takes its limit where its denominator is zero (lm = 0: all rates zero;
//                lp = 0: a c = 0; delta = 0: a = c, b = 0), so a zero-rate entry is bitwise unchanged; near a
//                double eigenvalue G is taken in the form that does not divide a difference by 2 delta.
//   monotone D   D is never formed as 1 - N - U: dD is clamped at 0 from below, and A - lm I has the
//                non-negative entries p = (b + c - a) / 2 + delta, b, a, q = (a - b - c) / 2 + delta
//                (delta >= |a - b - c| / 2 because (2 delta)^2 - (a - b - c)^2 = 4 a b), formed without a
//                subtraction through p q = a b: N, U >= 0 by construction.  All three are clamped at 1 from above.
#pragma once

#include <cmath>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace ecm2
{

enum CellDeathModel : int
{
   CELLDEATH_THREE_STATE = 0,
   CELLDEATH_ARRHENIUS = 1
};

constexpr double kGasConstant = 8.31446261815324;  // J / (mol K)
// the discriminant squares the rates: frequency factors above this are refused at create
constexpr double kCellDeathMaxA = 1e150;

struct CellDeathParams
{
   int model;
   double A[3], dE[3];  // k_i = A_i exp(-dE_i / (R T_K))
   double t_offset;     // T_K = T + t_offset
};

// The exact propagator of the three-state kinetics over dt at frozen rates a, b, c >= 0.
__host__ __device__ inline void celldeath_propagate(double a, double b, double c, double dt, double &N, double &U,
                                                    double &D)
{
   const double amc = a - c;
   const double two_delta = sqrt(amc * amc + b * b + 2.0 * b * (a + c));
   const double delta = 0.5 * two_delta, h = 0.5 * ((b + c) - a);
   const double lm = -(0.5 * ((a + b) + c) + delta);
   const double lp = lm != 0.0 ? (a * c) / lm : 0.0;
   const double xm = lm * dt;
   const double em = exp(xm), em1m = expm1(xm), em1p = expm1(lp * dt);
   const double ep = 1.0 + em1p;
   const double psim = lm != 0.0 ? em1m / lm : dt;
   const double psip = lp != 0.0 ? em1p / lp : dt;
   // g and G.  G has two algebraically equal forms (e^{lp dt} = e^{lm dt} + 2 delta g): the divided difference
   // (psi(lp) - psi(lm)) / (2 delta), which cancels near a double eigenvalue (2 delta << |lp|), and
   // (g - psi(lm)) / lp, which cancels where |lp| << |lm|: the one whose denominator is the larger is taken.  With
   // |lp| >= 2 delta, |lm| <= 2 |lp|, and what multiplies G is c (a N + q U) with c a / |lp| = |lm|: the second
   // form's rounding, u max(g, psi(lm)), enters dD times |lm|, and psi(lm) |lm| <= 1, g |lm| <= 2 |lp| dt e^{lp dt}
   // <= 2 / e -- an absolute error of a few u.  It also covers delta = 0 (g = dt e^{lm dt}) without a limit of
   // its own.  lp = delta = 0: all rates are zero and c G is zero whatever G is.
   const double g = two_delta != 0.0 ? ep * (-expm1(-(two_delta * dt))) / two_delta : ep * dt;
   const double G = -lp >= two_delta ? (lp != 0.0 ? (g - psim) / lp : 0.0) : (psip - psim) / two_delta;
   // p q = a b: the one of p, q that is a sum of non-negative terms directly, the other through the product
   // (delta - |h| cancels: it left an error of u (a + b + c) in a term that 1 / u-sized factors multiply)
   const double big = fabs(h) + delta, prod = a * b;
   const double little = big != 0.0 ? prod / big : 0.0;
   const double p = h >= 0.0 ? big : little, q = h >= 0.0 ? little : big;
   const double fu = a * N + q * U;
   const double Nn = em * N + g * (p * N + b * U);
   const double Un = em * U + g * fu;
   const double dD = fmax(c * (psim * U + G * fu), 0.0);
   N = fmin(Nn, 1.0);
   U = fmin(Un, 1.0);
   D = fmin(D + dD, 1.0);
}

// One entry over a step of length dt in nsub substeps; substep m takes T0 + ((m + 1/2) / nsub) dT (dT = T1 - T0,
// or 0 without T1).  Returns false and leaves the state untouched when T_K = T + t_offset is non-finite or <= 0
// at any substep.  CELLDEATH_ARRHENIUS keeps Omega in U: Omega += dt_sub A_1 exp(-dE_1 / (R T_K)); then
// D = max(D, -expm1(-Omega)), N = 1 - D; an entry whose Omega did not move is left untouched.
__host__ __device__ inline bool celldeath_update(const CellDeathParams &P, double T0, double dT, double dt, int nsub,
                                                 double &N, double &U, double &D)
{
   const double h = dt / nsub;
   double n = N, u = U, d = D;
   double k1 = 0.0, k2 = 0.0, k3 = 0.0;
   for (int m = 0; m < nsub; m++)
   {
      if (m == 0 || dT != 0.0)
      {
         const double w = (m + 0.5) / nsub;
         const double TK = (T0 + w * dT) + P.t_offset;
         if (!(TK > 0.0) || !(TK - TK == 0.0)) { return false; }
         const double irt = 1.0 / (kGasConstant * TK);
         k1 = P.A[0] * exp(-(P.dE[0] * irt));
         if (P.model == CELLDEATH_THREE_STATE)
         {
            k2 = P.A[1] * exp(-(P.dE[1] * irt));
            k3 = P.A[2] * exp(-(P.dE[2] * irt));
         }
      }
      if (P.model == CELLDEATH_THREE_STATE) { celldeath_propagate(k1, k2, k3, h, n, u, d); }
      else { u = u + h * k1; }
   }
   if (P.model != CELLDEATH_THREE_STATE)
   {
      if (u == U) { return true; }
      d = fmax(D, -expm1(-u));
      n = 1.0 - d;
   }
   N = n;
   U = u;
   D = d;
   return true;
}

} // namespace ecm2
