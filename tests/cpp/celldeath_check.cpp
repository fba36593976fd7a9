// celldeath_check.cpp -- CPU check of the cell-death update (csrc/celldeath_math.hpp: the function the device
// kernel calls per entry), run by tests/test_celldeath_host.py under ASan + UBSan.
// Reads entries "model A1 dE1 A2 dE2 A3 dE3 t_offset T0 dT dt nsub N U D" (reals as C99 hex floats, or nan / inf)
// from stdin and prints one line per entry: the header's return value, the new N, U, D as hex floats, and their
// absolute errors against the closed form below evaluated in long double (Arrhenius model: Omega's error
// relative to max(1, Omega)).  The test applies the tolerance and the invariants.
//
// The closed form, per substep at frozen rates: the spectral form of the 2 x 2 block,
//   exp(A t) = (e^{lp t} (A - lm I) - e^{lm t} (A - lp I)) / (lp - lm) = e^{lm t} I + gq (A - lm I),
// gq = (e^{lp t} - e^{lm t}) / (lp - lm) taken through expm1l (the plain difference loses u / (2 delta t) near a
// double eigenvalue, in long double too), with D advanced by conservation, D += (N + U)_old - (N + U)_new -- a
// statement the header does not use: it never forms the integral of U.
#include "celldeath_math.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace
{
typedef long double ld;

void closed_form_substep(ld a, ld b, ld c, ld t, ld &N, ld &U, ld &D)
{
   const ld disc = (a - c) * (a - c) + b * b + 2 * b * (a + c);
   const ld two_delta = sqrtl(disc);
   const ld lm = -((a + b + c) + two_delta) / 2;
   const ld lp = lm != 0 ? a * c / lm : 0;
   const ld ep = expl(lp * t), em = expl(lm * t);
   // A - lm I = [[p, b], [a, q]] (p + q = 2 delta, p q = a b)
   const ld h = ((b + c) - a) / 2, big = fabsl(h) + two_delta / 2;
   const ld little = big != 0 ? a * b / big : 0;
   const ld p = h >= 0 ? big : little, q = h >= 0 ? little : big;
   const ld gq = two_delta != 0 ? ep * (-expm1l(-two_delta * t)) / two_delta : ep * t;
   const ld Nn = (em + gq * p) * N + gq * b * U;
   const ld Un = gq * a * N + (em + gq * q) * U;
   D += (N - Nn) + (U - Un);
   N = Nn;
   U = Un;
}

bool closed_form(const ecm2::CellDeathParams &P, double T0, double dT, double dt, int nsub, ld &N, ld &U, ld &D)
{
   const ld R = ecm2::kGasConstant, h = (ld)dt / nsub;
   ld n = N, u = U, d = D;
   for (int m = 0; m < nsub; m++)
   {
      const ld TK = ((ld)T0 + ((m + 0.5L) / nsub) * (ld)dT) + (ld)P.t_offset;
      if (!(TK > 0) || !std::isfinite((double)TK)) { return false; }
      ld k[3];
      for (int i = 0; i < 3; i++) { k[i] = (ld)P.A[i] * expl(-(ld)P.dE[i] / (R * TK)); }
      if (P.model == ecm2::CELLDEATH_THREE_STATE) { closed_form_substep(k[0], k[1], k[2], h, n, u, d); }
      else { u += h * k[0]; }
   }
   if (P.model != ecm2::CELLDEATH_THREE_STATE)
   {
      if (u == U) { return true; }
      const ld dn = -expm1l(-u);
      d = dn > D ? dn : D;
      n = 1 - d;
   }
   N = n;
   U = u;
   D = d;
   return true;
}
} // namespace

int main()
{
   char line[1024];
   int ncase = 0;
   while (std::fgets(line, sizeof line, stdin))
   {
      if (std::strncmp(line, "end", 3) == 0) { break; }
      double v[15];
      char *s = line;
      for (int i = 0; i < 15; i++)
      {
         char *e = nullptr;
         v[i] = std::strtod(s, &e);
         if (e == s)
         {
            std::fprintf(stderr, "bad entry line: %s", line);
            return 1;
         }
         s = e;
      }
      ecm2::CellDeathParams P;
      P.model = (int)v[0];
      for (int i = 0; i < 3; i++) { P.A[i] = v[1 + 2 * i]; P.dE[i] = v[2 + 2 * i]; }
      P.t_offset = v[7];
      const double T0 = v[8], dT = v[9], dt = v[10];
      const int nsub = (int)v[11];
      double N = v[12], U = v[13], D = v[14];
      ld Nr = N, Ur = U, Dr = D;
      const bool ok = ecm2::celldeath_update(P, T0, dT, dt, nsub, N, U, D);
      const bool okr = closed_form(P, T0, dT, dt, nsub, Nr, Ur, Dr);
      if (ok != okr)
      {
         std::fprintf(stderr, "validity differs from the closed form's: %s", line);
         return 1;
      }
      const ld us = P.model == ecm2::CELLDEATH_ARRHENIUS ? fmaxl(1.0L, fabsl(Ur)) : 1.0L;
      std::printf("%d %a %a %a %Le %Le %Le\n", ok ? 1 : 0, N, U, D, fabsl(N - Nr), fabsl(U - Ur) / us, fabsl(D - Dr));
      ncase++;
   }
   std::printf("cases %d\n", ncase);
   return 0;
}
