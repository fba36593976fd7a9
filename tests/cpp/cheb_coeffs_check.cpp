// cheb_coeffs_check.cpp -- CPU check of the Chebyshev smoother's coefficients (csrc/cheb_coeffs.hpp: the
// function the smoother's constructor calls), run by tests/test_cheb_host.py under ASan + UBSan.
// Reads cases "order max_eig" (max_eig as a C99 hex float) from stdin and prints one line per case: the
// status and the five coefficients as hex floats; the test compares them with tests/cheb_ref.py's
// coefficients.
#include "cheb_coeffs.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main()
{
   char line[256];
   int ncase = 0;
   while (std::fgets(line, sizeof line, stdin))
   {
      if (std::strncmp(line, "end", 3) == 0) { break; }
      char vs[64];
      int order = 0;
      if (std::sscanf(line, "%d %63s", &order, vs) != 2)
      {
         std::fprintf(stderr, "bad case line: %s", line);
         return 1;
      }
      double c[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};
      const int rc = ecm2::cheb_coeffs(order, std::strtod(vs, nullptr), c);
      std::printf("%d %a %a %a %a %a\n", rc, c[0], c[1], c[2], c[3], c[4]);
      ncase++;
   }
   std::printf("cases %d\n", ncase);
   return 0;
}
