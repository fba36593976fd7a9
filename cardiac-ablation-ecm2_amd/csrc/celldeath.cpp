// celldeath.cpp -- host side of the cell-death state (celldeath.hpp): argument checks, workspace, launches.
#include "celldeath.hpp"

#include <cmath>

namespace ecm2
{

namespace
{
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// [a, a + n) and [b, b + n) share an entry
bool overlap(const double *a, const double *b, int n)
{
   const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * 8;
   return x < y + len && y < x + len;
}
} // namespace

CellDeath::CellDeath(int model, const double params[6], double t_offset, int n) : n_(n), parts_(0)
{
   ECM2_VERIFY(model == CELLDEATH_THREE_STATE || model == CELLDEATH_ARRHENIUS, ERR_ARG,
               "unknown cell-death model " << model);
   ECM2_VERIFY(params != nullptr, ERR_ARG, "null cell-death parameters");
   for (int i = 0; i < 6; i++)
   {
      ECM2_VERIFY(std::isfinite(params[i]) && params[i] >= 0.0, ERR_ARG,
                  "cell-death parameter " << i << " = " << params[i] << " is negative or not finite");
   }
   for (int i = 0; i < 3; i++)
   {
      ECM2_VERIFY(params[2 * i] <= kCellDeathMaxA, ERR_ARG,
                  "cell-death frequency factor A" << i + 1 << " = " << params[2 * i] << " exceeds " << kCellDeathMaxA);
   }
   ECM2_VERIFY(std::isfinite(t_offset), ERR_ARG, "cell-death t_offset is not finite");
   ECM2_VERIFY(n >= 1, ERR_ARG, "cell-death state of " << n << " entries");
   p_.model = model;
   for (int i = 0; i < 3; i++) { p_.A[i] = params[2 * i]; p_.dE[i] = params[2 * i + 1]; }
   p_.t_offset = t_offset;
   require_device();
   parts_ = kern::celldeath_parts(n);
   partials_.resize((size_t)3 * parts_);
   sums_.resize(3);
   count_.resize(1);
}

void CellDeath::step(const double *T0, const double *T1, double dt, int nsub, double *N, double *U, double *D,
                     int *invalid, hipStream_t s)
{
   ECM2_VERIFY(T0 && N && U && D, ERR_ARG, "cell-death step: null vector");
   ECM2_VERIFY(nsub >= 1, ERR_ARG, "cell-death step: nsub = " << nsub);
   ECM2_VERIFY(std::isfinite(dt) && dt >= 0.0, ERR_ARG, "cell-death step: dt = " << dt);
   ECM2_VERIFY(aligned16(T0) && aligned16(T1) && aligned16(N) && aligned16(U) && aligned16(D), ERR_ARG,
               "cell-death step: every vector must be 16-byte aligned (two entries per access)");
   ECM2_VERIFY(!overlap(N, U, n_) && !overlap(N, D, n_) && !overlap(U, D, n_), ERR_ARG,
               "cell-death step: N, U, D must be distinct vectors");
   for (const double *T : {T0, T1})
   {
      ECM2_VERIFY(!T || (!overlap(T, N, n_) && !overlap(T, U, n_) && !overlap(T, D, n_)), ERR_ARG,
                  "cell-death step: a temperature vector aliases a state vector");
   }
   kern::celldeath_step(n_, p_, T0, T1, dt, nsub, N, U, D, partials_.data(), s);
   if (invalid)
   {
      kern::celldeath_count(parts_, partials_.data(), count_.data(), s);
      ECM2_HIP(hipMemcpyAsync(invalid, count_.data(), sizeof(int), hipMemcpyDeviceToHost, s));
      ECM2_HIP(hipStreamSynchronize(s));
   }
}

void CellDeath::measure(const double *D, const double *w, double theta, double out[3], hipStream_t s)
{
   ECM2_VERIFY(D && w && out, ERR_ARG, "cell-death measure: null argument");
   ECM2_VERIFY(!std::isnan(theta), ERR_ARG, "cell-death measure: theta is NaN");
   ECM2_VERIFY(aligned16(D) && aligned16(w), ERR_ARG,
               "cell-death measure: D and w must be 16-byte aligned (two entries per access)");
   kern::celldeath_measure(n_, D, w, theta, partials_.data(), sums_.data(), s);
   ECM2_HIP(hipMemcpyAsync(out, sums_.data(), 3 * sizeof(double), hipMemcpyDeviceToHost, s));
   ECM2_HIP(hipStreamSynchronize(s));
}

} // namespace ecm2
