// celldeath.hpp -- the cell-death state on the device (include/ecm2_pa.h, "Cell death"): the three-state kinetics
// N <-> U -> D with Arrhenius rates, advanced per dof by the exact propagator of a substep (celldeath_math.hpp,
// k_celldeath.hip), and the deterministic lesion measure.  The model is the application's, not the reference
// library's: the header states it, the tests pin it against an extended-precision restatement and closed forms.
#pragma once

#include "common.hpp"
#include "celldeath_math.hpp"

namespace ecm2
{

class CellDeath
{
public:
   // params: A1, dE1, A2, dE2, A3, dE3.  Checks its arguments (ERR_ARG) before it asks for a device (ERR_HIP).
   CellDeath(int model, const double params[6], double t_offset, int n);

   // One step of length dt in nsub substeps at T0 -> T1 (T1 null: T0 frozen); N, U, D in place.  All device
   // vectors of n entries, 16-byte aligned, T0 / T1 not overlapping a state vector, the state vectors distinct
   // (ERR_ARG before anything is enqueued).  invalid (host, optional): the number of entries left untouched
   // because T_K was non-finite or <= 0; reading it back synchronises the stream, null does not.
   void step(const double *T0, const double *T1, double dt, int nsub, double *N, double *U, double *D, int *invalid,
             hipStream_t s);
   // out (host) = sum w D, sum w [D >= theta], sum w in one pass, a fixed summation order; synchronises the stream.
   void measure(const double *D, const double *w, double theta, double out[3], hipStream_t s);

   const CellDeathParams &params() const { return p_; }
   int size() const { return n_; }

private:
   CellDeathParams p_;
   int n_, parts_;
   DeviceArray<double> partials_, sums_;  // 3 lists of parts_ partials; the final pass's results
   DeviceArray<int> count_;
};

namespace kern
{
// ---- kernels of the cell-death state (k_celldeath.hip) ----
// The partial lists' length for n entries (one partial per workgroup of the flat chunked grid = step_parts(n)).
int celldeath_parts(int n);
// celldeath_update on every entry, two per thread; partials[workgroup] = the workgroup's count of invalid entries.
void celldeath_step(int n, const CellDeathParams &p, const double *T0, const double *T1, double dt, int nsub,
                    double *N, double *U, double *D, double *partials, hipStream_t s);
// *count = the sum of the step's partials (one workgroup, a fixed order)
void celldeath_count(int nparts, const double *partials, int *count, hipStream_t s);
// sums[0..2] = sum w D, sum w [D >= theta], sum w: three partial lists (stride celldeath_parts(n)), then one
// workgroup sums each in a fixed order
void celldeath_measure(int n, const double *D, const double *w, double theta, double *partials, double *sums,
                       hipStream_t s);
} // namespace kern

} // namespace ecm2
