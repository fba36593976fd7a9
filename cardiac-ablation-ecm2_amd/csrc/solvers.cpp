// solvers.cpp -- see solvers.hpp.
#include "solvers.hpp"
#include "bicgstab_stop.hpp"
#include "cheb_coeffs.hpp"
#include "transfer.hpp"

#include <thread>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>

namespace ecm2
{

// ---------------------------------------------------------------------------------------
// loopback group as one operator
// ---------------------------------------------------------------------------------------
GroupOp::GroupOp(std::vector<ParPAForm *> forms) : forms_(std::move(forms))
{
   off_.assign(forms_.size() + 1, 0);
   for (size_t r = 0; r < forms_.size(); r++) { off_[r + 1] = off_[r] + forms_[r]->true_size(); }
   n_ = off_.back();
}

void GroupOp::mult(const double *x, double *y, hipStream_t s)
{
   std::vector<const double *> xs;
   std::vector<double *> ys;
   for (size_t r = 0; r < forms_.size(); r++)
   {
      xs.push_back(x + off_[r]);
      ys.push_back(y + off_[r]);
   }
   par_group_mult(forms_, xs, ys, s);
}

void GroupOp::diagonal(double *d, hipStream_t s)
{
   std::vector<double *> ds;
   for (size_t r = 0; r < forms_.size(); r++) { ds.push_back(d + off_[r]); }
   par_group_diagonal(forms_, ds, s);
}

MemberOp::MemberOp(std::vector<ParPAForm *> forms, int member) : forms_(std::move(forms)), member_(member)
{
   const int n = (int)forms_.size();
   ECM2_VERIFY(member >= 0 && member < n, ERR_ARG, "member " << member << " outside the group of " << n);
   // the peers' x live in this operator's own buffer, on which no group Mult runs: their packed sends
   // and (RAP) their ghost sums would be stale
   ECM2_VERIFY(forms_[member]->part().overlap, ERR_UNSUPPORTED, "a member operator needs the OVERLAP decomposition");
   for (ParPAForm *f : forms_)
   {
      ECM2_VERIFY(!f->pack_needed(), ERR_UNSUPPORTED, "a member operator needs contiguous sends (slabs)");
   }
   off_.assign(n + 1, 0);
   for (int r = 0; r < n; r++) { off_[r + 1] = off_[r] + forms_[r]->true_size(); }
   peers_.resize(std::max(off_.back(), 1));
   yscratch_.resize(std::max(off_.back(), 1));
   ECM2_HIP(hipMemset(peers_.data(), 0, peers_.size() * sizeof(double)));
}

void MemberOp::mult(const double *x, double *y, hipStream_t s)
{
   std::vector<const double *> xs;
   std::vector<double *> ys;
   for (size_t r = 0; r < forms_.size(); r++)
   {
      const bool me = (int)r == member_;
      xs.push_back(me ? x : peers_.data() + off_[r]);
      ys.push_back(me ? y : yscratch_.data() + off_[r]);
   }
   par_group_mult_member(forms_, xs, ys, member_, s);
}

void MemberOp::diagonal(double *d, hipStream_t s)
{
   std::vector<double *> ds;
   for (size_t r = 0; r < forms_.size(); r++) { ds.push_back(yscratch_.data() + off_[r]); }
   par_group_diagonal(forms_, ds, s);
   const int n = size();
   if (n) { ECM2_HIP(hipMemcpyAsync(d, ds[member_], n * sizeof(double), hipMemcpyDeviceToDevice, s)); }
}

// ---------------------------------------------------------------------------------------
// what the device-driven solvers share: the loop driver, the workspace, the constrained Mult, Jacobi
// ---------------------------------------------------------------------------------------
namespace
{
// The host side of a device-driven loop (kernels.hpp LoopCtl): the device state and its mapped pinned mirror
// (coherent: the host polls it while kernels run).  The only place that reads the mirror through volatile.
class LoopDriver
{
public:
   LoopDriver() : ctl_(1)
   {
      ECM2_HIP(hipHostMalloc(&mirror_, sizeof(kern::LoopCtl), hipHostMallocMapped | hipHostMallocCoherent));
      ECM2_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&mirror_dev_), mirror_, 0));
   }
   ~LoopDriver() { (void)hipHostFree(mirror_); }
   LoopDriver(const LoopDriver &) = delete;
   LoopDriver &operator=(const LoopDriver &) = delete;
   kern::LoopCtl *ctl() { return ctl_.data(); }        // the device state
   kern::LoopCtl *mirror() { return mirror_dev_; }     // the mirror, as the kernels address it
   // before a loop's first kernel is enqueued (no kernel of a previous solve writes the mirror any more:
   // SolverWork's invariant)
   void reset(hipStream_t s)
   {
      ECM2_HIP(hipMemsetAsync(ctl_.data(), 0, sizeof(kern::LoopCtl), s));
      *mirror_ = kern::LoopCtl{};
   }
   // Has the loop stopped at an iteration <= waited?  Waits until the tests of iteration `waited` have run,
   // without synchronising the stream; the host has enqueued nothing past `waited`.
   // "At an iteration <= waited", not "done != 0" alone: a stop found in the tail of `waited` carries iters =
   // waited + 1 (PCG: (A d, d) == 0 or not finite; BiCGSTAB: the next rho_1 == 0), and the PCG finds it in a
   // kernel that runs after the progress mark of `waited` -- whether done is already set when the host looks
   // is a matter of timing.  With the iteration in the predicate the answer is not: after such a stop every
   // caller enqueues iteration waited + 1 (each kernel of it returns at once) and stops at the next call, so
   // the ranks of a distributed operator issue the same collectives.  No result depends on it: what runs
   // after the loop (pcg_finish_x, bcg_finish_x) keys on the stop code.
   bool stopped_by(int waited, hipStream_t s, const char *solver_name)
   {
      const volatile kern::LoopCtl *m = mirror_;
      for (long spin = 1;; spin++)
      {
         // (the device writes iters and done before checked: a stop at `waited` is visible once checked says so)
         if (m->checked >= waited || m->done != 0) { return m->done != 0 && m->iters <= waited; }
         if (spin % 4096 == 0)
         {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess && m->checked < waited && m->done == 0)
            {
               ECM2_VERIFY(false, ERR_INTERNAL,
                           "device " << solver_name << " loop: stream idle before the tests of iteration " << waited);
            }
            if (e != hipSuccess && e != hipErrorNotReady) { ECM2_HIP(e); }
         }
         // back off after a short spin: the host core stays free for RCCL's
         // proxy and the other ranks' host threads while the device runs the iteration
         if (spin > 256) { std::this_thread::yield(); }
      }
   }
   // Has the loop stopped at all, a stop in the tail of the last enqueued iteration included?  Synchronises the
   // stream: for a caller whose next step synchronises anyway (pcg_loop before a cycle with a coarse PCG).
   bool stopped_after_sync(hipStream_t s)
   {
      ECM2_HIP(hipStreamSynchronize(s));
      const volatile kern::LoopCtl *m = mirror_;
      return m->done != 0;
   }
   // after the loop's last kernel: the stream synchronised, then done, iters and final
   kern::LoopCtl finish(hipStream_t s)
   {
      ECM2_HIP(hipStreamSynchronize(s));
      const volatile kern::LoopCtl *m = mirror_;
      kern::LoopCtl end{};
      end.done = m->done;
      end.iters = m->iters;
      end.final = m->final;
      return end;
   }

private:
   DeviceArray<kern::LoopCtl> ctl_;
   kern::LoopCtl *mirror_ = nullptr, *mirror_dev_ = nullptr;
};

// CGSolver's and BiCGSTABSolver's work vectors live across solves (CGSolver::SetOperator allocates them once,
// solvers.cpp:869-880; UpdateVectors, :1579-1604): one workspace per host thread and device for both methods,
// grown on demand.  Sharing it is safe because every solve ends with the stream synchronised -- the
// ERR_NUMERIC throws and the early returns included, each of which follows a synchronisation with nothing
// enqueued after it: when a solve starts, no kernel of the previous one reads a vector here or writes the
// loop's mirror.
struct SolverWork
{
   // by role: the residual, the direction (PCG's d), the operator's product (PCG's z = A d, BiCGSTAB's v)
   DeviceArray<double> r, p, ap;
   DeviceArray<double> rt, phat, t, shat;  // BiCGSTAB alone: r~, M^{-1} p, A shat, M^{-1} s (s lives in r's storage)
   DeviceArray<double> z, ct;              // the PCG with a smoother alone: z = B r and the smoother's running term
   DeviceArray<double> dinv, saved, partials, scal;  // Jacobi; the constrained Mult's ess entries; sums; PCG's scalars
   DeviceArray<kern::BcgScal> bcg;                   // BiCGSTAB's scalars
   double *hs = nullptr, *hs_dev = nullptr;  // mapped pinned scalar the final passes write a read-back value into
   LoopDriver loop;
   SolverWork() : scal(4)
   {
      ECM2_HIP(hipHostMalloc(&hs, sizeof(double), hipHostMallocMapped));
      ECM2_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&hs_dev), hs, 0));
   }
   ~SolverWork() { (void)hipHostFree(hs); }
   void ensure(int n, int n_ess, bool jacobi, bool bicgstab, size_t nparts, bool prec = false)
   {
      auto grow = [](DeviceArray<double> &a, size_t m) {
         if (a.size() < m) { a.resize(m); }
      };
      const size_t m = std::max(n, 1);
      for (DeviceArray<double> *a : {&r, &p, &ap}) { grow(*a, m); }
      if (bicgstab)
      {
         for (DeviceArray<double> *a : {&rt, &phat, &t}) { grow(*a, m); }
         if (jacobi) { grow(shat, m); }
         if (bcg.size() < 1) { bcg.resize(1); }
      }
      if (jacobi) { grow(dinv, m); }
      if (prec)
      {
         for (DeviceArray<double> *a : {&z, &ct}) { grow(*a, m); }
      }
      grow(saved, std::max(n_ess, 1));
      grow(partials, nparts);
   }
};

// One workspace (and so one LoopDriver) per host thread, device and nesting depth: a solve that runs inside
// another solve's loop -- the multigrid cycle's coarse PCG inside pcg_solve_mg -- is one level deeper and touches
// neither the outer solve's vectors nor its loop state.  Depth 0 is every solve that is not nested.
thread_local int g_solver_depth = 0;
struct NestedSolve
{
   NestedSolve() { g_solver_depth++; }
   ~NestedSolve() { g_solver_depth--; }
};

SolverWork &solver_work()
{
   static thread_local std::vector<std::vector<std::unique_ptr<SolverWork>>> per_device;
   int dev = 0;
   ECM2_HIP(hipGetDevice(&dev));
   if ((int)per_device.size() <= dev) { per_device.resize(dev + 1); }
   std::vector<std::unique_ptr<SolverWork>> &by_depth = per_device[dev];
   if ((int)by_depth.size() <= g_solver_depth) { by_depth.resize(g_solver_depth + 1); }
   if (!by_depth[g_solver_depth]) { by_depth[g_solver_depth].reset(new SolverWork()); }
   return *by_depth[g_solver_depth];
}

// ConstrainedOperator::ConstrainedMult, DIAG_ONE (operator.cpp:586-646): the input's ess entries are zeroed
// in place for the Mult and restored after (no vector copy); out[ess] = in[ess].  With `en` (an operator that
// folds its energy, LinOp::energy_parts() of them): the Mult's energy partials of the zeroed input at en, the
// essential rows' sum of in[ess]^2 behind them.
struct ConstrainedMult
{
   LinOp &A;
   const int *ess;
   int n_ess;
   double *saved;
   hipStream_t s;
   void operator()(double *in, double *out, double *en = nullptr) const
   {
      kern::ess_save_zero(n_ess, ess, in, saved, s);  // (n_ess == 0: neither kernel is launched)
      if (en) { A.mult_energy(in, out, en, s); }
      else { A.mult(in, out, s); }
      kern::ess_restore(n_ess, ess, saved, in, out, s, en ? en + A.energy_parts() : nullptr);
   }
};

// OperatorJacobiSmoother on the constrained operator: dinv = 1 / diag(D), the essential rows' diag 1
void jacobi_dinv(LinOp &D, const int *ess, int n_ess, double *scratch, double *dinv, hipStream_t s)
{
   D.diagonal(scratch, s);
   if (n_ess) { kern::set_values(n_ess, ess, 1.0, scratch, s); }
   kern::reciprocal(D.size(), scratch, dinv, s);
}
} // namespace

// ---------------------------------------------------------------------------------------
// ConstrainedOperator + CGSolver, prec = none | OperatorJacobiSmoother | OperatorChebyshevSmoother | Multigrid
// ---------------------------------------------------------------------------------------
namespace
{
// One solve's operator, vectors and device scalars, as the loop and its preconditioner see them.
struct PcgState
{
   LinOp &A;
   const int *ess;
   int n_ess, n;
   // serial: the final-dot kernel also writes the value into mapped pinned memory and runs the stopping test;
   // distributed: the value is copied after the all-reduce, the test is a kernel of its own (pcg_check)
   bool direct;
   SolverWork &w;
   hipStream_t s;
   double *x, *r, *d, *ap, *partials;    // the caller's x; the residual, the direction, A d (SolverWork's r, p, ap)
   double *nom, *den, *betanom, *alpha;  // device scalars; nom and betanom swap roles every iteration (no copy)
   kern::LoopCtl *ctl;
   void copy(double *dst, const double *src) const
   {
      if (n) { ECM2_HIP(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, s)); }
   }
   // the residual step's arguments up to what follows the update, which the preconditioner fills
   kern::PcgStepR step_r() const { return kern::PcgStepR{n, nom, den, ap, r, alpha, ctl}; }
};

// What differs between CGSolver's preconditioners B: how z = B r enters an iteration, and which direction update
// consumes it.  Everything else is pcg_loop.
struct PcgPrec
{
   // what the solve needs from SolverWork::ensure: dinv; z and the smoother's term; room on `saved` for the
   // essential entries of the preconditioner's own constrained Mult
   bool jacobi = false, stored_z = false;
   int n_ess = 0;
   // applying it synchronises the stream and may raise (the cycle with a coarse PCG)
   bool syncs = false;
   virtual void setup(PcgState &) {}        // once, before r = b is enqueued
   virtual void first(PcgState &p) = 0;     // d = B r
   // the residual half of an iteration: r -= alpha A d, betanom = (r, B r) and its test
   virtual void step_r(PcgState &p, const kern::PcgStop &stop) = 0;
   virtual void update_xd(PcgState &p) = 0;  // the direction half: x += alpha d, d = B r + beta d

protected:
   ~PcgPrec() = default;
};

// CGSolver::Mult (solvers.cpp:869-1004) on the constrained A; x overwritten, or with iterative_mode the start.
PCGResult pcg_loop(LinOp &A, PcgPrec &B, const int *ess, int n_ess, const double *b, double *x, double rel_tol,
                   double abs_tol, int max_iter, hipStream_t s, bool iterative_mode)
{
   // the update passes and k_pcg_finish_x read and write the caller's x two entries at a time; refused here,
   // before anything is allocated or enqueued (the work vectors are allocations of their own)
   ECM2_VERIFY(((uintptr_t)x % 16) == 0, ERR_ARG, "PCG: x must be 16-byte aligned (got " << (const void *)x << ")");
   // (iterative_mode: the residual pass reads b two entries at a time)
   ECM2_VERIFY(!iterative_mode || ((uintptr_t)b % 16) == 0, ERR_ARG,
               "PCG: with iterative_mode b must be 16-byte aligned (got " << (const void *)b << ")");
   const int n = A.size();
   PCGResult res;
   const bool direct = !A.distributed();
   // den = (A d, d) folded into the Mult where the operator can (serial snapshot forms): the
   // kernel's element energies sum_e d~_e . A_e d~_e (d~ = d with the ess entries zeroed, as the
   // constrained Mult sees it) plus the DIAG_ONE rows' sum_ess d_i^2 -- the same value as the dot of
   // d and A d up to the summation order -- one partial per workgroup, summed in a fixed order by
   // dot_final: no pass over the two vectors (2 streams and a launch per iteration).
   const int nen = direct ? A.energy_parts() : 0;
   SolverWork &w = solver_work();
   w.ensure(n, std::max(n_ess, B.n_ess), B.jacobi, false,
            std::max({kern::kDotPartials, kern::step_parts(n), nen + kern::ess_parts(n_ess)}), B.stored_z);
   double *const scal = w.scal.data();
   PcgState p{A, ess, n_ess, n, direct, w, s, x, w.r.data(), w.p.data(), w.ap.data(), w.partials.data(),
              scal, scal + 1, scal + 2, scal + 3, w.loop.ctl()};
   auto readback = [&](const double *dv) {
      if (!direct) { ECM2_HIP(hipMemcpyAsync(w.hs, dv, sizeof(double), hipMemcpyDeviceToHost, s)); }
      ECM2_HIP(hipStreamSynchronize(s));
      return *(volatile double *)w.hs;
   };
   const ConstrainedMult cmult{A, ess, n_ess, w.saved.data(), s};
   // ap = A d, den = (A d, d); in the loop (c) with its test, before it with the value for the read-back
   auto cmult_den = [&](const kern::LoopCtl *c, const kern::PcgStop *stop) {
      if (nen > 0)
      {
         cmult(p.d, p.ap, p.partials);
         kern::dot_final(nen + kern::ess_parts(n_ess), p.partials, p.den, s, c, stop, c ? nullptr : w.hs_dev);
         return;
      }
      cmult(p.d, p.ap);
      kern::dot(n, p.d, p.ap, p.partials, p.den, s, direct && !c ? w.hs_dev : nullptr, c, direct ? stop : nullptr);
      if (!direct)
      {
         A.sum_scalars(p.den, 1, s);
         if (stop) { kern::pcg_check(p.den, *stop, s); }
      }
   };
   B.setup(p);
   if (iterative_mode)
   {
      // r = b - A~ x (solvers.cpp:875-884): the constrained Mult zeroes and restores the essential entries of the
      // caller's x in place; x is not cleared
      cmult(x, p.ap);
      kern::pcg_residual(n, b, p.ap, p.r, s);
   }
   else
   {
      p.copy(p.r, b);
      if (n) { ECM2_HIP(hipMemsetAsync(x, 0, sizeof(double) * n, s)); }
   }
   // d = B r, nom = (d, r) (solvers.cpp:893-903)
   B.first(p);
   kern::dot(n, p.d, p.r, p.partials, p.nom, s, direct ? w.hs_dev : nullptr);
   if (!direct) { A.sum_scalars(p.nom, 1, s); }
   // Every return below follows a read-back (or finish()) with nothing enqueued after it: the stream is
   // synchronised, which is SolverWork's invariant.
   const double nom0 = readback(p.nom);
   // CGSolver::Mult's checks before the loop (solvers.cpp:893-948)
   ECM2_VERIFY(std::isfinite(nom0), ERR_NUMERIC, "PCG: nom = " << nom0);
   res.initial_norm = nom0 >= 0 ? std::sqrt(nom0) : nom0;
   res.final_norm = res.initial_norm;
   // the preconditioner is not positive definite (a smoother whose estimate is far below the largest eigenvalue,
   // a cycle of such smoothers): not converged, final_norm = nom (:905-917)
   if (nom0 < 0.0) { return res; }
   const double r0 = std::max(nom0 * rel_tol * rel_tol, abs_tol * abs_tol);
   if (nom0 <= r0)
   {
      res.converged = true;
      return res;
   }
   // the device-driven loop's state, reset before the read-back below idles the stream
   w.loop.reset(s);
   cmult_den(nullptr, nullptr);
   const double den0 = readback(p.den);
   ECM2_VERIFY(std::isfinite(den0), ERR_NUMERIC, "PCG: den = " << den0);
   if (den0 == 0.0) { return res; }
   // CGSolver's loop (solvers.cpp:930-1000) driven by the device: the stopping tests run on the device after each
   // (r, B r) and each (A d, d) (in the dot's final pass, or in a one-thread kernel after the all-reduce), and once
   // one stops every later vector kernel of the loop returns at once.  The host enqueues iteration i as soon as the
   // betanom test of i - 1 has run (it polls the mirror's progress mark; no host synchronisation of the stream), so
   // the queue holds the rest of iteration i - 1 while it does, and it ends at the iteration the device stopped
   // at: the same iteration on every rank, so the ranks issue the same collectives.  The iterates are CGSolver's
   // (the same operations per entry, in its order; x += alpha d deferred into the next pass that reads d); at
   // most the stopping iteration's Mult runs after the stop.  The order of events around a stop:
   //  1. stopped_by(i - 1) answers for the stops found up to the betanom test of i - 1.  A stop the device finds
   //     after that, in the (A d, d) test of i - 1's tail, carries iters = i and may not be visible yet, so the
   //     host may enqueue iteration i once more; the loop's own kernels (step_r's, update_xd's, the Mult's test)
   //     return at once.
   //  2. A preconditioner's own kernels (the smoother's Mults, the cycle) are not keyed on the loop state.  One
   //     that is enqueued in such an iteration runs on the unchanged r and writes z and its own vectors, which
   //     nothing after the loop reads (pcg_finish_x reads alpha, d and x): the result cannot change, and it has no
   //     host-side check that could raise.
   //  3. A preconditioner that synchronises (B.syncs: the cycle with a coarse PCG, whose inner solve reads back
   //     and verifies its own scalars) is different.  Before applying it the host synchronises and looks at the
   //     loop's state itself: after any stop, the tail's included, it is not applied again, so an inner solve can
   //     neither run on a stopped loop's vectors nor raise over the outer loop's own stop, which finish() reports
   //     below.  While the outer loop runs, the inner solve works one nesting level down (its own SolverWork and
   //     LoopDriver) and ends with the stream synchronised.
   for (int i = 1;; i++)
   {
      if (i > 1 && w.loop.stopped_by(i - 1, s, "PCG")) { break; }
      if (i > 1 && B.syncs && w.loop.stopped_after_sync(s)) { break; }
      const kern::PcgStop stop{r0, i, max_iter, p.ctl, w.loop.mirror()};
      B.step_r(p, stop);
      if (i >= max_iter) { break; }
      B.update_xd(p);
      // ap = A d, den = (A d, d) and its test (after ++i: final_iter = i + 1 on a den == 0 stop)
      const kern::PcgStop dstop{r0, i + 1, max_iter, p.ctl, w.loop.mirror(), p.betanom, 1};
      cmult_den(p.ctl, &dstop);
      std::swap(p.nom, p.betanom);  // nom <- betanom
   }
   // the stopping iteration's x += alpha d (a betanom stop)
   kern::pcg_finish_x(n, p.alpha, p.d, x, s, p.ctl);
   const kern::LoopCtl end = w.loop.finish(s);
   ECM2_VERIFY(end.done != kern::PCG_RUNNING, ERR_INTERNAL, "device PCG loop ended without a stop");
   const double bn = end.final;
   ECM2_VERIFY(end.done != kern::PCG_NONFINITE, ERR_NUMERIC,
               "PCG: non-finite (B r, r) or (A d, d) at iteration " << end.iters << " (" << bn << ")");
   res.final_norm = bn >= 0 ? std::sqrt(bn) : bn;
   res.iterations = end.iters;
   res.converged = end.done == kern::PCG_CONVERGED;
   return res;
}

// OperatorJacobiSmoother, or none (dinv null): z is never stored, dinv is applied inside the two fused passes
struct JacobiPrec final : PcgPrec
{
   double *dinv = nullptr;
   explicit JacobiPrec(bool on) { jacobi = on; }
   void setup(PcgState &p) override
   {
      if (!jacobi) { return; }
      dinv = p.w.dinv.data();
      jacobi_dinv(p.A, p.ess, p.n_ess, p.ap, dinv, p.s);
   }
   void first(PcgState &p) override
   {
      if (dinv) { kern::pcg_precond(p.n, dinv, p.r, p.ap, p.s); }
      p.copy(p.d, dinv ? p.ap : p.r);
   }
   void step_r(PcgState &p, const kern::PcgStop &stop) override
   {
      // r -= alpha A d, betanom = r.(M^{-1} r) in one pass, its test
      kern::PcgStepR a = p.step_r();
      a.after = kern::PCG_STEP_JACOBI;
      a.dinv = dinv;
      a.partials = p.partials;
      kern::pcg_step_r(a, p.s);
      kern::dot_final(kern::kDotPartials, p.partials, p.betanom, p.s, p.ctl, p.direct ? &stop : nullptr);
      if (!p.direct)
      {
         p.A.sum_scalars(p.betanom, 1, p.s);
         kern::pcg_check(p.betanom, stop, p.s);
      }
   }
   // x += alpha d, d = M^{-1} r + beta d
   void update_xd(PcgState &p) override { kern::pcg_update_xd(p.n, p.nom, p.den, p.betanom, p.x, p.d, p.r, dinv, p.s, p.ctl); }
};

// The smoother and the cycle: z = B r is a vector of its own (SolverWork's z), serial operators only
template <class Prec>
struct StoredPrec : PcgPrec
{
   Prec &B;
   explicit StoredPrec(Prec &b) : B(b) { stored_z = true; }
   void first(PcgState &p) override
   {
      B.mult(p.r, p.w.z.data(), p.s);
      p.copy(p.d, p.w.z.data());
   }
   // x += alpha d, d = z + beta d
   void update_xd(PcgState &p) override { kern::pcg_update_xd_z(p.n, p.nom, p.den, p.betanom, p.x, p.d, p.w.z.data(), p.s, p.ctl); }
};

// OperatorChebyshevSmoother: its first term in the pass that updates r, its last in the pass that sums (r, z)
struct ChebPrec final : StoredPrec<ChebyshevSmoother>
{
   explicit ChebPrec(ChebyshevSmoother &b) : StoredPrec(b) { n_ess = b.n_ess(); }
   void step_r(PcgState &p, const kern::PcgStop &stop) override
   {
      const int order = B.order();
      const double *c = B.coeffs(), *dinv = B.dinv();
      // ap holds A d until the entry pass has consumed it, then the smoother's A~ t
      double *z = p.w.z.data(), *t = p.w.ct.data();
      const ConstrainedMult bmult{B.op(), B.ess(), B.n_ess(), p.w.saved.data(), p.s};
      // r -= alpha A d and the smoother's first term: t = dinv .* r, z = c_0 t
      kern::PcgStepR a = p.step_r();
      a.after = kern::PCG_STEP_CHEB;
      a.dinv = dinv;
      a.partials = p.partials;
      a.c0 = c[0];
      a.t = order > 1 ? t : nullptr;
      a.z = z;
      a.sum = order == 1;
      kern::pcg_step_r(a, p.s);
      // its further terms: t = dinv .* (A~ t), z += c_k t; the last one sums betanom = (r, z)
      for (int k = 1; k < order; k++)
      {
         const bool last = k + 1 == order;
         bmult(t, p.ap);
         kern::cheb_accum(p.n, dinv, p.ap, c[k], last ? nullptr : t, z, p.s, last ? p.r : nullptr, p.partials, p.ctl);
      }
      kern::dot_final(kern::kDotPartials, p.partials, p.betanom, p.s, p.ctl, &stop);
   }
};

// Multigrid: one cycle between the pass that updates r and the pass that sums (r, z)
struct MgPrec final : StoredPrec<Multigrid>
{
   explicit MgPrec(Multigrid &b) : StoredPrec(b) { syncs = b.coarse_pcg(); }
   void step_r(PcgState &p, const kern::PcgStop &stop) override
   {
      kern::pcg_step_r(p.step_r(), p.s);  // r -= alpha A d (PCG_STEP_ONLY)
      B.mult(p.r, p.w.z.data(), p.s);
      kern::dot(p.n, p.r, p.w.z.data(), p.partials, p.betanom, p.s, nullptr, p.ctl, &stop);  // betanom = (r, z), its test
   }
};
} // namespace

PCGResult pcg_solve(LinOp &A, const int *ess, int n_ess, const double *b, double *x, double rel_tol,
                    double abs_tol, int max_iter, bool jacobi, hipStream_t s, bool iterative_mode)
{
   JacobiPrec B(jacobi);
   return pcg_loop(A, B, ess, n_ess, b, x, rel_tol, abs_tol, max_iter, s, iterative_mode);
}

PCGResult pcg_solve(PAForm &A, const int *ess, int n_ess, const double *b, double *x, double rel_tol,
                    double abs_tol, int max_iter, bool jacobi, hipStream_t s)
{
   FormOp op(A);
   return pcg_solve(op, ess, n_ess, b, x, rel_tol, abs_tol, max_iter, jacobi, s);
}

PCGResult pcg_solve_prec(LinOp &A, ChebyshevSmoother &S, const int *ess, int n_ess, const double *b, double *x,
                         double rel_tol, double abs_tol, int max_iter, hipStream_t s, bool iterative_mode)
{
   ECM2_VERIFY(!A.distributed(), ERR_UNSUPPORTED, "PCG with a Chebyshev smoother: distributed operators are not supported");
   ECM2_VERIFY(S.size() == A.size(), ERR_ARG, "PCG: the smoother has size " << S.size() << ", the operator " << A.size());
   ChebPrec B(S);
   return pcg_loop(A, B, ess, n_ess, b, x, rel_tol, abs_tol, max_iter, s, iterative_mode);
}

PCGResult pcg_solve_mg(LinOp &A, Multigrid &M, const int *ess, int n_ess, const double *b, double *x, double rel_tol,
                       double abs_tol, int max_iter, hipStream_t s, bool iterative_mode)
{
   ECM2_VERIFY(!A.distributed(), ERR_UNSUPPORTED, "PCG with a multigrid cycle: distributed operators are not supported");
   ECM2_VERIFY(!A.concatenated(), ERR_UNSUPPORTED,
               "PCG with a multigrid cycle: a loopback group's vectors are not in the cycle's numbering");
   ECM2_VERIFY(M.size() == A.size(), ERR_ARG,
               "PCG: the multigrid's finest level has size " << M.size() << ", the operator " << A.size());
   MgPrec B(M);
   return pcg_loop(A, B, ess, n_ess, b, x, rel_tol, abs_tol, max_iter, s, iterative_mode);
}

// ---------------------------------------------------------------------------------------
// ConstrainedOperator + BiCGSTABSolver + OperatorJacobiSmoother(second operator)
// ---------------------------------------------------------------------------------------
PCGResult bicgstab_solve(LinOp &A, LinOp *jacobi_of, const int *ess, int n_ess, const double *b, double *x,
                         double rel_tol, double abs_tol, int max_iter, hipStream_t s, bool iterative_mode)
{
   // refused before anything is enqueued: k_bcg_update_xr reads and writes the caller's x two entries at a time
   ECM2_VERIFY(((uintptr_t)x % 16) == 0, ERR_ARG,
               "BiCGSTAB: x must be 16-byte aligned (got " << (const void *)x << ")");
   ECM2_VERIFY(!iterative_mode || ((uintptr_t)b % 16) == 0, ERR_ARG,
               "BiCGSTAB: with iterative_mode b must be 16-byte aligned (got " << (const void *)b << ")");
   ECM2_VERIFY(!A.distributed(), ERR_UNSUPPORTED,
               "BiCGSTAB: distributed operators are not supported (no distributed form carries the convection term)");
   const int n = A.size();
   ECM2_VERIFY(!jacobi_of || jacobi_of->size() == n, ERR_ARG,
               "BiCGSTAB: the preconditioner's operator has size " << jacobi_of->size() << ", the operator " << n);
   PCGResult res;
   SolverWork &w = solver_work();
   const bool jacobi = jacobi_of != nullptr;
   w.ensure(n, n_ess, jacobi, true, 2 * (size_t)kern::bcg_parts(n));
   double *r = w.r.data(), *rt = w.rt.data(), *p = w.p.data(), *phat = w.phat.data(), *v = w.ap.data(), *t = w.t.data();
   double *dinv = jacobi ? w.dinv.data() : nullptr, *shat = jacobi ? w.shat.data() : nullptr;
   double *partials = w.partials.data();
   kern::BcgScal *sc = w.bcg.data();
   kern::LoopCtl *ctl = w.loop.ctl();
   // the loop's state, reset first
   w.loop.reset(s);
   ECM2_HIP(hipMemsetAsync(sc, 0, sizeof(kern::BcgScal), s));
   const ConstrainedMult cmult{A, ess, n_ess, w.saved.data(), s};
   if (jacobi) { jacobi_dinv(*jacobi_of, ess, n_ess, t, dinv, s); }
   // iterative_mode: r = b - A~ x, r~ = r (solvers.cpp:1618-1622; v is free until the loop's first Mult)
   if (iterative_mode)
   {
      cmult(x, v);
      kern::pcg_residual(n, b, v, r, s);
      if (n) { ECM2_HIP(hipMemcpyAsync(rt, r, sizeof(double) * n, hipMemcpyDeviceToDevice, s)); }
   }
   // x = 0, r = b, r~ = r (solvers.cpp:1623-1628)
   else if (n)
   {
      ECM2_HIP(hipMemsetAsync(x, 0, sizeof(double) * n, s));
      ECM2_HIP(hipMemcpyAsync(r, b, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
      ECM2_HIP(hipMemcpyAsync(rt, b, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
   }
   // (r~, r) = ||r_0||^2 is also iteration 1's rho_1, summed by the pass that sums (r~, v)
   kern::BcgFinal fin;
   fin.ctl = ctl;
   fin.host = w.loop.mirror();
   fin.sc = sc;
   fin.max_iter = max_iter;
   fin.mode = kern::BCG_FINAL_DOT;
   fin.out = &sc->rho1;
   fin.hout = w.hs_dev;
   kern::bcg_dot(n, rt, r, nullptr, partials, fin, s);
   ECM2_HIP(hipStreamSynchronize(s));
   const double nrm0 = *(volatile double *)w.hs;
   const double resid0 = nrm0 >= 0 ? std::sqrt(nrm0) : nrm0;
   // the reference's checks before the loop (solvers.cpp:1630-1648)
   const double tol_goal = std::max(resid0 * rel_tol, abs_tol);
   const int start = bcg_stop(BCG_TEST_R0, resid0, tol_goal, 0, max_iter);
   ECM2_VERIFY(start != BCG_NONFINITE, ERR_NUMERIC, "BiCGSTAB: resid = " << resid0);
   res.initial_norm = res.final_norm = resid0;
   if (start == BCG_CONVERGED)
   {
      res.converged = true;
      return res;
   }
   if (max_iter < 1) { return res; }  // (the loop does not run: not converged, final_norm = ||r_0||)
   fin.tol_goal = tol_goal;
   fin.hout = nullptr;
   // BiCGSTABSolver's loop (solvers.cpp:1650-1784) driven by the device: the host enqueues iteration i as
   // soon as the last test of i - 1 has run (it polls the mirror's progress mark; no host synchronisation
   // of the stream) and ends at the iteration the device stopped at; at most the stopping iteration's
   // Mults run after the stop (a rho_1 == 0 stop carries the next iteration's number: that iteration's too).
   for (int i = 1;; i++)
   {
      if (i > 1 && w.loop.stopped_by(i - 1, s, "BiCGSTAB")) { break; }
      fin.it = i;
      // p, phat
      kern::bcg_update_p(n, i, sc, p, v, r, dinv, phat, ctl, s);
      // v = A phat, (r~, v)
      cmult(phat, v);
      fin.mode = kern::BCG_FINAL_DOT;
      fin.out = &sc->rtv;
      kern::bcg_dot(n, rt, v, nullptr, partials, fin, s);
      // alpha, s, shat, ||s|| and its test
      fin.mode = kern::BCG_FINAL_S;
      kern::bcg_update_s(n, sc, r, v, dinv, shat, partials, fin, s);
      // t = A shat, (t, s) and (t, t)
      cmult(shat ? shat : r, t);
      fin.mode = kern::BCG_FINAL_DOT2;
      kern::bcg_dot(n, t, r, t, partials, fin, s);
      // omega, x, r, ||r|| and (r~, r) with the tests of ||r||, omega, max_iter and the next rho_1
      fin.mode = kern::BCG_FINAL_R;
      kern::bcg_update_xr(n, sc, x, phat, shat, r, t, rt, partials, fin, s);
      if (i >= max_iter) { break; }
   }
   // the stopping iteration's x += alpha phat (a ||s|| stop)
   kern::bcg_finish_x(n, sc, phat, x, ctl, s);
   const kern::LoopCtl end = w.loop.finish(s);
   ECM2_VERIFY(end.done != BCG_RUNNING, ERR_INTERNAL, "device BiCGSTAB loop ended without a stop");
   ECM2_VERIFY(end.done != BCG_NONFINITE, ERR_NUMERIC,
               "BiCGSTAB: resid = " << end.final << " at iteration " << end.iters);
   res.final_norm = end.final;
   res.iterations = end.iters;
   res.converged = bcg_converged(end.done);
   return res;
}

// ---------------------------------------------------------------------------------------
// PowerMethod + OperatorChebyshevSmoother + CGSolver(prec = the smoother)
// ---------------------------------------------------------------------------------------
static_assert(kChebOk == OK && kChebErrArg == ERR_ARG, "cheb_coeffs.hpp restates Status");

PowerResult power_method(LinOp &A, const double *dinv, const int *ess, int n_ess, double *v0, int num_steps,
                         double tol, hipStream_t s)
{
   ECM2_VERIFY(!A.distributed(), ERR_UNSUPPORTED, "power method: distributed operators are not supported");
   ECM2_VERIFY(((uintptr_t)v0 % 16) == 0, ERR_ARG, "power method: v0 must be 16-byte aligned (got " << (const void *)v0 << ")");
   const int n = A.size();
   SolverWork &w = solver_work();
   w.ensure(n, n_ess, false, false, std::max(2 * kern::kDotPartials, kern::step_parts(n)));
   // EstimateLargestEigenvalue's v0, v1 (operator.cpp:875-879) and h = A~ v0
   double *va = v0 ? v0 : w.r.data(), *vb = w.p.data(), *h = w.ap.data();
   double *partials = w.partials.data(), *norm = w.scal.data(), *v0v1 = w.scal.data() + 1;
   const ConstrainedMult cmult{A, ess, n_ess, w.saved.data(), s};
   if (!v0) { kern::cheb_fill_hash(n, va, s); }
   kern::dot(n, va, va, partials, norm, s);
   PowerResult res;
   for (int iter = 0; iter < num_steps; iter++)
   {
      kern::cheb_scale(n, norm, va, s);
      cmult(va, h);
      // v1 = D^-1 A~ v0, (v0, v1) and the next step's (v1, v1) in one sweep
      kern::cheb_power_pass(n, dinv, h, va, vb, partials, s);
      kern::dot_final(kern::kDotPartials, partials, v0v1, s, nullptr, nullptr, w.hs_dev);
      kern::dot_final(kern::kDotPartials, partials + kern::kDotPartials, norm, s);
      ECM2_HIP(hipStreamSynchronize(s));
      const double eig_new = *(volatile double *)w.hs;
      ECM2_VERIFY(std::isfinite(eig_new), ERR_NUMERIC, "power method: eigenvalue = " << eig_new << " at step " << iter + 1);
      const double diff = std::abs((eig_new - res.eig) / res.eig);
      res.eig = eig_new;
      res.steps = iter + 1;
      std::swap(va, vb);
      if (diff < tol) { break; }
   }
   if (v0 && va != v0 && n) { ECM2_HIP(hipMemcpyAsync(v0, va, sizeof(double) * n, hipMemcpyDeviceToDevice, s)); }
   ECM2_HIP(hipStreamSynchronize(s));
   return res;
}

PowerResult power_method(LinOp &A, LinOp *diag_of, const int *ess, int n_ess, double *v0, int num_steps, double tol,
                         hipStream_t s)
{
   LinOp &D = diag_of ? *diag_of : A;
   ECM2_VERIFY(D.size() == A.size(), ERR_ARG,
               "power method: the diagonal's operator has size " << D.size() << ", the operator " << A.size());
   ECM2_VERIFY(!A.distributed() && !D.distributed(), ERR_UNSUPPORTED,
               "power method: distributed operators are not supported");
   // (checked again below; here before the diagonal is enqueued)
   ECM2_VERIFY(((uintptr_t)v0 % 16) == 0, ERR_ARG, "power method: v0 must be 16-byte aligned (got " << (const void *)v0 << ")");
   DeviceArray<double> scratch(std::max(A.size(), 1)), dinv(std::max(A.size(), 1));
   jacobi_dinv(D, ess, n_ess, scratch.data(), dinv.data(), s);
   return power_method(A, dinv.data(), ess, n_ess, v0, num_steps, tol, s);  // (ends synchronised)
}

void ChebyshevSmoother::setup(LinOp *diag_of, const int *ess_dev, hipStream_t s)
{
   // refused before anything is allocated or enqueued
   ECM2_VERIFY(order_ >= 1 && order_ <= kChebMaxOrder, ERR_ARG,
               "Chebyshev smoother not implemented for order = " << order_ << " (1.." << kChebMaxOrder << ")");
   ECM2_VERIFY(n_ess_ >= 0 && (n_ess_ == 0 || ess_dev), ERR_ARG, "Chebyshev smoother: null essential dof list");
   LinOp &D = diag_of ? *diag_of : A_;
   ECM2_VERIFY(D.size() == n_, ERR_ARG,
               "Chebyshev smoother: the diagonal's operator has size " << D.size() << ", the operator " << n_);
   ECM2_VERIFY(!A_.distributed() && !D.distributed(), ERR_UNSUPPORTED,
               "Chebyshev smoother: distributed operators are not supported");
   const size_t m = std::max(n_, 1);
   dinv_.resize(m);
   t_.resize(m);
   h_.resize(m);
   saved_.resize(std::max(n_ess_, 1));
   ess_.resize(std::max(n_ess_, 1));
   if (n_ess_) { ECM2_HIP(hipMemcpyAsync(ess_.data(), ess_dev, sizeof(int) * n_ess_, hipMemcpyDeviceToDevice, s)); }
   jacobi_dinv(D, ess_.data(), n_ess_, h_.data(), dinv_.data(), s);
}

ChebyshevSmoother::ChebyshevSmoother(LinOp &A, LinOp *diag_of, const int *ess_dev, int n_ess, int order,
                                     double max_eig_estimate, hipStream_t s)
   : A_(A), n_(A.size()), n_ess_(n_ess), order_(order), max_eig_(max_eig_estimate)
{
   ECM2_VERIFY(std::isfinite(max_eig_) && max_eig_ != 0.0, ERR_ARG, "Chebyshev smoother: max_eig_estimate = " << max_eig_);
   setup(diag_of, ess_dev, s);
   ECM2_VERIFY(cheb_coeffs(order_, max_eig_, coeffs_) == kChebOk, ERR_ARG, "Chebyshev smoother: order " << order_);
   ECM2_HIP(hipStreamSynchronize(s));
}

ChebyshevSmoother::ChebyshevSmoother(LinOp &A, LinOp *diag_of, const int *ess_dev, int n_ess, int order,
                                     int power_iterations, double power_tolerance, double *v0, hipStream_t s)
   : A_(A), n_(A.size()), n_ess_(n_ess), order_(order)
{
   // (power_method's own check, made here before setup() allocates and enqueues)
   ECM2_VERIFY(((uintptr_t)v0 % 16) == 0, ERR_ARG,
               "Chebyshev smoother: v0 must be 16-byte aligned (got " << (const void *)v0 << ")");
   setup(diag_of, ess_dev, s);
   const PowerResult pr = power_method(A_, dinv_.data(), ess_.data(), n_ess_, v0, power_iterations, power_tolerance, s);
   max_eig_ = pr.eig;
   power_steps_ = pr.steps;
   ECM2_VERIFY(max_eig_ != 0.0, ERR_NUMERIC, "Chebyshev smoother: the power method's estimate is 0");
   ECM2_VERIFY(cheb_coeffs(order_, max_eig_, coeffs_) == kChebOk, ERR_ARG, "Chebyshev smoother: order " << order_);
}

void ChebyshevSmoother::mult(const double *x, double *y, hipStream_t s)
{
   ECM2_VERIFY(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, ERR_ARG,
               "Chebyshev smoother: x and y must be 16-byte aligned (got " << (const void *)x << ", " << (const void *)y << ")");
   ECM2_VERIFY(x != y, ERR_ARG, "Chebyshev smoother: x and y must be distinct");
   const ConstrainedMult cmult{A_, ess_.data(), n_ess_, saved_.data(), s};
   double *t = t_.data(), *h = h_.data();
   // OperatorChebyshevSmoother::Mult (solvers.cpp:631-657): the term t <- dinv .* (A~ t), y += c_k t
   kern::cheb_first(n_, dinv_.data(), x, coeffs_[0], order_ > 1 ? t : nullptr, y, s);
   for (int k = 1; k < order_; k++)
   {
      cmult(t, h);
      kern::cheb_accum(n_, dinv_.data(), h, coeffs_[k], k + 1 < order_ ? t : nullptr, y, s);
   }
}

// ---------------------------------------------------------------------------------------
// Multigrid (V-cycle over caller-supplied levels) + CGSolver(prec = the cycle)
// ---------------------------------------------------------------------------------------
Multigrid::Multigrid(const std::vector<LinOp *> &ops, const std::vector<ChebyshevSmoother *> &smoothers,
                     const std::vector<const Transfer *> &transfers, const std::vector<const int *> &ess_dev,
                     const std::vector<int> &n_ess, int pre, int post, hipStream_t s)
   : pre_(pre), post_(post)
{
   // refused before anything is allocated or enqueued
   const size_t L = ops.size();
   ECM2_VERIFY(L >= 1, ERR_ARG, "multigrid: at least one level is needed");
   ECM2_VERIFY(smoothers.size() == L && ess_dev.size() == L && n_ess.size() == L && transfers.size() == L - 1, ERR_ARG,
               "multigrid: " << L << " levels need " << L << " smoothers and essential lists and " << L - 1 << " transfers");
   ECM2_VERIFY(pre >= 0 && post >= 0, ERR_ARG, "multigrid: negative smoothing count");
   for (size_t k = 0; k < L; k++)
   {
      ECM2_VERIFY(ops[k] && smoothers[k], ERR_ARG, "multigrid: null operator or smoother at level " << k);
      ECM2_VERIFY(!ops[k]->distributed(), ERR_UNSUPPORTED, "multigrid: distributed operators are not supported");
      ECM2_VERIFY(!ops[k]->concatenated(), ERR_UNSUPPORTED,
                  "multigrid: a loopback group's concatenated true vectors are not a space's L-vector (level " << k << ")");
      ECM2_VERIFY(smoothers[k]->size() == ops[k]->size(), ERR_ARG,
                  "multigrid: level " << k << "'s smoother has size " << smoothers[k]->size() << ", its operator "
                                      << ops[k]->size());
      ECM2_VERIFY(n_ess[k] >= 0 && (n_ess[k] == 0 || ess_dev[k]), ERR_ARG, "multigrid: null essential dof list at level " << k);
      if (k + 1 < L)
      {
         ECM2_VERIFY(transfers[k], ERR_ARG, "multigrid: null transfer " << k);
         ECM2_VERIFY(transfers[k]->width() == ops[k]->size() && transfers[k]->height() == ops[k + 1]->size(), ERR_ARG,
                     "multigrid: transfer " << k << " maps " << transfers[k]->width() << " -> " << transfers[k]->height()
                                            << ", levels " << k << " and " << k + 1 << " have sizes " << ops[k]->size()
                                            << " and " << ops[k + 1]->size());
      }
   }
   lv_.resize(L);
   for (size_t k = 0; k < L; k++)
   {
      Level &l = lv_[k];
      l.A = ops[k];
      l.S = smoothers[k];
      l.P = k + 1 < L ? transfers[k] : nullptr;
      l.n = ops[k]->size();
      l.n_ess = n_ess[k];
      const size_t m = std::max(l.n, 1);
      l.ess.resize(std::max(l.n_ess, 1));
      if (l.n_ess) { ECM2_HIP(hipMemcpyAsync(l.ess.data(), ess_dev[k], sizeof(int) * l.n_ess, hipMemcpyDeviceToDevice, s)); }
      l.saved.resize(std::max(l.n_ess, 1));
      // the per-level vectors, allocated once; the finest level's X and Y are the caller's
      if (k + 1 < L) { l.X.resize(m); l.Y.resize(m); }
      if (k > 0) { l.R.resize(m); l.Z.resize(m); }
   }
   ECM2_HIP(hipStreamSynchronize(s));
}

void Multigrid::set_coarse_pcg(double rel_tol, int max_iter)
{
   ECM2_VERIFY(max_iter >= 0 && rel_tol >= 0.0, ERR_ARG, "multigrid: coarse PCG rel_tol " << rel_tol << ", max_iter " << max_iter);
   coarse_rel_tol_ = rel_tol;
   coarse_max_iter_ = max_iter;
}

// R = X - A~ Y, A~ the DIAG_ONE constrained Mult (Z is free here: it holds A~ Y until the residual has read it)
void Multigrid::residual(Level &l, const double *X, double *Y, hipStream_t s)
{
   const ConstrainedMult cmult{*l.A, l.ess.data(), l.n_ess, l.saved.data(), s};
   cmult(Y, l.Z.data());
   kern::mg_residual(l.n, X, l.Z.data(), l.R.data(), s);
}

// MultigridBase::SmoothingStep (fem/multigrid.cpp:147-177): zero: Y = S X; else R = X - A~ Y, Z = S R, Y += Z
void Multigrid::smooth(Level &l, const double *X, double *Y, bool zero, hipStream_t s)
{
   if (zero) { return l.S->mult(X, Y, s); }
   residual(l, X, Y, s);
   l.S->mult(l.R.data(), l.Z.data(), s);
   kern::mg_add(l.n, l.Z.data(), Y, s);
}

// MultigridBase::Cycle (fem/multigrid.cpp:179-232), V-cycle
void Multigrid::cycle(int level, const double *X, double *Y, hipStream_t s)
{
   Level &l = lv_[level];
   if (level == 0)
   {
      if (coarse_pcg())
      {
         // (b) its own workspace and loop state, one nesting level below the caller's
         const NestedSolve nested;
         (void)pcg_solve(*l.A, l.ess.data(), l.n_ess, X, Y, coarse_rel_tol_, 0.0, coarse_max_iter_, true, s);
      }
      else { smooth(l, X, Y, true, s); }  // (a) SmoothingStep(0, true, false)
      return;
   }
   Level &c = lv_[level - 1];
   // pre-smooth: the first from the zero guess
   if (pre_ == 0 && l.n) { ECM2_HIP(hipMemsetAsync(Y, 0, sizeof(double) * l.n, s)); }
   for (int i = 0; i < pre_; i++) { smooth(l, X, Y, i == 0, s); }
   // the residual, restricted: X[k-1] = P~^T (X - A~ Y), P~ the prolongation without its essential rows and
   // columns (RectangularConstrainedOperator::MultTranspose: the fine essential entries of the input zeroed, the
   // coarse essential entries of the output zeroed); Y[k-1] = 0 is the coarse level's zero guess
   residual(l, X, Y, s);
   if (l.n_ess) { kern::set_values(l.n_ess, l.ess.data(), 0.0, l.R.data(), s); }
   c.P->mult_transpose(l.R.data(), c.X.data(), s);
   if (c.n_ess) { kern::set_values(c.n_ess, c.ess.data(), 0.0, c.X.data(), s); }
   cycle(level - 1, c.X.data(), c.Y.data(), s);
   // prolong and add: Y += P~ Y[k-1] (the coarse essential entries of the input zeroed -- in place, Y[k-1] is
   // not read again -- and the fine essential entries of the output)
   if (c.n_ess) { kern::set_values(c.n_ess, c.ess.data(), 0.0, c.Y.data(), s); }
   c.P->mult(c.Y.data(), l.Z.data(), s);
   if (l.n_ess) { kern::set_values(l.n_ess, l.ess.data(), 0.0, l.Z.data(), s); }
   kern::mg_add(l.n, l.Z.data(), Y, s);
   // post-smooth with the smoother's transpose, which is the smoother
   for (int i = 0; i < post_; i++) { smooth(l, X, Y, false, s); }
}

void Multigrid::mult(const double *x, double *y, hipStream_t s)
{
   ECM2_VERIFY(x && y, ERR_ARG, "multigrid: null vector");
   ECM2_VERIFY(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, ERR_ARG,
               "multigrid: x and y must be 16-byte aligned (got " << (const void *)x << ", " << (const void *)y << ")");
   ECM2_VERIFY(x != y, ERR_ARG, "multigrid: x and y must be distinct");
   cycle(levels() - 1, x, y, s);
}

// ---------------------------------------------------------------------------------------
// ConstrainedOperator::EliminateRHS and Operator::FormLinearSystem (identity prolongation)
// ---------------------------------------------------------------------------------------
namespace
{
// refused before anything is allocated or enqueued
void check_elimination_args(const char *what, const int *ess, int n_ess, const double *x, const double *b)
{
   ECM2_VERIFY(x && b, ERR_ARG, what << ": null vector");
   ECM2_VERIFY(n_ess >= 0 && (n_ess == 0 || ess), ERR_ARG, what << ": null essential dof list");
   ECM2_VERIFY(((uintptr_t)x % 16) == 0 && ((uintptr_t)b % 16) == 0, ERR_ARG,
               what << ": x and b must be 16-byte aligned (got " << (const void *)x << ", " << (const void *)b << ")");
   ECM2_VERIFY(x != b, ERR_ARG, what << ": x and b must be distinct");
}

// w = 0; w[ess] = x[ess]; z = A w; b -= z; b[ess] = x[ess] (operator.cpp:559-584), w and z SolverWork's p and ap.
// A rank of a distributed operator with no essential dof of its own still takes part: the Mult is collective, and the
// other ranks' lifted values reach its rows.
void eliminate(LinOp &A, const int *ess, int n_ess, const double *x, double *b, hipStream_t s)
{
   if (n_ess == 0 && !A.distributed()) { return; }
   const int n = A.size();
   SolverWork &wk = solver_work();
   wk.ensure(n, n_ess, false, false, 1);
   double *w = wk.p.data(), *z = wk.ap.data();
   if (n) { ECM2_HIP(hipMemsetAsync(w, 0, sizeof(double) * n, s)); }
   kern::copy_values(n_ess, ess, x, w, s);
   A.mult(w, z, s);
   kern::ess_sub(n, z, b, s);
   kern::copy_values(n_ess, ess, x, b, s);
   // SolverWork's invariant: no kernel reads its vectors when the next solve starts, on whichever stream
   ECM2_HIP(hipStreamSynchronize(s));
}
} // namespace

void eliminate_rhs(LinOp &A, const int *ess, int n_ess, const double *x, double *b, hipStream_t s)
{
   check_elimination_args("EliminateRHS", ess, n_ess, x, b);
   eliminate(A, ess, n_ess, x, b, s);
}

void form_linear_system(LinOp &A, const int *ess, int n_ess, double *x, double *b, bool copy_interior, hipStream_t s)
{
   check_elimination_args("FormLinearSystem", ess, n_ess, x, b);
   const int n = A.size();
   if (!copy_interior && n)
   {
      // X.SetSubVectorComplement(ess, 0.0): the essential entries parked on SolverWork's saved around a memset
      SolverWork &wk = solver_work();
      wk.ensure(n, n_ess, false, false, 1);
      kern::gather_idx(n_ess, ess, x, wk.saved.data(), s);
      ECM2_HIP(hipMemsetAsync(x, 0, sizeof(double) * n, s));
      kern::ess_scatter(n_ess, ess, wk.saved.data(), x, s);
   }
   eliminate(A, ess, n_ess, x, b, s);
}

// ---------------------------------------------------------------------------------------
// SDIRK family (slope form, ImplicitVarType::SLOPE) on an ex16-style conduction operator
// ---------------------------------------------------------------------------------------
namespace
{
const double kSdirk33A = 0.435866521508458999416019;  // ode.cpp SDIRK33Solver::Step
const double kSdirk33B = 1.20849664917601007033648;
const double kSdirk33C = 0.717933260754229499708010;
double sdirk34_a() { return 1. / std::sqrt(3.) * std::cos(M_PI / 18.) + 0.5; }
double sdirk23_gamma(int type)
{
   return type == 22 ? (2. - std::sqrt(2.)) / 2.   // gamma_opt = 2: L-stable, order 2
                     : (3. + std::sqrt(3.)) / 6.;  // default gamma_opt: A-stable, order 3
}
} // namespace

bool ode_implicit_supported(int type)
{
   return type == 21 || type == 22 || type == 23 || type == 32 || type == 33 || type == 34;
}

double ode_implicit_coeff(int type)
{
   switch (type)
   {
      case 21: return 1.0;
      case 22:
      case 33: return sdirk23_gamma(type);
      case 23: return kSdirk33A;
      case 32: return 0.5;
      case 34: return sdirk34_a();
      default: break;
   }
   ECM2_VERIFY(false, ERR_ARG, "unsupported implicit ODE solver type " << type);
   return 0.0;
}

StepStats ode_step(int type, LinOp &T, LinOp &K, double dt, double *u, const int *ess, int n_ess,
                   double rel_tol, int max_iter, bool jacobi, hipStream_t s, const double *b, int solver,
                   LinOp *jacobi_of, ChebyshevSmoother *prec)
{
   ECM2_VERIFY(ode_implicit_supported(type), ERR_ARG, "unsupported implicit ODE solver type " << type);
   ECM2_VERIFY(solver == STAGE_PCG || solver == STAGE_BICGSTAB, ERR_ARG, "unknown stage solver " << solver);
   ECM2_VERIFY(!prec || solver == STAGE_PCG, ERR_ARG, "a Chebyshev smoother goes with the PCG stage solver");
   ECM2_VERIFY(T.size() == K.size(), ERR_ARG, "T and K sizes differ");
   const int n = T.size();
   StepStats st;
   DeviceArray<double> k(std::max(n, 1)), y(std::max(n, 1)), z(std::max(n, 1)), rhs(std::max(n, 1));
   // ConductionOperator::ImplicitSolve (ex16.cpp:327-354), slope form: T k = -K u_stage [+ b]
   auto implicit_solve = [&](const double *us, double *kk) {
      K.mult(us, rhs.data(), s);
      kern::scale(n, -1.0, rhs.data(), s);
      if (b) { kern::add_scaled(n, rhs.data(), 1.0, b, rhs.data(), s); }
      if (n_ess) { kern::set_values(n_ess, ess, 0.0, rhs.data(), s); }
      const PCGResult r = solver == STAGE_BICGSTAB
                             ? bicgstab_solve(T, jacobi_of, ess, n_ess, rhs.data(), kk, rel_tol, 0.0, max_iter, s)
                          : prec ? pcg_solve_prec(T, *prec, ess, n_ess, rhs.data(), kk, rel_tol, 0.0, max_iter, s)
                                 : pcg_solve(T, ess, n_ess, rhs.data(), kk, rel_tol, 0.0, max_iter, jacobi, s);
      st.solves++;
      st.iterations += r.iterations;
      st.max_iterations = std::max(st.max_iterations, r.iterations);
      st.converged = st.converged && r.converged;
   };
   double *kk = k.data();
   switch (type)
   {
      case 21:  // BackwardEuler
         implicit_solve(u, kk);
         kern::add_scaled(n, u, dt, kk, u, s);
         break;
      case 32:  // ImplicitMidpoint
         implicit_solve(u, kk);
         kern::add_scaled(n, u, dt, kk, u, s);
         break;
      case 22:
      case 33:  // SDIRK23
      {
         const double g = sdirk23_gamma(type);
         implicit_solve(u, kk);
         kern::add_scaled(n, u, (1. - 2. * g) * dt, kk, y.data(), s);
         kern::add_scaled(n, u, dt / 2, kk, u, s);
         implicit_solve(y.data(), kk);
         kern::add_scaled(n, u, dt / 2, kk, u, s);
         break;
      }
      case 23:  // SDIRK33
      {
         const double a = kSdirk33A, b = kSdirk33B, c = kSdirk33C;
         implicit_solve(u, kk);
         kern::add_scaled(n, u, (c - a) * dt, kk, y.data(), s);
         kern::add_scaled(n, u, b * dt, kk, u, s);
         implicit_solve(y.data(), kk);
         kern::add_scaled(n, u, (1.0 - a - b) * dt, kk, u, s);
         implicit_solve(u, kk);
         kern::add_scaled(n, u, a * dt, kk, u, s);
         break;
      }
      case 34:  // SDIRK34
      {
         const double a = sdirk34_a(), b = 1. / (6. * (2. * a - 1.) * (2. * a - 1.));
         implicit_solve(u, kk);
         kern::add_scaled(n, u, (0.5 - a) * dt, kk, y.data(), s);
         kern::add_scaled(n, u, (2. * a) * dt, kk, z.data(), s);
         kern::add_scaled(n, u, b * dt, kk, u, s);
         implicit_solve(y.data(), kk);
         kern::add_scaled(n, z.data(), (1. - 4. * a) * dt, kk, z.data(), s);
         kern::add_scaled(n, u, (1. - 2. * b) * dt, kk, u, s);
         implicit_solve(z.data(), kk);
         kern::add_scaled(n, u, b * dt, kk, u, s);
         break;
      }
      default: break;
   }
   ECM2_HIP(hipStreamSynchronize(s));
   return st;
}

} // namespace ecm2
