// solvers.hpp -- the callers of the PA operator: constrained Jacobi-PCG, constrained BiCGSTAB and the SDIRK
// time steppers of an ex16-style conduction (Pennes bioheat) operator, all device
// resident, over one operator interface that the serial form, the RCCL-distributed form
// and the in-process loopback group implement.
//
// Reference:
//   Operator (the solver-facing interface)     linalg/operator.hpp:24-110
//   ConstrainedOperator DIAG_ONE               linalg/operator.cpp:586-646
//   ConstrainedOperator::EliminateRHS          linalg/operator.cpp:559-584
//   Operator::FormLinearSystem                 linalg/operator.cpp:114-129
//   IterativeSolver::iterative_mode            linalg/solvers.cpp:29-30, 875-884, 1618-1627
//   CGSolver::Mult                             linalg/solvers.cpp:869-1004
//   BiCGSTABSolver::Mult                       linalg/solvers.cpp:1579-1805
//   OperatorJacobiSmoother (PA diagonal)       linalg/solvers.hpp:421, bilinearform_ext.cpp:370-454
//   OperatorChebyshevSmoother                  linalg/solvers.hpp:498-586, solvers.cpp:455-658
//   PowerMethod::EstimateLargestEigenvalue     linalg/operator.cpp:871-928
//   Multigrid / MultigridBase (V-cycle)        fem/multigrid.cpp:106-232
//   GeometricMultigrid's constrained transfers fem/multigrid.cpp:296-309
//   parallel dot (MPI_Allreduce)               linalg/hypre / InnerProduct(comm, ...)
//   BackwardEuler / SDIRK23 / SDIRK33 / ImplicitMidpoint / SDIRK34 ::Step
//                                              linalg/ode.cpp:682-859, selection :77-91
//   ConductionOperator::ImplicitSolve          examples/ex16.cpp:327-354
#pragma once

#include "pa_form.hpp"
#include "par_form.hpp"

#include <vector>

namespace ecm2
{

// A square operator on this rank's slice of the true-dof vector.
class LinOp
{
public:
   virtual ~LinOp() = default;
   virtual int size() const = 0;
   // y = A x (Operator::Mult; y overwritten)
   virtual void mult(const double *x, double *y, hipStream_t s) = 0;
   // diagonal of the global operator on this rank's true dofs
   virtual void diagonal(double *d, hipStream_t s) = 0;
   // in-place global sum of n device scalars over all ranks (serial: nothing to do)
   virtual void sum_scalars(double *dev, int n, hipStream_t s) { (void)dev; (void)n; (void)s; }
   // true when sum_scalars communicates (a locally reduced scalar is not yet global)
   virtual bool distributed() const { return false; }
   // true when the vectors are the concatenated true vectors of a loopback group's members and not one space's
   // L-vector: what acts in a space's numbering (the multigrid's transfers and essential lists) refuses it
   virtual bool concatenated() const { return false; }
   // The Mult with its energy x^T A x folded in as energy_parts() partials (PAForm::mult_energy),
   // or 0 when this operator does not fold it
   virtual int energy_parts() const { return 0; }
   virtual void mult_energy(const double *x, double *y, double *en, hipStream_t s)
   {
      (void)x; (void)y; (void)en; (void)s;
      ECM2_VERIFY(false, ERR_UNSUPPORTED, "this operator does not fold the Mult's energy");
   }
};

class FormOp : public LinOp
{
public:
   explicit FormOp(PAForm &f) : f_(f) {}
   int size() const override { return f_.ndofs(); }
   void mult(const double *x, double *y, hipStream_t s) override { f_.mult(x, y, s); }
   void diagonal(double *d, hipStream_t s) override { f_.assemble_diagonal(d, s); }
   int energy_parts() const override { return f_.energy_parts(); }
   void mult_energy(const double *x, double *y, double *en, hipStream_t s) override { f_.mult_energy(x, y, en, s); }

private:
   PAForm &f_;
};

class ParFormOp : public LinOp
{
public:
   explicit ParFormOp(ParPAForm &f) : f_(f) {}
   int size() const override { return f_.true_size(); }
   void mult(const double *x, double *y, hipStream_t s) override { f_.mult(x, y, s); }
   void diagonal(double *d, hipStream_t s) override { f_.assemble_diagonal(d, s); }
   void sum_scalars(double *dev, int n, hipStream_t s) override { f_.allreduce_sum(dev, n, s); }
   bool distributed() const override { return true; }

private:
   ParPAForm &f_;
};

// The loopback group as one operator on the concatenated true vectors of its members
// (rank r's slice at offset(r)); dots over the concatenation are already global.
class GroupOp : public LinOp
{
public:
   explicit GroupOp(std::vector<ParPAForm *> forms);
   int size() const override { return n_; }
   bool concatenated() const override { return true; }
   void mult(const double *x, double *y, hipStream_t s) override;
   void diagonal(double *d, hipStream_t s) override;
   int offset(int r) const { return off_[r]; }

private:
   std::vector<ParPAForm *> forms_;
   std::vector<int> off_;
   int n_ = 0;
};

// One member of the loopback group as one rank's operator (measurement of a rank's solver
// iteration on its own GPU; no reference counterpart): Mult = par_group_mult_member (the P
// exchange as device copies from the peers' x, held in a private concatenated vector), the
// dots summed by a real ncclAllReduce on a one-rank communicator (the collective call without
// the xGMI hops).  Vectors are the member's true dofs.
class MemberOp : public LinOp
{
public:
   MemberOp(std::vector<ParPAForm *> forms, int member);
   int size() const override { return forms_[member_]->true_size(); }
   void mult(const double *x, double *y, hipStream_t s) override;
   void diagonal(double *d, hipStream_t s) override;
   void sum_scalars(double *dev, int n, hipStream_t s) override { group_self_allreduce(dev, n, s); }
   bool distributed() const override { return true; }

private:
   std::vector<ParPAForm *> forms_;
   int member_;
   std::vector<int> off_;
   DeviceArray<double> peers_, yscratch_;  // the peers' x (zeros) and y (never read), concatenated
};

struct PCGResult
{
   int iterations = 0;
   double final_norm = 0.0, initial_norm = 0.0;
   bool converged = false;
};

// Constrained (DIAG_ONE on ess) Jacobi-PCG, x overwritten (iterative_mode = false).
// Scalars stay on the device and so do the stopping tests: the loop is driven by the device (kernels.hpp
// LoopCtl), the host polls a mapped mirror's progress mark and synchronises the stream for the two read-backs
// before the loop and once after it.
// iterative_mode (IterativeSolver's default in the reference, solvers.cpp:29-30; here off unless asked for): x is the
// start, r = b - A~ x (CGSolver::Mult, solvers.cpp:875-884) by the constrained Mult on the caller's x and one
// 16-byte pass; everything after that is the same loop.  b must then be 16-byte aligned too (ERR_ARG).  With
// b[ess] = x[ess] (form_linear_system) r[ess] = 0 exactly and x[ess] keeps its bits.  The preconditioners stay
// iterative_mode = false (solvers.cpp:181).  false: the launches of before, not one more.
PCGResult pcg_solve(LinOp &A, const int *ess_dev, int n_ess, const double *b, double *x,
                    double rel_tol, double abs_tol, int max_iter, bool jacobi, hipStream_t s,
                    bool iterative_mode = false);
PCGResult pcg_solve(PAForm &A, const int *ess_dev, int n_ess, const double *b, double *x,
                    double rel_tol, double abs_tol, int max_iter, bool jacobi, hipStream_t s);

// Constrained (DIAG_ONE on ess) BiCGSTAB for a nonsymmetric A (a form with a ConvectionIntegrator), x
// overwritten (iterative_mode = false): BiCGSTABSolver::Mult (linalg/solvers.cpp:1579-1805) restated
// around the same constrained Mult as the PCG, the iteration's vector work in the fused passes of
// k_bicgstab.hip, the loop driven by the device.  final_norm = ||r|| or ||s|| (norms, as the reference's
// tol_goal = max(||r_0|| rel_tol, abs_tol)); iterations = final_iter.  Not converged: rho_1 == 0, omega == 0,
// max_iter.  A non-finite ||r_0||, ||s|| or ||r|| (alpha = rho_1 / 0 among them), where MFEM_VERIFY aborts:
// ERR_NUMERIC.
// jacobi_of (or null: no preconditioner): OperatorJacobiSmoother built from a second operator of A's size --
// dinv = 1 / diag(jacobi_of), essential rows 1 -- as a caller builds it from the symmetric part, since the
// diagonal of a form with an active convection integrator is refused.
// A distributed operator (distributed() == true): ERR_UNSUPPORTED.  x must be 16-byte aligned (ERR_ARG).
// iterative_mode: r = b - A~ x, r~ = r (solvers.cpp:1618-1622), as pcg_solve's; nothing else changes.
PCGResult bicgstab_solve(LinOp &A, LinOp *jacobi_of, const int *ess_dev, int n_ess, const double *b, double *x,
                         double rel_tol, double abs_tol, int max_iter, hipStream_t s, bool iterative_mode = false);

// PowerMethod::EstimateLargestEigenvalue (linalg/operator.cpp:871-928) on D^-1 A~, A~ the DIAG_ONE constrained A
// and dinv a device vector (1 / diag, essential rows 1): each step normalises v0 (v0 *= 1 / sqrt((v0, v0))),
// applies v1 = dinv .* (A~ v0), takes eig_new = (v0, v1), forms diff = |(eig_new - eig) / eig| with eig starting
// at 1, swaps and breaks on diff < tol -- one host read-back per step ((v1, v1), the next step's norm, is summed
// by the pass that sums (v0, v1)).  v0 (device, A.size(), 16-byte aligned: ERR_ARG otherwise): the start vector
// on entry, the last iterate (not normalised) on return; null: the library's own, filled from an integer hash
// of the index in (0, 1) (kern::cheb_fill_hash) -- the reference's Vector::Randomize(seed) draws from glibc's
// rand(), which is not reproduced.  A non-finite eigenvalue: ERR_NUMERIC.  Distributed operators: ERR_UNSUPPORTED.
struct PowerResult
{
   double eig = 1.0;
   int steps = 0;
};
PowerResult power_method(LinOp &A, const double *dinv, const int *ess_dev, int n_ess, double *v0, int num_steps,
                         double tol, hipStream_t s);
// ... with dinv taken from diag_of's diagonal (null: A's), essential rows 1, as the smoother takes it
PowerResult power_method(LinOp &A, LinOp *diag_of, const int *ess_dev, int n_ess, double *v0, int num_steps,
                         double tol, hipStream_t s);

// OperatorChebyshevSmoother (linalg/solvers.hpp:498-586, solvers.cpp:455-658) on the DIAG_ONE constrained
// operator A~: y = sum_{k < order} c_k (D^-1 A~)^k D^-1 x, the coefficients from cheb_coeffs.hpp (Setup,
// :538-617), Mult's operations per entry in the reference's order (:619-658), iterative_mode = false.
// diag_of (null: A itself): the operator whose diagonal D is taken, of A's size (as bicgstab_solve's jacobi_of).
// The diagonal is taken at construction (dinv = 1 / diag, essential rows 1) and so is the essential list (a
// copy): a form that is assembled again with other coefficients needs a new smoother.  The operator(s) must
// outlive the smoother.  order outside 1..5: ERR_ARG (the reference aborts).  Distributed operators
// (distributed() == true): ERR_UNSUPPORTED.  Two applications are bitwise equal.
class ChebyshevSmoother
{
public:
   // a given estimate of the largest eigenvalue of D^-1 A~
   ChebyshevSmoother(LinOp &A, LinOp *diag_of, const int *ess_dev, int n_ess, int order, double max_eig_estimate,
                     hipStream_t s);
   // the estimate from power_method (the reference's defaults: 10 iterations, tolerance 1e-8); v0 as there
   ChebyshevSmoother(LinOp &A, LinOp *diag_of, const int *ess_dev, int n_ess, int order, int power_iterations,
                     double power_tolerance, double *v0, hipStream_t s);
   int size() const { return n_; }
   int order() const { return order_; }
   double max_eig() const { return max_eig_; }
   int power_steps() const { return power_steps_; }  // (0: the estimate was given)
   const double *coeffs() const { return coeffs_; }
   // y = S x (x, y device vectors of size(), 16-byte aligned and distinct: ERR_ARG otherwise)
   void mult(const double *x, double *y, hipStream_t s);
   // what the PCG's fused passes take (solvers.cpp ChebPrec)
   LinOp &op() { return A_; }
   const double *dinv() const { return dinv_.data(); }
   const int *ess() const { return ess_.data(); }
   int n_ess() const { return n_ess_; }

private:
   void setup(LinOp *diag_of, const int *ess_dev, hipStream_t s);
   LinOp &A_;
   int n_, n_ess_, order_;
   double max_eig_ = 0.0, coeffs_[5] = {};
   int power_steps_ = 0;
   DeviceArray<int> ess_;
   DeviceArray<double> dinv_, t_, h_, saved_;  // 1 / diag; the term (D^-1 A~)^k D^-1 x, A~ of it, its ess entries
};

// CGSolver::Mult (linalg/solvers.cpp:869-1004) with prec = B on the constrained A, x overwritten.  The loop is the
// one of pcg_solve (solvers.cpp pcg_loop: the same device-driven stops -- (B r, r) < 0 before or inside the loop,
// (A d, d) == 0, non-finite -> ERR_NUMERIC, converged, max_iter -- the same folded (A d, d) where A offers it, the
// same deferred x += alpha d); this function supplies the preconditioner: z = B r stored, the smoother's first term
// in the pass that updates r, its last in the pass that sums (r, z).  Refused, in this order and before anything is
// allocated or enqueued: distributed operators (ERR_UNSUPPORTED), B not of A's size (ERR_ARG), x not 16-byte
// aligned (ERR_ARG, the loop's own check).
PCGResult pcg_solve_prec(LinOp &A, ChebyshevSmoother &B, const int *ess_dev, int n_ess, const double *b, double *x,
                         double rel_tol, double abs_tol, int max_iter, hipStream_t s, bool iterative_mode = false);

// Multigrid / MultigridBase (fem/multigrid.cpp:106-232: Mult, SmoothingStep, Cycle), V-cycle only, over levels 0
// (coarsest) .. L - 1 that the caller supplies: each level's operator, its ChebyshevSmoother (built by the caller
// on that level's operator and essential list), its essential list (device, copied) and the transfer k -> k + 1
// (a Transfer, transfer.hpp: one class for both kinds, between two orders on one mesh or between a mesh and its
// refinement, mixed freely).  The essential rows and columns of the prolongations are removed as GeometricMultigrid does (fem/multigrid.cpp:296-309,
// RectangularConstrainedOperator): the coarse essential entries of the input and the fine essential entries of
// the output are zero, and likewise for the transpose.
// mult(x, y): one cycle from a zero guess (iterative_mode is not used), the reference's operations per entry:
//   the first pre-smoothing Y = S X; every other smoothing R = X - A~ Y, Y += S R (A~ the DIAG_ONE constrained
//   Mult; the post-smoothing's S^T is S: OperatorChebyshevSmoother::MultTranspose calls Mult); the residual
//   restricted into X[k-1]; the coarse correction prolonged and added.
// The coarsest level: (a) its smoother applied once (Multigrid's smoother at level 0), or (b) after
// set_coarse_pcg(rel_tol, max_iter > 0) a constrained Jacobi-PCG from a zero guess (ex26: sqrt(1e-4), 200), which
// synchronises the stream; with (b) the cycle is not a symmetric operator.
// Sizes that do not chain (transfer k's width / height against levels k / k + 1, a smoother's size against its
// level): ERR_ARG; no level: ERR_ARG; distributed operators, and a loopback group (whose concatenated true vectors
// are not in the numbering of the transfers and essential lists): ERR_UNSUPPORTED.  x, y: device vectors of the finest
// size, 16-byte aligned and distinct (ERR_ARG).  Operators, smoothers and transfers must outlive it.  Two cycles
// are bitwise equal.
class Transfer;
class Multigrid
{
public:
   Multigrid(const std::vector<LinOp *> &ops, const std::vector<ChebyshevSmoother *> &smoothers,
             const std::vector<const Transfer *> &transfers, const std::vector<const int *> &ess_dev,
             const std::vector<int> &n_ess, int pre, int post, hipStream_t s);
   int levels() const { return (int)lv_.size(); }
   int size() const { return lv_.back().n; }
   void set_coarse_pcg(double rel_tol, int max_iter);
   // the coarse solve synchronises the stream and may throw ERR_NUMERIC (what the PCG's loop orders its events by)
   bool coarse_pcg() const { return coarse_max_iter_ > 0; }
   void mult(const double *x, double *y, hipStream_t s);

private:
   struct Level
   {
      LinOp *A = nullptr;
      ChebyshevSmoother *S = nullptr;
      const Transfer *P = nullptr;   // this level -> the next finer one (null on the finest)
      int n = 0, n_ess = 0;
      DeviceArray<int> ess;
      DeviceArray<double> X, Y, R, Z, saved;
   };
   void residual(Level &l, const double *X, double *Y, hipStream_t s);  // l.R = X - A~ Y
   void smooth(Level &l, const double *X, double *Y, bool zero, hipStream_t s);
   void cycle(int level, const double *X, double *Y, hipStream_t s);
   std::vector<Level> lv_;
   int pre_, post_;
   double coarse_rel_tol_ = 0.0;
   int coarse_max_iter_ = 0;
};

// CGSolver::Mult (linalg/solvers.cpp:869-1004) with prec = the cycle on the constrained A, x overwritten: the same
// loop again (pcg_loop: the same stops, folded (A d, d), deferred x += alpha d, results and read-backs); this function
// supplies the preconditioner: z = B r computed by one cycle between the pass that updates r and the pass that sums
// (r, z), and, with a coarse PCG, the loop's synchronise-and-look before each cycle.  Refused, in this order and
// before anything is allocated or enqueued: distributed operators and a loopback group as A (ERR_UNSUPPORTED), B not
// of A's size (ERR_ARG), x not 16-byte aligned (ERR_ARG, the loop's own check).
PCGResult pcg_solve_mg(LinOp &A, Multigrid &B, const int *ess_dev, int n_ess, const double *b, double *x, double rel_tol,
                       double abs_tol, int max_iter, hipStream_t s, bool iterative_mode = false);

// ConstrainedOperator::EliminateRHS (linalg/operator.cpp:559-584) per entry: w = 0; w[ess] = x[ess]; z = A w; b -= z;
// b[ess] = x[ess].  Any LinOp: the serial form, a loopback group in its concatenated numbering, an RCCL rank or a
// member (the Mult is collective; no dot is needed).  w and z are the solvers' workspace (its p and ap: nothing is
// allocated after the first call of a size) and the call ends with the stream synchronised, as every solve does.
// n_ess == 0 on an operator that does not communicate: b keeps its bits and no kernel is launched.  x, b: device
// vectors of A.size(), 16-byte aligned and distinct (ERR_ARG otherwise, before anything is enqueued).
void eliminate_rhs(LinOp &A, const int *ess_dev, int n_ess, const double *x, double *b, hipStream_t s);
// Operator::FormLinearSystem (linalg/operator.cpp:114-129) for the identity prolongation (X = x, B = b in place):
// unless copy_interior, X.SetSubVectorComplement(ess, 0.0) (the essential entries gathered, x cleared, scattered
// back); then eliminate_rhs.  RecoverFEMSolution is the identity.
void form_linear_system(LinOp &A, const int *ess_dev, int n_ess, double *x, double *b, bool copy_interior,
                        hipStream_t s);

// ODESolver::SelectImplicit numbering (ode.cpp:77-91): 21 BackwardEuler, 22 SDIRK23(L-stable),
// 23 SDIRK33, 32 ImplicitMidpoint, 33 SDIRK23 (A-stable, order 3), 34 SDIRK34.
bool ode_implicit_supported(int type);
// The implicit coefficient c of every stage solve (M + c*dt*K) k = -K u of `type`.
double ode_implicit_coeff(int type);

struct StepStats
{
   int solves = 0, iterations = 0, max_iterations = 0;
   bool converged = true;
};

// One implicit step u <- u(t + dt) of M du/dt = -K u (ex16 ConductionOperator, slope
// form): each stage solves T k = -K u_stage with T = M + c*dt*K supplied assembled by
// the caller (c = ode_implicit_coeff(type)); ess dofs keep their values (k = 0 there).
// b (optional, device, true dofs in the operator's numbering): a source frozen over the step,
// M du/dt = -K u + b -- every stage solves T k = -K u_stage + b (essential rows zeroed as before);
// null: exactly the homogeneous step.
// solver: the stage solver.  STAGE_PCG (the default: the launches above, `jacobi` its preconditioner switch);
// STAGE_BICGSTAB: bicgstab_solve with jacobi_of -- the caller assembles T = M + c*dt*(K_sym + C) and
// K = K_sym + C with the convection inside both, and passes jacobi_of = M + c*dt*K_sym (null: none;
// `jacobi` is not read).
// prec (STAGE_PCG only, ERR_ARG otherwise): the stage solves run pcg_solve_prec with it and `jacobi` is not
// read; T is fixed over a step, so one smoother built from T serves every stage.
enum StageSolver : int { STAGE_PCG = 0, STAGE_BICGSTAB = 1 };
StepStats ode_step(int type, LinOp &T, LinOp &K, double dt, double *u, const int *ess_dev, int n_ess,
                   double rel_tol, int max_iter, bool jacobi, hipStream_t s, const double *b = nullptr,
                   int solver = STAGE_PCG, LinOp *jacobi_of = nullptr, ChebyshevSmoother *prec = nullptr);

} // namespace ecm2
