// k_bdr.hip -- the boundary-face kernels of a Robin condition (gfx950, FP64): what the reference
// runs for  a.AddBoundaryIntegrator(new MassIntegrator(h), marker)  and
// b.AddBoundaryIntegrator(new BoundaryLFIntegrator(h T_b), marker)  on the device path.
//
// Reference mirrored:
//   MassIntegrator::AssemblePABoundary     fem/integ/bilininteg_mass_pa.cpp:81-125
//                                          (pa_data(q, f) = W_q c detJ_face(q, f), dim = 2)
//   2D mass apply B^T D B and diagonal     bilininteg_mass_pa.cpp:127-169 (ApplyPAKernels /
//                                          DiagonalPAKernels, dim = 2)
//   FaceGeometricFactors DETERMINANTS      mesh/mesh.cpp:15275-15334 (|dx/dxi x dx/deta|)
//   BoundaryLFIntegrator::AssembleDevice   fem/integ/lininteg_boundary.cpp:74-153, 214-228
//                                          (BLFEvalAssemble3D: Y(dx, dy, e) += sum B B (W c detJ))
//   the boundary FaceRestriction's add     fem/bilinearform_ext.cpp:625-675 (AddMultTransposeInPlace)
//
// The faces are a compacted list (the marked part of the boundary).  Four kernels:
//   k_bdr_setup      thread per (face, point): qd = W c detJ w_f, detJ from the quad's four corners
//                    (a bilinear face) or a caller's array
//   k_bdr_apply_tpf  p <= 2: thread per face, the whole 2D sum factorisation in registers, the basis
//                    in the kernel-argument segment (constant indices, scalar loads)
//   k_bdr_apply_grp  p >= 3: 8 lanes per face, 8 faces per 64-lane workgroup; a lane owns one line of
//                    the face (a xi index, then a point column, then a xi index again), the other
//                    direction goes through the face's LDS slice; the basis sits in LDS
//   k_bdr_tapply     thread per (face, dof): B^T B^T qd (the face linear form) or with squared
//                    tables (the face mass diagonal)
//   k_bdr_add        thread per boundary dof: y[d] += its CSR row of face-vector entries in ascending
//                    face order.  No atomics: two runs are bitwise equal.
#include "dev_common.hpp"

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kBdrThreads = 64;
constexpr int kGrpLanes = 8;                          // lanes per face (>= max(D, Q))
constexpr int kGrpFaces = kBdrThreads / kGrpLanes;    // faces per workgroup

__global__ void __launch_bounds__(256) k_bdr_setup(const kern::BdrSetupArgs a)
{
   const int nq = a.q1d * a.q1d;
   const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= (long)a.n * nq) { return; }
   const int f = (int)(t / nq), q = (int)(t % nq);
   const int be = a.faces[f];
   double dj;
   if (a.detj) { dj = a.detj[(size_t)be * nq + q]; }
   else
   {
      const double xi = a.qpts[q % a.q1d], et = a.qpts[q / a.q1d];
      const double *X = a.nodes + (size_t)be * 12;  // [c][a], a = 0..3 <-> v0, v1, v3, v2
      double tx[3], ty[3];
#pragma unroll
      for (int c = 0; c < 3; c++)
      {
         const double x0 = X[c * 4], x1 = X[c * 4 + 1], x2 = X[c * 4 + 2], x3 = X[c * 4 + 3];
         tx[c] = (1.0 - et) * (x1 - x0) + et * (x3 - x2);
         ty[c] = (1.0 - xi) * (x2 - x0) + xi * (x3 - x1);
      }
      const double nx = tx[1] * ty[2] - tx[2] * ty[1], ny = tx[2] * ty[0] - tx[0] * ty[2],
                   nz = tx[0] * ty[1] - tx[1] * ty[0];
      dj = sqrt(nx * nx + ny * ny + nz * nz);
   }
   const double c = a.quad ? a.quad[(size_t)be * nq + q] : a.value;
   const double v = a.wq[q] * c * dj * a.wf[f];
   double *o = a.qd + (size_t)f * nq + q;
   *o = a.accumulate ? *o + v : v;
}

// p <= 2: one thread per face.  u (D x D) -> B u along xi -> along eta -> times qd -> B^T along eta
// -> B^T along xi; every index a constant after unrolling.
template <int D, int Q>
__global__ void __launch_bounds__(kBdrThreads) k_bdr_apply_tpf(int n, const int *__restrict__ faces,
                                                              const int *__restrict__ bmap, const double *__restrict__ qd,
                                                              const double *__restrict__ x, double *__restrict__ yf,
                                                              const Basis1D b)
{
   const int f = blockIdx.x * kBdrThreads + threadIdx.x;
   if (f >= n) { return; }
   const int *m = bmap + (size_t)faces[f] * (D * D);
   double u[D * D];
#pragma unroll
   for (int i = 0; i < D * D; i++) { u[i] = x[m[i]]; }
   double t[D][Q];  // [i2][q1]
#pragma unroll
   for (int i2 = 0; i2 < D; i2++)
#pragma unroll
      for (int q1 = 0; q1 < Q; q1++)
      {
         double s = 0.0;
#pragma unroll
         for (int i1 = 0; i1 < D; i1++) { s += b.B[q1 + MQ * i1] * u[i1 + D * i2]; }
         t[i2][q1] = s;
      }
   const double *qf = qd + (size_t)f * (Q * Q);
   double v[Q][Q];  // [q2][q1]
#pragma unroll
   for (int q2 = 0; q2 < Q; q2++)
#pragma unroll
      for (int q1 = 0; q1 < Q; q1++)
      {
         double s = 0.0;
#pragma unroll
         for (int i2 = 0; i2 < D; i2++) { s += b.B[q2 + MQ * i2] * t[i2][q1]; }
         v[q2][q1] = s * qf[q1 + Q * q2];
      }
#pragma unroll
   for (int i2 = 0; i2 < D; i2++)
   {
      double w[Q];  // [q1]
#pragma unroll
      for (int q1 = 0; q1 < Q; q1++)
      {
         double s = 0.0;
#pragma unroll
         for (int q2 = 0; q2 < Q; q2++) { s += b.B[q2 + MQ * i2] * v[q2][q1]; }
         w[q1] = s;
      }
#pragma unroll
      for (int i1 = 0; i1 < D; i1++)
      {
         double s = 0.0;
#pragma unroll
         for (int q1 = 0; q1 < Q; q1++) { s += b.B[q1 + MQ * i1] * w[q1]; }
         yf[(size_t)f * (D * D) + i1 + D * i2] = s;
      }
   }
}

// p >= 3: kGrpLanes lanes per face.  Stage 1: lane i1 < D gathers its eta line and contracts it
// (t[i1][q2]); stage 2: lane q1 < Q contracts xi from LDS, scales by qd and contracts eta back
// (s[q1][i2]); stage 3: lane i1 < D contracts xi back and stores.  The barriers are uniform: lanes of
// a face past n, or past D / Q, skip the loads and stores only.
template <int D, int Q>
__global__ void __launch_bounds__(kBdrThreads) k_bdr_apply_grp(int n, const int *__restrict__ faces,
                                                              const int *__restrict__ bmap, const double *__restrict__ qd,
                                                              const double *__restrict__ x, double *__restrict__ yf,
                                                              const double *__restrict__ Bdev)
{
   static_assert(D <= kGrpLanes && Q <= kGrpLanes, "a face line per lane");
   __shared__ double sB[Q * D];                  // B[q + Q d]
   __shared__ double sT[kGrpFaces][D * Q + 1];   // [i1][q2]
   __shared__ double sS[kGrpFaces][Q * D + 1];   // [q1][i2]
   const int tid = threadIdx.x, fs = tid / kGrpLanes, l = tid % kGrpLanes;
   const int f = blockIdx.x * kGrpFaces + fs;
   const bool valid = f < n;
   for (int i = tid; i < Q * D; i += kBdrThreads) { sB[i] = Bdev[i]; }
   __syncthreads();
   if (valid && l < D)
   {
      const int *m = bmap + (size_t)faces[f] * (D * D);
      double u[D];
#pragma unroll
      for (int i2 = 0; i2 < D; i2++) { u[i2] = x[m[l + D * i2]]; }
#pragma unroll
      for (int q2 = 0; q2 < Q; q2++)
      {
         double s = 0.0;
#pragma unroll
         for (int i2 = 0; i2 < D; i2++) { s += sB[q2 + Q * i2] * u[i2]; }
         sT[fs][l * Q + q2] = s;
      }
   }
   __syncthreads();
   if (valid && l < Q)
   {
      const double *qf = qd + (size_t)f * (Q * Q);
      double v[Q];
#pragma unroll
      for (int q2 = 0; q2 < Q; q2++)
      {
         double s = 0.0;
#pragma unroll
         for (int i1 = 0; i1 < D; i1++) { s += sB[l + Q * i1] * sT[fs][i1 * Q + q2]; }
         v[q2] = s * qf[l + Q * q2];
      }
#pragma unroll
      for (int i2 = 0; i2 < D; i2++)
      {
         double s = 0.0;
#pragma unroll
         for (int q2 = 0; q2 < Q; q2++) { s += sB[q2 + Q * i2] * v[q2]; }
         sS[fs][l * D + i2] = s;
      }
   }
   __syncthreads();
   if (valid && l < D)
   {
#pragma unroll
      for (int i2 = 0; i2 < D; i2++)
      {
         double s = 0.0;
#pragma unroll
         for (int q1 = 0; q1 < Q; q1++) { s += sB[q1 + Q * l] * sS[fs][q1 * D + i2]; }
         yf[(size_t)f * (D * D) + l + D * i2] = s;
      }
   }
}

// yf[f][i1 + D i2] = sum_q2 T[q2][i2] sum_q1 T[q1][i1] qd[f][q1 + Q q2], T = B or B^2 entrywise
__global__ void __launch_bounds__(256) k_bdr_tapply(int D, int Q, int n, const double *__restrict__ qd, int squared,
                                                    double *__restrict__ yf, const double *__restrict__ Bdev)
{
   __shared__ double sB[MAX_Q1D * MAX_D1D];
   for (int i = threadIdx.x; i < Q * D; i += blockDim.x)
   {
      const double v = Bdev[i];
      sB[i] = squared ? v * v : v;
   }
   __syncthreads();
   const int dd = D * D;
   const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= (long)n * dd) { return; }
   const int f = (int)(t / dd), i = (int)(t % dd), i1 = i % D, i2 = i / D;
   const double *qf = qd + (size_t)f * (Q * Q);
   double s = 0.0;
   for (int q2 = 0; q2 < Q; q2++)
   {
      double r = 0.0;
      for (int q1 = 0; q1 < Q; q1++) { r += sB[q1 + Q * i1] * qf[q1 + Q * q2]; }
      s += sB[q2 + Q * i2] * r;
   }
   yf[t] = s;
}

__global__ void __launch_bounds__(256) k_bdr_add(int nrows, const int *__restrict__ dof, const int *__restrict__ off,
                                                 const int *__restrict__ idx, const double *__restrict__ yf,
                                                 double *__restrict__ y)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= nrows) { return; }
   double s = y[dof[r]];
   for (int k = off[r]; k < off[r + 1]; k++) { s += yf[idx[k]]; }
   y[dof[r]] = s;
}

} // namespace

namespace kern
{

void bdr_setup_qdata(const BdrSetupArgs &a, hipStream_t s)
{
   if (a.n == 0) { return; }
   ECM2_VERIFY(a.q1d >= 1 && a.q1d <= MAX_Q1D, ERR_ARG, "boundary rule of " << a.q1d << " points");
   ECM2_VERIFY((a.nodes != nullptr) != (a.detj != nullptr), ERR_STATE, "boundary faces need corners or a detJ array");
   ECM2_VERIFY(a.faces && a.wq && a.wf && a.qd && (a.detj || a.qpts), ERR_INTERNAL, "boundary setup arguments");
   const long nt = (long)a.n * a.q1d * a.q1d;
   hipLaunchKernelGGL(k_bdr_setup, dim3(grid_for(nt, 256)), dim3(256), 0, s, a);
   ECM2_HIP(hipGetLastError());
}

bool has_bdr_apply(int D, int Q) { return D >= 2 && D <= 5 && (Q == D || Q == D + 1); }

void bdr_mass_apply(int D, int Q, int n, const int *faces, const int *bmap, const double *qd, const double *x,
                    double *yf, const Basis1D &b, const double *Bdev, hipStream_t s)
{
   ECM2_VERIFY(has_bdr_apply(D, Q), ERR_UNSUPPORTED, "no face mass kernel for D1D=" << D << " Q1D=" << Q);
   if (n == 0) { return; }
#define ECM2_BDR_TPF(d, q)                                                                                             \
   if (D == d && Q == q)                                                                                               \
   {                                                                                                                   \
      hipLaunchKernelGGL((k_bdr_apply_tpf<d, q>), dim3(grid_for(n, kBdrThreads)), dim3(kBdrThreads), 0, s, n, faces,  \
                         bmap, qd, x, yf, b);                                                                          \
   }
#define ECM2_BDR_GRP(d, q)                                                                                             \
   if (D == d && Q == q)                                                                                               \
   {                                                                                                                   \
      hipLaunchKernelGGL((k_bdr_apply_grp<d, q>), dim3(grid_for(n, kGrpFaces)), dim3(kBdrThreads), 0, s, n, faces,    \
                         bmap, qd, x, yf, Bdev);                                                                       \
   }
   ECM2_BDR_TPF(2, 2) ECM2_BDR_TPF(2, 3) ECM2_BDR_TPF(3, 3) ECM2_BDR_TPF(3, 4)
   ECM2_BDR_GRP(4, 4) ECM2_BDR_GRP(4, 5) ECM2_BDR_GRP(5, 5) ECM2_BDR_GRP(5, 6)
#undef ECM2_BDR_TPF
#undef ECM2_BDR_GRP
   ECM2_HIP(hipGetLastError());
}

void bdr_transpose_apply(int D, int Q, int n, const double *qd, bool squared, double *yf, const double *Bdev,
                         hipStream_t s)
{
   ECM2_VERIFY(D >= 1 && D <= MAX_D1D && Q >= 1 && Q <= MAX_Q1D, ERR_ARG, "face table size");
   if (n == 0) { return; }
   hipLaunchKernelGGL(k_bdr_tapply, dim3(grid_for((long)n * D * D, 256)), dim3(256), 0, s, D, Q, n, qd,
                      squared ? 1 : 0, yf, Bdev);
   ECM2_HIP(hipGetLastError());
}

void bdr_add(int nrows, const int *dof, const int *off, const int *idx, const double *yf, double *y, hipStream_t s)
{
   if (nrows == 0) { return; }
   hipLaunchKernelGGL(k_bdr_add, dim3(grid_for(nrows, 256)), dim3(256), 0, s, nrows, dof, off, idx, yf, y);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
