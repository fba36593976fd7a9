// k_conv.hip -- the convection kernels (gfx950, FP64): what the reference runs for
// a.AddDomainIntegrator(new ConvectionIntegrator(vel, alpha), marker) at AssemblyLevel::PARTIAL -- the
// blood-flow advection term rho_b c_b u . grad T of the bioheat operator.
//
// Reference mirrored:
//   PAConvectionSetup3D      fem/integ/bilininteg_convection_pa.cpp:100-152
//                            (pa_data(q, c, e) = alpha W_q (adj J(q) v(q))_c, layout [e][3][nq])
//   PAConvectionApply3D      fem/integ/bilininteg_convection_kernels.hpp:274-451
//                            (y_e += B^T [(pa . grad_ref)(x_e)])
//   PAConvectionApplyT3D     bilininteg_convection_kernels.hpp:897-
//                            (y_e += sum_c G_c^T [pa_c (B x_e)])
//   ElementRestriction::MultTranspose  fem/restriction.cpp:146-186 (the add pass's CSR sum)
//
// The elements are a compacted list (the marked part of the mesh: the blood pool).  Four kernels:
//   k_conv_setup        thread per (active element, point): adj(J) from the element's corners (the
//                       trilinear map, as k_lform) or from the caller's Jacobians
//   k_conv_apply_tpe    p <= 2: thread per element, 64 per wave, everything in registers, the basis in
//                       the kernel-argument segment (constant indices, scalar loads); plane by plane:
//                       one z contraction per plane, y per row, x per point, and back.  qdata
//                       [blk][q][3][lane] and map / E-vector [blk][nd][lane]: every wave-wide access
//                       is contiguous; the qdata loads are nontemporal (read once per apply)
//   k_conv_apply_sheet  p = 3, 4: k_lform's mapping -- a Q x Q thread sheet per element, 256 / Q^2
//                       sheets per workgroup, z columns in registers, the x / y stages through the
//                       sheet's LDS slice (odd length); qdata in the reference layout
//   k_conv_add          thread per touched dof: y[d] += its CSR row of E-vector entries in ascending
//                       element order.  No atomics: two runs are bitwise equal.
// Lanes / sheets past the active count compute on in-bounds data (padded map rows, zero qdata) or
// skip the LDS stages, and store nothing; the workgroup's barriers are uniform.
#include "dev_common.hpp"

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kCvWave = 64;       // elements per workgroup of the thread-per-element kernel
constexpr int kCvThreads = 256;   // threads per workgroup of the sheet kernel

__global__ void __launch_bounds__(256) k_conv_setup(const kern::ConvSetupArgs a)
{
   const int Q = a.q1d, nq = Q * Q * Q;
   const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
   int k, q, blk = 0, lane = 0;
   if (a.blocked)
   {
      // (blk, q, lane), the lane fastest: a wave writes 64 consecutive doubles per component
      const long nb = ((long)a.n + kCvWave - 1) / kCvWave;
      if (t >= nb * nq * kCvWave) { return; }
      lane = (int)(t % kCvWave);
      q = (int)((t / kCvWave) % nq);
      blk = (int)(t / ((long)kCvWave * nq));
      k = blk * kCvWave + lane;
   }
   else
   {
      if (t >= (long)a.n * nq) { return; }
      k = (int)(t / nq);
      q = (int)(t % nq);
   }
   double y[3] = {0.0, 0.0, 0.0};  // (the padding lanes of the last block store zeros)
   if (k < a.n)
   {
      const size_t e = (size_t)a.act[k];
      double J[3][3];
      if (a.J)
      {
#pragma unroll
         for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) { J[i][j] = a.J[q + (size_t)nq * (i + 3 * (j + 3 * e))]; }
      }
      else
      {
         // x_i = c0 + c1 xi + c2 eta + c3 zeta + c4 xi eta + c5 xi zeta + c6 eta zeta + c7 xi eta zeta
         // from the corners a = ax + 2 ay + 4 az (kernels.hpp TRILINEAR): c[3 (k - 1) + i]
         double c[21];
#pragma unroll
         for (int i = 0; i < 3; i++)
         {
            const double *X = a.enodes + (e * 3 + i) * 8;
            c[i] = X[1] - X[0];
            c[3 + i] = X[2] - X[0];
            c[6 + i] = X[4] - X[0];
            c[9 + i] = (X[3] - X[2]) - (X[1] - X[0]);
            c[12 + i] = (X[5] - X[4]) - (X[1] - X[0]);
            c[15 + i] = (X[6] - X[4]) - (X[2] - X[0]);
            c[18 + i] = ((X[7] - X[6]) - (X[5] - X[4])) - ((X[3] - X[2]) - (X[1] - X[0]));
         }
         trilinear_jacobian(c, a.qp.x[q % Q], a.qp.x[(q / Q) % Q], a.qp.x[q / (Q * Q)], J);
      }
      double A[3][3];
      adj3(J, A);
      const double w = a.alpha * a.W[q];
      const double *v = a.vq ? a.vq + (e * nq + q) * 3 : nullptr;
      const double wx = w * (v ? v[0] : a.v[0]), wy = w * (v ? v[1] : a.v[1]), wz = w * (v ? v[2] : a.v[2]);
#pragma unroll
      for (int c = 0; c < 3; c++) { y[c] = wx * A[c][0] + wy * A[c][1] + wz * A[c][2]; }
   }
#pragma unroll
   for (int c = 0; c < 3; c++)
   {
      if (a.blocked) { a.qd[(((size_t)blk * nq + q) * 3 + c) * kCvWave + lane] = y[c]; }
      else { a.qd[((size_t)k * 3 + c) * nq + q] = y[c]; }
   }
}

// p <= 2: one thread per element.  TRANSPOSE = false: u -> (d/dxi, d/deta, d/dzeta) u at the points
// -> pa . grad -> B^T back; true: u -> B u at the points -> pa_c times it -> G_c^T back.  Every index
// is a constant after unrolling.
template <int D, int Q, bool TRANSPOSE>
__global__ void __launch_bounds__(kCvWave) k_conv_apply_tpe(int n, const int *__restrict__ map,
                                                           const double *__restrict__ qd, const double *__restrict__ x,
                                                           double *__restrict__ ye, const Basis1D b)
{
   constexpr int ND = D * D * D, NQ = Q * Q * Q;
   const int lane = threadIdx.x, blk = blockIdx.x;
   const int *m = map + (size_t)blk * ND * kCvWave + lane;
   const double *qp = qd + (size_t)blk * NQ * 3 * kCvWave + lane;
   double u[ND], y[ND];
#pragma unroll
   for (int i = 0; i < ND; i++)
   {
      const int g = m[i * kCvWave];
      const double v = x[dof_of(g)];
      u[i] = g >= 0 ? v : -v;
      y[i] = 0.0;
   }
   // (the plane loop is kept rolled: unrolled, the scheduler hoists every plane's qdata loads and spills)
#pragma unroll 1
   for (int qz = 0; qz < Q; qz++)
   {
      // the plane: B_z u and (forward only) G_z u, [dy][dx]
      double bz[D * D], gz[D * D];
#pragma unroll
      for (int i = 0; i < D * D; i++)
      {
         double sb = 0.0, sg = 0.0;
#pragma unroll
         for (int dz = 0; dz < D; dz++)
         {
            sb += b.B[qz + MQ * dz] * u[i + D * D * dz];
            if (!TRANSPOSE) { sg += b.G[qz + MQ * dz] * u[i + D * D * dz]; }
         }
         bz[i] = sb;
         gz[i] = sg;
      }
      // the plane's way back: forward one table (B_z^T of it), transpose two (B_z^T and G_z^T)
      double pb[D * D], pg[D * D];
#pragma unroll
      for (int i = 0; i < D * D; i++) { pb[i] = 0.0; pg[i] = 0.0; }
#pragma unroll
      for (int qy = 0; qy < Q; qy++)
      {
         double bb[D], gb[D], bg[D];  // [dx]: B_y B_z u, G_y B_z u, B_y G_z u
#pragma unroll
         for (int dx = 0; dx < D; dx++)
         {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int dy = 0; dy < D; dy++)
            {
               s0 += b.B[qy + MQ * dy] * bz[dx + D * dy];
               if (!TRANSPOSE)
               {
                  s1 += b.G[qy + MQ * dy] * bz[dx + D * dy];
                  s2 += b.B[qy + MQ * dy] * gz[dx + D * dy];
               }
            }
            bb[dx] = s0;
            gb[dx] = s1;
            bg[dx] = s2;
         }
         double r0[D], r1[D], r2[D];  // the row's way back, [dx]
#pragma unroll
         for (int dx = 0; dx < D; dx++) { r0[dx] = 0.0; r1[dx] = 0.0; r2[dx] = 0.0; }
#pragma unroll
         for (int qx = 0; qx < Q; qx++)
         {
            const int q = (qz * Q + qy) * Q + qx;
            const double p0 = __builtin_nontemporal_load(qp + (size_t)(q * 3 + 0) * kCvWave);
            const double p1 = __builtin_nontemporal_load(qp + (size_t)(q * 3 + 1) * kCvWave);
            const double p2 = __builtin_nontemporal_load(qp + (size_t)(q * 3 + 2) * kCvWave);
            if (!TRANSPOSE)
            {
               double ux = 0.0, uy = 0.0, uz = 0.0;
#pragma unroll
               for (int dx = 0; dx < D; dx++)
               {
                  ux += b.G[qx + MQ * dx] * bb[dx];
                  uy += b.B[qx + MQ * dx] * gb[dx];
                  uz += b.B[qx + MQ * dx] * bg[dx];
               }
               const double v = p0 * ux + p1 * uy + p2 * uz;
#pragma unroll
               for (int dx = 0; dx < D; dx++) { r0[dx] += b.B[qx + MQ * dx] * v; }
            }
            else
            {
               double v = 0.0;
#pragma unroll
               for (int dx = 0; dx < D; dx++) { v += b.B[qx + MQ * dx] * bb[dx]; }
               const double w0 = p0 * v, w1 = p1 * v, w2 = p2 * v;
#pragma unroll
               for (int dx = 0; dx < D; dx++)
               {
                  r0[dx] += b.G[qx + MQ * dx] * w0;
                  r1[dx] += b.B[qx + MQ * dx] * w1;
                  r2[dx] += b.B[qx + MQ * dx] * w2;
               }
            }
         }
#pragma unroll
         for (int dy = 0; dy < D; dy++)
#pragma unroll
            for (int dx = 0; dx < D; dx++)
            {
               if (!TRANSPOSE) { pb[dx + D * dy] += b.B[qy + MQ * dy] * r0[dx]; }
               else
               {
                  pb[dx + D * dy] += b.B[qy + MQ * dy] * r0[dx] + b.G[qy + MQ * dy] * r1[dx];
                  pg[dx + D * dy] += b.B[qy + MQ * dy] * r2[dx];
               }
            }
      }
#pragma unroll
      for (int dz = 0; dz < D; dz++)
#pragma unroll
         for (int i = 0; i < D * D; i++)
         {
            if (!TRANSPOSE) { y[i + D * D * dz] += b.B[qz + MQ * dz] * pb[i]; }
            else { y[i + D * D * dz] += b.B[qz + MQ * dz] * pb[i] + b.G[qz + MQ * dz] * pg[i]; }
         }
   }
   if (blk * kCvWave + lane >= n) { return; }  // a padding lane
   double *o = ye + (size_t)blk * ND * kCvWave + lane;
#pragma unroll
   for (int i = 0; i < ND; i++) { o[i * kCvWave] = y[i]; }
}

template <int D, int Q>
struct CvShape
{
   static constexpr int TS = Q * Q;                 // threads of one element's sheet
   static constexpr int EPB = kCvThreads / TS;      // elements per workgroup
   static constexpr int ND = D * D * D, NQ = Q * Q * Q;
   static constexpr int NX = 2 * D * D * Q;         // x stage: two tables
   static constexpr int NY = 3 * D * Q * Q;         // y stage: three tables
   // the element's LDS slice, an odd number of doubles (neighbouring sheets on different banks)
   static constexpr int ES = (ND + NX + NY) | 1;
};

// p = 3, 4: a Q x Q sheet per element (thread t = qx + Q qy owns the z column of its point).
// Forward: sU -> sX = (B_x u, G_x u) -> sY = (B_y B_x u, B_y G_x u, G_y B_x u) -> the column's
// gradient -> pa . grad -> B^T in z, y, x (k_lform's three stages).  Transpose: B only on the way in;
// on the way back sY = (B_z^T w0, B_z^T w1, G_z^T w2), sX = (B_y^T sY0, G_y^T sY1 + B_y^T sY2), and
// the x stage applies G^T to the first and B^T to the second.
template <int D, int Q, bool TRANSPOSE>
__global__ void __launch_bounds__(kCvThreads) k_conv_apply_sheet(int n, const int *__restrict__ map,
                                                                const double *__restrict__ qd,
                                                                const double *__restrict__ x, double *__restrict__ ye,
                                                                const Basis1D b)
{
   typedef CvShape<D, Q> S;
   constexpr int TS = S::TS, EPB = S::EPB, ND = S::ND, NQ = S::NQ, ES = S::ES, DDQ = D * D * Q, DQQ = D * Q * Q;
   __shared__ double sB[Q * D], sG[Q * D];
   __shared__ double sE[EPB * ES];

   const int tid = threadIdx.x;
   for (int i = tid; i < Q * D; i += kCvThreads)
   {
      sB[i] = b.B[(i % Q) + MQ * (i / Q)];
      sG[i] = b.G[(i % Q) + MQ * (i / Q)];
   }
   const int le = tid / TS, t = tid - le * TS;
   const long k = (long)blockIdx.x * EPB + le;
   const bool valid = le < EPB && k < n;  // this sheet has an element
   double *sU = sE + (valid ? le : 0) * ES;
   double *sX = sU + ND, *sY = sX + S::NX;
   const int qx = t % Q, qy = t / Q;

   if (valid)
   {
      const int *gm = map + k * ND;
      for (int i = t; i < ND; i += TS)
      {
         const int g = gm[i];
         const double v = x[dof_of(g)];
         sU[i] = g >= 0 ? v : -v;
      }
   }
   __syncthreads();  // sB, sG, sU
   if (valid)
   {
      for (int i = t; i < DDQ; i += TS)  // (dz, dy, qx)
      {
         const int ix = i % Q, r = i / Q;
         double u = 0.0, g = 0.0;
#pragma unroll
         for (int dx = 0; dx < D; dx++)
         {
            const double v = sU[r * D + dx];
            u += sB[ix + Q * dx] * v;
            if (!TRANSPOSE) { g += sG[ix + Q * dx] * v; }
         }
         sX[i] = u;
         if (!TRANSPOSE) { sX[DDQ + i] = g; }
      }
   }
   __syncthreads();
   if (valid)
   {
      for (int i = t; i < DQQ; i += TS)  // (dz, qy, qx)
      {
         const int ix = i % Q, iy = (i / Q) % Q, dz = i / (Q * Q);
         double bb = 0.0, gb = 0.0, bg = 0.0;
#pragma unroll
         for (int dy = 0; dy < D; dy++)
         {
            const double u = sX[(dz * D + dy) * Q + ix];
            bb += sB[iy + Q * dy] * u;
            if (!TRANSPOSE)
            {
               gb += sB[iy + Q * dy] * sX[DDQ + (dz * D + dy) * Q + ix];
               bg += sG[iy + Q * dy] * u;
            }
         }
         sY[i] = bb;
         if (!TRANSPOSE)
         {
            sY[DQQ + i] = gb;
            sY[2 * DQQ + i] = bg;
         }
      }
   }
   __syncthreads();
   // the z column: the value or the reference gradient, times pa
   double w0[Q], w1[Q], w2[Q];  // forward: w0 = pa . grad; transpose: pa_c (B u)
#pragma unroll
   for (int qz = 0; qz < Q; qz++) { w0[qz] = 0.0; w1[qz] = 0.0; w2[qz] = 0.0; }
   if (valid)
   {
      double v[Q], gx[Q], gy[Q], gz[Q];
#pragma unroll
      for (int qz = 0; qz < Q; qz++) { v[qz] = 0.0; gx[qz] = 0.0; gy[qz] = 0.0; gz[qz] = 0.0; }
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         const double bb = sY[dz * TS + t];
         const double gb = TRANSPOSE ? 0.0 : sY[DQQ + dz * TS + t];
         const double bg = TRANSPOSE ? 0.0 : sY[2 * DQQ + dz * TS + t];
#pragma unroll
         for (int qz = 0; qz < Q; qz++)
         {
            const double bzv = sB[qz + Q * dz];
            if (TRANSPOSE) { v[qz] += bzv * bb; }
            else
            {
               gx[qz] += bzv * gb;
               gy[qz] += bzv * bg;
               gz[qz] += sG[qz + Q * dz] * bb;
            }
         }
      }
      const double *qe = qd + (size_t)k * 3 * NQ;
#pragma unroll
      for (int qz = 0; qz < Q; qz++)
      {
         const int q = (qz * Q + qy) * Q + qx;
         const double p0 = __builtin_nontemporal_load(qe + q);
         const double p1 = __builtin_nontemporal_load(qe + NQ + q);
         const double p2 = __builtin_nontemporal_load(qe + 2 * NQ + q);
         if (TRANSPOSE)
         {
            w0[qz] = p0 * v[qz];
            w1[qz] = p1 * v[qz];
            w2[qz] = p2 * v[qz];
         }
         else { w0[qz] = p0 * gx[qz] + p1 * gy[qz] + p2 * gz[qz]; }
      }
   }
   __syncthreads();  // sY's readers (the z stage) are done
   if (valid)
   {
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u0 = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
         for (int qz = 0; qz < Q; qz++)
         {
            u0 += sB[qz + Q * dz] * w0[qz];
            if (TRANSPOSE)
            {
               u1 += sB[qz + Q * dz] * w1[qz];
               u2 += sG[qz + Q * dz] * w2[qz];
            }
         }
         sY[dz * TS + t] = u0;
         if (TRANSPOSE)
         {
            sY[DQQ + dz * TS + t] = u1;
            sY[2 * DQQ + dz * TS + t] = u2;
         }
      }
   }
   __syncthreads();
   if (valid)
   {
      for (int i = t; i < DDQ; i += TS)  // (dz, dy, qx)
      {
         const int ix = i % Q, dy = (i / Q) % D, dz = i / (Q * D);
         double u = 0.0, g = 0.0;
#pragma unroll
         for (int iy = 0; iy < Q; iy++)
         {
            const int j = (dz * Q + iy) * Q + ix;
            u += sB[iy + Q * dy] * sY[j];
            if (TRANSPOSE) { g += sG[iy + Q * dy] * sY[DQQ + j] + sB[iy + Q * dy] * sY[2 * DQQ + j]; }
         }
         sX[i] = u;
         if (TRANSPOSE) { sX[DDQ + i] = g; }
      }
   }
   __syncthreads();
   if (valid)
   {
      double *out = ye + k * ND;
      for (int i = t; i < ND; i += TS)  // (dz, dy, dx)
      {
         const int dx = i % D, r = i / D;
         double u = 0.0;
#pragma unroll
         for (int ix = 0; ix < Q; ix++)
         {
            if (TRANSPOSE) { u += sG[ix + Q * dx] * sX[r * Q + ix] + sB[ix + Q * dx] * sX[DDQ + r * Q + ix]; }
            else { u += sB[ix + Q * dx] * sX[r * Q + ix]; }
         }
         out[i] = u;
      }
   }
   (void)qx; (void)qy;
}

__global__ void __launch_bounds__(256) k_conv_add(int nrows, const int *__restrict__ dof, const int *__restrict__ off,
                                                  const int *__restrict__ idx, const double *__restrict__ ye,
                                                  double *__restrict__ y)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= nrows) { return; }
   double s = y[dof[r]];
   for (int k = off[r]; k < off[r + 1]; k++)
   {
      const int j = idx[k];
      s += j >= 0 ? ye[j] : -ye[-1 - j];
   }
   y[dof[r]] = s;
}

template <int D, int Q>
void launch_conv(bool transpose, int n, const int *map, const double *qd, const double *x, double *ye, const Basis1D &b,
                 hipStream_t s)
{
   if constexpr (D <= 3)
   {
      const dim3 grid(grid_for(n, kCvWave)), block(kCvWave);
      if (transpose) { hipLaunchKernelGGL((k_conv_apply_tpe<D, Q, true>), grid, block, 0, s, n, map, qd, x, ye, b); }
      else { hipLaunchKernelGGL((k_conv_apply_tpe<D, Q, false>), grid, block, 0, s, n, map, qd, x, ye, b); }
   }
   else
   {
      const dim3 grid(grid_for(n, CvShape<D, Q>::EPB)), block(kCvThreads);
      if (transpose) { hipLaunchKernelGGL((k_conv_apply_sheet<D, Q, true>), grid, block, 0, s, n, map, qd, x, ye, b); }
      else { hipLaunchKernelGGL((k_conv_apply_sheet<D, Q, false>), grid, block, 0, s, n, map, qd, x, ye, b); }
   }
   ECM2_HIP(hipGetLastError());
}

} // namespace

namespace kern
{

void conv_setup_qdata(const ConvSetupArgs &a, hipStream_t s)
{
   if (a.n == 0) { return; }
   ECM2_VERIFY(a.q1d >= 1 && a.q1d <= MAX_Q1D, ERR_ARG, "convection rule of " << a.q1d << " points");
   ECM2_VERIFY((a.enodes != nullptr) != (a.J != nullptr), ERR_STATE, "the convection term needs corners or Jacobians");
   ECM2_VERIFY(a.act && a.W && a.qd, ERR_INTERNAL, "convection setup arguments");
   const long nq = (long)a.q1d * a.q1d * a.q1d;
   const long nt = a.blocked ? (((long)a.n + kCvWave - 1) / kCvWave) * kCvWave * nq : (long)a.n * nq;
   hipLaunchKernelGGL(k_conv_setup, dim3(grid_for(nt, 256)), dim3(256), 0, s, a);
   ECM2_HIP(hipGetLastError());
}

// ConvectionIntegrator's specialisations (bilininteg_convection_pa.cpp:30-58) for p = 1..4
bool has_conv_apply(int D, int Q) { return D >= 2 && D <= 5 && (Q == D || Q == D + 1); }
bool conv_blocked(int D) { return D <= 3; }

void conv_apply(int D, int Q, bool transpose, int n, const int *map, const double *qd, const double *x, double *ye,
                const Basis1D &b, hipStream_t s)
{
   ECM2_VERIFY(has_conv_apply(D, Q), ERR_UNSUPPORTED, "no convection kernel for D1D=" << D << " Q1D=" << Q);
   if (n == 0) { return; }
#define ECM2_CV_CASE(d, q) if (D == d && Q == q) { launch_conv<d, q>(transpose, n, map, qd, x, ye, b, s); return; }
   ECM2_CV_CASE(2, 2) ECM2_CV_CASE(2, 3) ECM2_CV_CASE(3, 3) ECM2_CV_CASE(3, 4)
   ECM2_CV_CASE(4, 4) ECM2_CV_CASE(4, 5) ECM2_CV_CASE(5, 5) ECM2_CV_CASE(5, 6)
#undef ECM2_CV_CASE
   ECM2_VERIFY(false, ERR_INTERNAL, "convection kernel table");
}

void conv_add(int nrows, const int *dof, const int *off, const int *idx, const double *ye, double *y, hipStream_t s)
{
   if (nrows == 0) { return; }
   hipLaunchKernelGGL(k_conv_add, dim3(grid_for(nrows, 256)), dim3(256), 0, s, nrows, dof, off, idx, ye, y);
   ECM2_HIP(hipGetLastError());
}

} // namespace kern
} // namespace ecm2
