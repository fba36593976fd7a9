// k_lform.hip -- the device linear form (gfx950): one fused kernel per (D1D, Q1D) computes every
// element's vector  be[e][nd] = B^T (x) B^T (x) B^T (W_q f_q det J_q)  of a DomainLFIntegrator --
// the reference's DLFEvalAssemble3D (fem/integ/lininteg_domain_kernels.hpp:164-300, map_type ==
// VALUE) -- with the source coefficient f_q and the geometry evaluated in the same kernel: no
// per-point array is stored unless the caller supplied one (COEFF_QUAD).
//
// Thread mapping: the reference's (one Q1D x Q1D thread sheet per element, z columns in registers),
// but a 256-thread workgroup holds 256 / Q1D^2 such sheets -- 64 elements at p = 1 (Q1D = 2), 28 at
// p = 2 (Q1D = 3), 7 at p = 4 (Q1D = 6) -- so that a 4- to 36-point sheet does not leave a 64-lane
// wave mostly idle.  Every 1D stage goes through the element's own LDS slice; the workgroup's
// barriers are uniform (elements past ne or excluded by a marker run the stages on in-bounds
// data and write zeros).
//
// Source kinds (LFormArgs::kind): COEFF_CONSTANT, COEFF_QUAD, COEFF_GRIDFUNC, COEFF_GRIDFUNC_AFFINE
// (the field gathered through the map and interpolated with B, then coeff_law), and COEFF_JOULE:
// f = sigma0 (1 + slope (T_q - t_ref)) |grad phi|^2_q with the reference gradient of phi interpolated
// with G and mapped by grad phi = J^-T grad_ref phi = adj(J)^T grad_ref phi / det J
// (GradientGridFunctionCoefficient into InnerProductCoefficient, fem/coefficient.hpp:872, :1760;
// JouleHeatingCoefficient::Eval, miniapps/electromagnetics/joule_solver.cpp:898).
//
// Geometry: the element's 8 lexicographic corners (the trilinear map's J, adj(J), det J at each
// point, the algebra of QLAYOUT_TRILINEAR) or MFEM-layout Jacobians J(q, i, j, e).
//
// No atomics anywhere: the E-vector is summed by the CSR transpose (kern::restriction_mult_transpose),
// so two Assembles of the same inputs are bitwise equal.
#include "dev_common.hpp"

namespace ecm2
{
namespace
{
using namespace dev;

constexpr int kLfThreads = 256;

// source evaluation the kernel is compiled for
enum LfMode : int { LF_POINT = 0,   // constant or per-point values: no field
                    LF_VALUE = 1,   // a law of one interpolated field
                    LF_JOULE = 2 }; // sigma(T) |grad phi|^2

template <int D, int Q, int MODE, int GEOM>
struct LfShape
{
   static constexpr int TS = Q * Q;                 // threads of one element's sheet
   static constexpr int EPB = kLfThreads / TS;      // elements per workgroup
   static constexpr int ND = D * D * D, NQ = Q * Q * Q;
   static constexpr int NX = (MODE == LF_JOULE ? 2 : 1) * D * D * Q;  // x-stage: (B u [, G u])
   static constexpr int NY = (MODE == LF_JOULE ? 3 : 1) * D * Q * Q;  // y-stage: (BB u [, GB u, BG u])
   static constexpr int NC = GEOM == 0 ? 21 : 0;    // trilinear-map coefficients c1..c7 of x, y, z
   // the element's LDS slice, an odd number of doubles (neighbouring sheets on different banks)
   static constexpr int ES = (ND + NX + NY + NC) | 1;
};

// One field of the element (sU[ND], lexicographic) to the quadrature points of this thread's z
// column: v[qz] = the value, and with GRAD the reference gradient (gx, gy, gz)[qz].  Stages x and y
// through sX / sY.  Called by the whole workgroup (two barriers inside; the caller has synchronised
// sU, and synchronises before it next writes sX / sY).
template <int D, int Q, bool GRAD>
__device__ __forceinline__ void lf_interp(bool valid, int t, const double *sB, const double *sG, const double *sU,
                                          double *sX, double *sY, double (&v)[Q], double (&gx)[Q], double (&gy)[Q],
                                          double (&gz)[Q])
{
   constexpr int TS = Q * Q, DDQ = D * D * Q, DQQ = D * Q * Q;
   if (valid)
   {
      for (int i = t; i < DDQ; i += TS)  // (dz, dy, qx)
      {
         const int qx = i % Q, r = i / Q;
         double u = 0.0, g = 0.0;
#pragma unroll
         for (int dx = 0; dx < D; dx++)
         {
            const double x = sU[r * D + dx];
            u += sB[qx + Q * dx] * x;
            if (GRAD) { g += sG[qx + Q * dx] * x; }
         }
         sX[i] = u;
         if (GRAD) { sX[DDQ + i] = g; }
      }
   }
   __syncthreads();
   if (valid)
   {
      for (int i = t; i < DQQ; i += TS)  // (dz, qy, qx)
      {
         const int qx = i % Q, qy = (i / Q) % Q, dz = i / (Q * Q);
         double bb = 0.0, gb = 0.0, bg = 0.0;
#pragma unroll
         for (int dy = 0; dy < D; dy++)
         {
            const double u = sX[(dz * D + dy) * Q + qx];
            bb += sB[qy + Q * dy] * u;
            if (GRAD)
            {
               gb += sB[qy + Q * dy] * sX[DDQ + (dz * D + dy) * Q + qx];
               bg += sG[qy + Q * dy] * u;
            }
         }
         sY[i] = bb;
         if (GRAD)
         {
            sY[DQQ + i] = gb;
            sY[2 * DQQ + i] = bg;
         }
      }
   }
   __syncthreads();
#pragma unroll
   for (int qz = 0; qz < Q; qz++) { v[qz] = 0.0; gx[qz] = 0.0; gy[qz] = 0.0; gz[qz] = 0.0; }
   if (valid)
   {
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         const double bb = sY[dz * TS + t];
         const double gb = GRAD ? sY[DQQ + dz * TS + t] : 0.0;
         const double bg = GRAD ? sY[2 * DQQ + dz * TS + t] : 0.0;
#pragma unroll
         for (int qz = 0; qz < Q; qz++)
         {
            const double bz = sB[qz + Q * dz];
            v[qz] += bz * bb;
            if (GRAD)
            {
               gx[qz] += bz * gb;
               gy[qz] += bz * bg;
               gz[qz] += sG[qz + Q * dz] * bb;
            }
         }
      }
   }
}

// the element's field through the gather map (orientation signs as ElementRestriction::Mult)
template <int ND, int TS>
__device__ __forceinline__ void lf_gather(bool valid, int t, const int *__restrict__ gm, const double *__restrict__ x,
                                          double *sU)
{
   if (valid)
   {
      for (int i = t; i < ND; i += TS)
      {
         const int g = gm[i];
         const double v = x[dof_of(g)];
         sU[i] = g >= 0 ? v : -v;
      }
   }
}

template <int D, int Q, int MODE, int GEOM>
__global__ void __launch_bounds__(kLfThreads) k_lform(const kern::LFormArgs a, const Basis1D b)
{
   typedef LfShape<D, Q, MODE, GEOM> S;
   constexpr int TS = S::TS, EPB = S::EPB, ND = S::ND, NQ = S::NQ, ES = S::ES, DDQ = D * D * Q, DQQ = D * Q * Q;
   __shared__ double sB[Q * D], sG[Q * D];
   __shared__ double sE[EPB * ES];

   const int tid = threadIdx.x;
   for (int i = tid; i < Q * D; i += kLfThreads)
   {
      sB[i] = b.B[(i % Q) + MQ * (i / Q)];
      sG[i] = b.G[(i % Q) + MQ * (i / Q)];
   }
   const int le = tid / TS, t = tid - le * TS;
   const long e = (long)blockIdx.x * EPB + le;
   const bool valid = le < EPB && e < a.ne;                      // this sheet has an element
   const bool active = valid && (!a.emark || a.emark[e] != 0);   // ... that the integrator's marker keeps
   double *sU = sE + (valid ? le : 0) * ES;
   double *sX = sU + ND, *sY = sX + S::NX, *sC = sY + S::NY;
   const int *gm = a.gmap + (valid ? e : 0) * ND;
   const int qx = t % Q, qy = t / Q;

   if (GEOM == 0 && valid)
   {
      // x_i = c0 + c1 xi + c2 eta + c3 zeta + c4 xi eta + c5 xi zeta + c6 eta zeta + c7 xi eta zeta
      // from the corners a = ax + 2 ay + 4 az (kernels.hpp TRILINEAR); sC[3 (k - 1) + i] = c_k of x_i
      for (int i = t; i < 21; i += TS)
      {
         const int k = i / 3 + 1;
         const double *X = a.enodes + (e * 3 + (i % 3)) * 8;
         double c;
         switch (k)
         {
            case 1: c = X[1] - X[0]; break;
            case 2: c = X[2] - X[0]; break;
            case 3: c = X[4] - X[0]; break;
            case 4: c = (X[3] - X[2]) - (X[1] - X[0]); break;
            case 5: c = (X[5] - X[4]) - (X[1] - X[0]); break;
            case 6: c = (X[6] - X[4]) - (X[2] - X[0]); break;
            default: c = ((X[7] - X[6]) - (X[5] - X[4])) - ((X[3] - X[2]) - (X[1] - X[0])); break;
         }
         sC[i] = c;
      }
   }

   double fv[Q], gx[Q], gy[Q], gz[Q];  // the z column: field value (or T), reference gradient of phi
   (void)fv; (void)gx; (void)gy; (void)gz;
   if (MODE == LF_POINT)
   {
      __syncthreads();  // sB, sG, sC
   }
   else
   {
      lf_gather<ND, TS>(valid, t, gm, a.lvec, sU);
      __syncthreads();  // sB, sG, sC, sU
      lf_interp<D, Q, MODE == LF_JOULE>(valid, t, sB, sG, sU, sX, sY, fv, gx, gy, gz);
      if (MODE == LF_JOULE && a.lvec2)  // (uniform over the launch)
      {
         double d0[Q], d1[Q], d2[Q];
         lf_gather<ND, TS>(valid, t, gm, a.lvec2, sU);  // (sU was last read before lf_interp's first barrier)
         __syncthreads();
         lf_interp<D, Q, false>(valid, t, sB, sG, sU, sX, sY, fv, d0, d1, d2);
      }
   }

   // f_q, the geometry and W_q f_q det J_q down this thread's z column
   double w[Q];
#pragma unroll
   for (int qz = 0; qz < Q; qz++)
   {
      w[qz] = 0.0;
      if (!valid) { continue; }
      const int q = (qz * Q + qy) * Q + qx;
      double J[3][3];
      if (GEOM == 0) { trilinear_jacobian(sC, a.qp.x[qx], a.qp.x[qy], a.qp.x[qz], J); }
      else
      {
#pragma unroll
         for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) { J[i][j] = a.J[q + (size_t)NQ * (i + 3 * (j + 3 * (size_t)e))]; }
      }
      double A[3][3];
      adj3(J, A);
      const double det = J[0][0] * A[0][0] + J[0][1] * A[1][0] + J[0][2] * A[2][0];
      double f;
      if (MODE == LF_POINT) { f = a.kind == COEFF_QUAD ? a.quad[(size_t)e * NQ + q] : a.value; }
      else if (MODE == LF_VALUE) { f = coeff_law(a.kind, fv[qz], a.scale, a.slope, a.t_ref, nullptr); }
      else
      {
         // grad phi = adj(J)^T grad_ref phi / det J
         const double p0 = A[0][0] * gx[qz] + A[1][0] * gy[qz] + A[2][0] * gz[qz];
         const double p1 = A[0][1] * gx[qz] + A[1][1] * gy[qz] + A[2][1] * gz[qz];
         const double p2 = A[0][2] * gx[qz] + A[1][2] * gy[qz] + A[2][2] * gz[qz];
         const double sigma = a.lvec2 ? a.scale * (1.0 + a.slope * (fv[qz] - a.t_ref)) : a.scale;
         f = sigma * ((p0 * p0 + p1 * p1 + p2 * p2) / (det * det));
      }
      w[qz] = a.W[q] * f * det;
   }

   // B^T in z, y, x (DLFEvalAssemble3D's three stages)
   __syncthreads();  // sY's readers (lf_interp's z stage) are done
   if (valid)
   {
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { u += sB[qz + Q * dz] * w[qz]; }
         sY[dz * TS + t] = u;
      }
   }
   __syncthreads();
   if (valid)
   {
      for (int i = t; i < DDQ; i += TS)  // (dz, dy, qx)
      {
         const int x = i % Q, dy = (i / Q) % D, dz = i / (Q * D);
         double u = 0.0;
#pragma unroll
         for (int y = 0; y < Q; y++) { u += sB[y + Q * dy] * sY[(dz * Q + y) * Q + x]; }
         sX[i] = u;
      }
   }
   __syncthreads();
   if (valid)
   {
      double *out = a.be + e * ND;
      for (int i = t; i < ND; i += TS)  // (dz, dy, dx)
      {
         const int dx = i % D, r = i / D;
         double u = 0.0;
#pragma unroll
         for (int x = 0; x < Q; x++) { u += sB[x + Q * dx] * sX[r * Q + x]; }
         out[i] = active ? u : 0.0;  // an excluded element: the reference's zeroed E-vector
      }
   }
   (void)DQQ;
}

template <int D, int Q>
void launch_lform(const kern::LFormArgs &a, const Basis1D &b, hipStream_t s)
{
   const int mode = a.kind == COEFF_JOULE ? LF_JOULE : (a.kind == COEFF_CONSTANT || a.kind == COEFF_QUAD) ? LF_POINT : LF_VALUE;
   const unsigned grid = grid_for(a.ne, LfShape<D, Q, 0, 0>::EPB);
#define ECM2_LF_LAUNCH(M, G) hipLaunchKernelGGL((k_lform<D, Q, M, G>), dim3(grid), dim3(kLfThreads), 0, s, a, b)
   if (a.J)
   {
      if (mode == LF_JOULE) { ECM2_LF_LAUNCH(LF_JOULE, 1); }
      else if (mode == LF_VALUE) { ECM2_LF_LAUNCH(LF_VALUE, 1); }
      else { ECM2_LF_LAUNCH(LF_POINT, 1); }
   }
   else
   {
      if (mode == LF_JOULE) { ECM2_LF_LAUNCH(LF_JOULE, 0); }
      else if (mode == LF_VALUE) { ECM2_LF_LAUNCH(LF_VALUE, 0); }
      else { ECM2_LF_LAUNCH(LF_POINT, 0); }
   }
#undef ECM2_LF_LAUNCH
   ECM2_HIP(hipGetLastError());
}

} // namespace

namespace kern
{

// DomainLFIntegrator's specialisations (lininteg_domain.cpp:104-115: p = 1..4 with p + 1 and p + 2
// points) plus the forms' p = 1, Q1D = 3 rule
bool has_lform(int D, int Q) { return D >= 2 && D <= 5 && (Q == D || Q == D + 1); }

void lform_element_vectors(int D, int Q, const LFormArgs &a, const Basis1D &b, hipStream_t s)
{
   ECM2_VERIFY(has_lform(D, Q), ERR_UNSUPPORTED, "no linear-form kernel for D1D=" << D << " Q1D=" << Q);
   ECM2_VERIFY(a.kind == COEFF_CONSTANT || a.kind == COEFF_QUAD || a.kind == COEFF_GRIDFUNC ||
               a.kind == COEFF_GRIDFUNC_AFFINE || a.kind == COEFF_JOULE, ERR_ARG,
               "coefficient kind " << a.kind << " is not a linear-form source");
   if (a.ne == 0) { return; }
   ECM2_VERIFY((a.enodes != nullptr) != (a.J != nullptr), ERR_STATE, "the linear form needs corners or Jacobians");
#define ECM2_LF_CASE(d, q) if (D == d && Q == q) { launch_lform<d, q>(a, b, s); return; }
   ECM2_LF_CASE(2, 2) ECM2_LF_CASE(2, 3) ECM2_LF_CASE(3, 3) ECM2_LF_CASE(3, 4)
   ECM2_LF_CASE(4, 4) ECM2_LF_CASE(4, 5) ECM2_LF_CASE(5, 5) ECM2_LF_CASE(5, 6)
#undef ECM2_LF_CASE
   ECM2_VERIFY(false, ERR_INTERNAL, "linear-form kernel table");
}

} // namespace kern
} // namespace ecm2
