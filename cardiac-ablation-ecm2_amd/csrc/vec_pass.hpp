// vec_pass.hpp -- the 16-byte vector passes of the device solvers (k_pcg.hip, k_cheb.hip, k_mg.hip, k_bicgstab.hip, k_ess.hip) and of the cell-death state (k_celldeath.hip):
// an FP64 vector is read and written two entries at a time, and one thread takes entry n - 1 of an odd n.  A pass
// states its arithmetic per entry once, as a body `[&](auto k) { ... }` that reaches its vectors through ld / st /
// dot_acc only: called with a Pair it works on v2d, called with an Entry on double, the same operations in the same
// order, so the tail entry rounds as every other one does.  Included by .hip files only.
#pragma once

#include "dev_common.hpp"

namespace ecm2
{
namespace dev
{

// One thread's pairs i = t, t + stride, ... < n / 2 of a grid-stride sweep over an FP64 vector read two entries at a
// time; the thread stride - 1 also takes entry n - 1 of an odd n.
struct Sweep
{
   long n2, stride, t;
   bool tail;
   __device__ explicit Sweep(int n)
      : n2(n / 2), stride((long)gridDim.x * blockDim.x), t((long)blockIdx.x * blockDim.x + threadIdx.x),
        tail((n & 1) && t == stride - 1)
   {
   }
};

// Its flat counterpart, a grid of n / 2 + 1 threads: thread t < n / 2 takes pair t, thread n / 2 entry n - 1 of an
// odd n; a thread with t > n2 has nothing to do (the kernels return on it before they read their scalars).
struct Flat
{
   long n2, t;
   bool tail;
   __device__ explicit Flat(int n)
      : n2(n / 2), t((long)blockIdx.x * blockDim.x + threadIdx.x), tail((n & 1) && t == n2)
   {
   }
};

struct Pair { long i; };   // entries 2 i, 2 i + 1
struct Entry { long i; };  // entry i

__device__ inline const v2d *as2(const double *p) { return reinterpret_cast<const v2d *>(p); }
__device__ inline v2d *as2(double *p) { return reinterpret_cast<v2d *>(p); }

__device__ __forceinline__ v2d ld(const double *p, Pair k) { return as2(p)[k.i]; }
__device__ __forceinline__ double ld(const double *p, Entry k) { return p[k.i]; }
__device__ __forceinline__ void st(double *p, Pair k, v2d v) { as2(p)[k.i] = v; }
__device__ __forceinline__ void st(double *p, Entry k, double v) { p[k.i] = v; }

// s += a . b, a pair's two products in index order
__device__ __forceinline__ void dot_acc(double &s, v2d a, v2d b)
{
   s += a.x * b.x;
   s += a.y * b.y;
}
__device__ __forceinline__ void dot_acc(double &s, double a, double b) { s += a * b; }

// The body over the thread's share of [0, n): its pairs, then (the tail thread) entry n - 1 in scalars.
template <class Body>
__device__ __forceinline__ void each_entry(const Sweep &w, int n, Body &&body)
{
   for (long i = w.t; i < w.n2; i += w.stride) { body(Pair{i}); }
   if (w.tail) { body(Entry{(long)n - 1}); }
}

template <class Body>
__device__ __forceinline__ void each_entry(const Flat &w, int n, Body &&body)
{
   if (w.t < w.n2) { body(Pair{w.t}); }
   else if (w.tail) { body(Entry{(long)n - 1}); }
}

} // namespace dev
} // namespace ecm2
