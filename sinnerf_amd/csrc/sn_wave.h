// sn_wave.h -- the wave and block reductions of the per-ray stages and the losses (gfx950, 64-lane waves, blocks of 256 threads).
//
// Every helper here carries the numerical contract the tests hold the kernels to: accumulation in the type it is given (fp64 for every
// floating-point sum), a FIXED combination order, nothing rounded in between -- so a result has the same bits on every call and on every
// grid.  A new stage or loss calls these; it does not write its own butterfly, scan or partials loop.
#pragma once
#include "sn_device.h"

namespace snwv {

// butterfly sum over the 64 lanes; the result is in every lane.  T: double or int
template <typename T>
SN_DEV T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// inclusive scans over the 64 lanes (Hillis-Steele); lane = threadIdx.x & 63.  T: double or int
template <typename T>
SN_DEV T wave_incl_scan_add(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}
SN_DEV double wave_incl_scan_mul(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(v, off, 64);
    if (lane >= off) v *= o;
  }
  return v;
}

// sum over the 256 threads of a block: the butterfly of each wave, then the four waves left to right.  All 256 threads call it; the
// result is valid in every thread.  sh: 4 doubles of LDS, free again after the call (the first barrier covers the previous call's reads)
SN_DEV double block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// phase 1 of a deterministic reduction over a grid: this block's record of NS sums goes to partials[blockIdx.x * NS + k]
template <int NS>
SN_DEV void write_block_partials(const double (&a)[NS], double* sh, double* __restrict__ partials) {
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double v = block_sum(a[k], sh);
    if (threadIdx.x == 0) partials[(long)blockIdx.x * NS + k] = v;
  }
}

// phase 2: one block adds the n_partials records in index order -- thread t takes the records t, t + 256, ... in turn, then block_sum.
// The totals are valid in every thread.
// For n_partials <= 256 this gives the bits of the form `block_sum(t < n_partials ? partials[t * NS + k] : 0.0)`: a thread with a
// record computes 0.0 + p, and that is p bit for bit unless p is -0.0.  No partial is ever -0.0: every accumulator behind one starts at
// +0.0, and a round-to-nearest addition gives -0.0 only from two -0.0 operands.
template <int NS>
SN_DEV void sum_partials(const double* __restrict__ partials, long n_partials, double* sh, double (&tot)[NS]) {
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = 0.0;
    for (long i = threadIdx.x; i < n_partials; i += 256) v += partials[i * NS + k];
    tot[k] = block_sum(v, sh);
  }
}

}  // namespace snwv
