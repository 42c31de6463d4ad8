// reduce.h -- the fixed-order block reductions of the small kernels.  Every result is the same bits
// on every run; the ORDER of each helper is its contract (tests pin bits against it), and the two
// families below add in different orders: do not express one through the other.
#pragma once
#include <hip/hip_runtime.h>

namespace aq {

// ---- butterfly, then the wave results in order.  Any block of whole waves (<= 1024 threads);
// red: LDS, one double per wave; every thread calls, every thread gets the result.

// Sum of v over the block.  Order: within each wave an xor butterfly over the lane offsets 32, 16,
// 8, 4, 2, 1 (every lane ends with the same wave sum); lane 0 of wave w writes red[w]; then every
// thread adds red[0], red[1], ... red[nwaves - 1] in ascending order, starting from 0.
// (The first barrier keeps a previous call's readers of red ahead of this call's writers.)
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += red[k];
  return t;
}
// the larger of two values, NaN if either is
__device__ __forceinline__ double nan_max(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
// Maximum of v over the block, NaN if any v is.  Order: block_sum's with nan_max for +, the wave
// results combined from red[0] upwards (a maximum is exact in any order; which NaN survives is not).
__device__ __forceinline__ double block_max_nan(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) t = nan_max(t, red[k]);
  return t;
}

// ---- LDS halving tree.  A block of NT threads (a power of two) over NT doubles already written
// and fenced by a __syncthreads(); the result is in element 0 after the call, for every thread.

// red[0] = the sum of red[0..NT).  Order: for w = NT/2, NT/4, ... 1, thread t < w does
// red[t] += red[t + w], a barrier after each level.
template <int NT>
__device__ __forceinline__ void block_tree_sum(double* red) {
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
}
// a[0], b[0] = the minima of a[0..NT), b[0..NT): the same tree with fmin on both arrays (exact in
// any order; NaN-ignoring as fmin is).
template <int NT>
__device__ __forceinline__ void block_tree_min2(double* a, double* b) {
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      a[threadIdx.x] = fmin(a[threadIdx.x], a[threadIdx.x + s]);
      b[threadIdx.x] = fmin(b[threadIdx.x], b[threadIdx.x + s]);
    }
    __syncthreads();
  }
}

}  // namespace aq
