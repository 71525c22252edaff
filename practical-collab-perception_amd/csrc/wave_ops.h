// Wave and workgroup scan / reduce primitives of libpcp_hip.so, once (gfx950 only: wavefront = 64).  Device code only.
// The xor form (wave_sum) and the shift-down form (inside block_sum_lane0) give lane 0 the same bits but are different instructions: a
// kernel keeps the one it was written with.  A loop that is still written out in a kernel says why beside it: as a call it would
// change that kernel's instruction schedule (profiles/wave_ops_refactor.txt).
#pragma once
#include <hip/hip_runtime.h>

// inclusive scan in lane order; lane = threadIdx.x & 63
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// xor butterfly: every lane holds the total
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// minimum of a 64-bit key over the wave (two 32-bit shuffles per step); every lane holds it
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), d, 64), hi = __shfl_xor((unsigned)(v >> 32), d, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// exclusive scan over the THREADS threads of the block; *total receives the block sum. scratch: >= THREADS / 64 + 1 ints of LDS.
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int *scratch, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v, lane);
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int w = threadIdx.x < THREADS / 64 ? scratch[threadIdx.x] : 0;
    const int wi = wave_incl_scan(w, lane);
    if (threadIdx.x < THREADS / 64) scratch[threadIdx.x] = wi - w;
    if (threadIdx.x == THREADS / 64 - 1) scratch[THREADS / 64] = wi;
  }
  __syncthreads();
  const int res = scratch[wave] + incl - v;
  *total = scratch[THREADS / 64];
  __syncthreads();
  return res;
}

// float64 sum over the block (any size up to 1024 threads); sh: one double per wave.  Valid on thread 0.
__device__ __forceinline__ double block_sum_lane0(double v, double *sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);          // no width argument: __shfl_down(v, o, 64) compiles to other instructions
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  double t = 0;
  if (threadIdx.x == 0) for (unsigned w = 0; w < (blockDim.x + 63) / 64; ++w) t += sh[w];
  return t;
}
