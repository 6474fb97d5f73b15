// Reproducible sums for the kernels that reduce an image to a few scalars
// (lsi_loss.hip, lsi_eval.hip): a grid of at most MAXBLK blocks of TPB threads,
// per-thread fp32 sums, per-block and final sums in fp64 in a fixed order.  No
// atomics: the same inputs give the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsi {

constexpr int TPB = 256;
constexpr int MAXBLK = 2048;  // partial sums per scalar

// Blocks of a grid-stride pass over n items.
inline int grid_for(long n) {
  long g = (n + TPB - 1) / TPB;
  if (g > MAXBLK) g = MAXBLK;
  if (g < 1) g = 1;
  return (int)g;
}

// Block-wide sum of NV per-thread values; thread 0 stores them (fp64) to
// part[v * stride + blockIdx.x] (stride: the partial sums kept per scalar).
template <int NV>
__device__ __forceinline__ void block_store_partials(const float (&v)[NV],
                                                     double* part,
                                                     int stride = MAXBLK) {
  __shared__ double sm[NV][TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double x = (double)v[k];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) sm[k][wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double s = 0.0;
      for (int w = 0; w < TPB / 64; ++w) s += sm[k][w];
      part[(size_t)k * stride + blockIdx.x] = s;
    }
  }
}

// The sum of part[0 .. nblk) by ONE block of TPB threads: a strided sum per
// thread, then a tree over `sm` (TPB doubles of LDS).  Every thread of the block
// calls it and gets the total; `sm` may be reused right after.
__device__ __forceinline__ double block_total(const double* part, int nblk,
                                              double* sm) {
  double x = 0.0;
  for (int i = threadIdx.x; i < nblk; i += TPB) x += part[i];
  sm[threadIdx.x] = x;
  __syncthreads();
  for (int off = TPB / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

}  // namespace lsi
