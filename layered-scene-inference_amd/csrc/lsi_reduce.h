// Reproducible sums for the kernels that reduce an image to a few scalars.  No
// atomics, every order fixed: the same inputs give the same bits on every run.
//
//   image-wide   a grid of at most MAXBLK blocks of TPB threads, per-thread
//                fp32 sums, per-block (block_store_partials) and final
//                (block_total) sums in fp64: lsi_loss.hip, lsi_eval.hip,
//                lsi_ssim.hip, lsi_depth_metrics.hip.
//   per-plane    a plane-aligned grid of bpp <= MAXBPP blocks per plane, three
//                sums per plane (plane_store_partials), then ONE block
//                (plane_finish_kernel) that writes the plane sums and the mean
//                of the planes' terms: lsi_edge_smooth.hip, lsi_depth_sup.hip,
//                lsi_geo_cons.hip, lsi_photo_reproj.hip.
//
// rc_of_launch() is here for all eight, sgn() for lsi_loss.hip and the four
// per-plane losses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace lsi {

constexpr int TPB = 256;
constexpr int MAXBLK = 2048;  // partial sums per scalar
constexpr int MAXBPP = 256;   // blocks (partial sums) per plane, at most
constexpr int FIN_TPB = 1024;
static_assert(MAXBPP <= 4 * 64, "plane_finish_kernel reads four partial sums per lane");

// What an entry point returns after its last launch.
inline int rc_of_launch() {
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

__device__ __forceinline__ float sgn(float v) {
  return (float)(v > 0.0f) - (float)(v < 0.0f);
}

// Blocks of a grid-stride pass over n items.
inline int grid_for(long n) {
  long g = (n + TPB - 1) / TPB;
  if (g > MAXBLK) g = MAXBLK;
  if (g < 1) g = 1;
  return (int)g;
}

__device__ __forceinline__ double wave_total(double t) {
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  return t;  // lane 0 holds the total
}

// The block's wave sums of NV per-thread values (widened first) to sm[k][wave].
template <int NV, class T>
__device__ __forceinline__ void block_wave_sums(const T (&v)[NV],
                                                double (&sm)[NV][TPB / 64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double x = wave_total((double)v[k]);
    if (lane == 0) sm[k][wave] = x;
  }
  __syncthreads();
}

__device__ __forceinline__ double waves_in_order(const double (&w)[TPB / 64]) {
  double s = 0.0;
  for (int i = 0; i < TPB / 64; ++i) s += w[i];
  return s;
}

// Block-wide sum of NV per-thread values; thread 0 stores them (fp64) to
// part[v * stride + blockIdx.x] (stride: the partial sums kept per scalar).
template <int NV>
__device__ __forceinline__ void block_store_partials(const float (&v)[NV],
                                                     double* part,
                                                     int stride = MAXBLK) {
  __shared__ double sm[NV][TPB / 64];
  block_wave_sums(v, sm);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
      part[(size_t)k * stride + blockIdx.x] = waves_in_order(sm[k]);
  }
}

// The same for block bx of the bpp blocks of plane p: thread k < NV stores
// scalar k to part[(k * planes + p) * bpp + bx].
template <int NV, class T>
__device__ __forceinline__ void plane_store_partials(const T (&v)[NV], double* part,
                                                     int planes, int p, int bpp,
                                                     int bx) {
  __shared__ double sm[NV][TPB / 64];
  block_wave_sums(v, sm);
  if (threadIdx.x < NV)
    part[((size_t)threadIdx.x * planes + p) * bpp + bx] = waves_in_order(sm[threadIdx.x]);
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

// Doubles of the per-plane workspace: part (3 * planes * bpp) | terms (planes).
inline size_t plane_ws_doubles(size_t planes, int bpp) {
  return 3 * planes * bpp + planes;
}

// One block of FIN_TPB threads.  Wave w adds up the planes w, w + 16, ...: lane j
// the partial sums j, j + 64, j + 128, j + 192 of each of the three scalars (12
// independent loads, issued together: a chain of dependent loads across XCDs
// costs a microsecond per link), then a shuffle tree; lane 0 writes the plane's
// three sums to plane_sums[3 p ..] and its term to terms[p].  Wave 0 then adds
// the terms and counts the planes S the same way; the loss is their mean.
// Term: bool counts(const double* s), whether a plane with the sums s[0 .. 2]
// enters the mean, and double term(const double* s), its term if it does.
template <class Term>
__global__ __launch_bounds__(FIN_TPB) void plane_finish_kernel(Term f, int planes, int bpp,
                                                               const double* part,
                                                               double* terms,
                                                               double* plane_sums,
                                                               float* out_loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = wave; p < planes; p += FIN_TPB / 64) {
    double v[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double* q = part + ((size_t)k * planes + p) * bpp;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = (lane + 64 * j < bpp) ? q[lane + 64 * j] : 0.0;
    }
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      s[k] = wave_total(((v[k][0] + v[k][1]) + v[k][2]) + v[k][3]);
    if (lane == 0) {
      plane_sums[3 * (size_t)p + 0] = s[0];
      plane_sums[3 * (size_t)p + 1] = s[1];
      plane_sums[3 * (size_t)p + 2] = s[2];
      terms[p] = f.counts(s) ? f.term(s) : 0.0;
    }
  }
  __syncthreads();  // terms[] and plane_sums[] of every wave are visible to wave 0
  if (wave == 0) {
    double t = 0.0, S = 0.0;
    for (int i = lane; i < planes; i += 64) {
      t += terms[i];
      S += f.counts(plane_sums + 3 * (size_t)i) ? 1.0 : 0.0;
    }
    t = wave_total(t);
    S = wave_total(S);
    if (lane == 0) *out_loss = S > 0.0 ? (float)(t / S) : 0.0f;
  }
}

// Launches it on part | terms of the workspace `ws`.
template <class Term>
inline void plane_finish(const Term& f, int planes, int bpp, void* ws, double* plane_sums,
                         float* out_loss, hipStream_t s) {
  const double* part = (const double*)ws;
  hipLaunchKernelGGL(plane_finish_kernel<Term>, dim3(1), dim3(FIN_TPB), 0, s, f, planes,
                     bpp, part, (double*)ws + 3 * (size_t)planes * bpp, plane_sums,
                     out_loss);
}

}  // namespace lsi
