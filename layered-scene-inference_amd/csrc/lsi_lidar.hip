// LiDAR scans rasterised into depth maps on the device (gfx950): every point of
// a scan is projected by a 3 x 4 matrix per view, the nearest return per pixel
// is kept in a z-buffer, and an optional occlusion filter drops returns that a
// much nearer neighbour says are seen through a foreground edge.  No reference
// counterpart; the definition is DESIGN.md section 4.19 and the header's
// comment.  All arithmetic is fp32 in the stated order without contraction
// (explicit __f*_rn, correctly rounded division), and the z-buffer is an
// unsigned minimum on the bits of positive floats, so the result is a function
// of the input alone, whatever order points and threads arrive in.
//
// Kernels and what bounds them (one call, in launch order):
//   (memset)         the z-buffer to 0xffffffff, "empty": above every float.
//   scatter_kernel   a thread per point, a grid row per scan (sized on the host
//                    from the longest scan; no offset table is searched).  One
//                    aligned 16-byte load per point (the compiler fetches the 12
//                    bytes used); the scan's descriptor and its V
//                    matrices are uniform loads (scalar registers).  One
//                    no-return atomic umin per kept point and view.  Bound by
//                    launch latency and the atomics; 16 B per point of HBM
//                    traffic.
//   finish_kernel    window off: a thread per pixel turns the bits into depth,
//                    inverse depth or 0.
//   filter_kernel    window on: a workgroup per TILE_H x TILE_W tile loads the
//                    tile and its halo into LDS, takes the minimum along rows,
//                    then along columns (exact in any order), and writes the
//                    tile.  Reads the unfiltered buffer only.
// 3 launches whatever the data.  No host synchronisation, no allocation, no
// state, plain vector stores and atomics only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int TILE_H = LSI_LIDAR_TILE_H;   // 16
constexpr int TILE_W = LSI_LIDAR_TILE_W;   // 64: a wave per tile row
constexpr int MAX_WIN = 8;
constexpr int RAW_H = TILE_H + 2 * MAX_WIN;
constexpr int RAW_W = TILE_W + 2 * MAX_WIN;
constexpr int ROWS_PER_PASS = TPB / TILE_W;       // 4
constexpr int PASSES = TILE_H / ROWS_PER_PASS;    // 4 pixels per thread
constexpr uint32_t EMPTY = 0xffffffffu;
constexpr int64_t MAX_PIXELS = 1ll << 27;
constexpr int64_t MAX_POINTS = 1ll << 27;

static_assert(TPB % TILE_W == 0 && TILE_H % ROWS_PER_PASS == 0, "tile shape");

// One point into one view's z-buffer (H x W words).
__device__ __forceinline__ void project(const float4 q, const float* m, int H, int W,
                                        float z_min, float z_max, uint32_t* zbuf) {
  const float X = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], q.x), __fmul_rn(m[1], q.y)),
                                      __fmul_rn(m[2], q.z)), m[3]);
  const float Y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4], q.x), __fmul_rn(m[5], q.y)),
                                      __fmul_rn(m[6], q.z)), m[7]);
  const float Z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[8], q.x), __fmul_rn(m[9], q.y)),
                                      __fmul_rn(m[10], q.z)), m[11]);
  if (!(Z >= z_min && Z <= z_max)) return;        // (a NaN fails both)
  const float u = __fdiv_rn(X, Z), v = __fdiv_rn(Y, Z);
  if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) return;
  // 0 <= u < W <= 2^27: the conversion truncates, which is floorf here
  const int col = (int)u, row = (int)v;
  __hip_atomic_fetch_min(zbuf + row * W + col, __float_as_uint(Z), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TPB) void scatter_kernel(const LsiScanDesc* __restrict__ desc,
                                                      const float4* __restrict__ pts,
                                                      const float* __restrict__ mats, int V,
                                                      int H, int W, float z_min, float z_max,
                                                      uint32_t* zbuf) {
  const int b = blockIdx.y;
  const LsiScanDesc d = desc[b];                  // uniform: scalar loads
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= d.n) return;
  const float* m = mats + (size_t)b * V * 12;
  float m0[12], m1[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) m0[k] = m[k];
#pragma unroll
  for (int k = 0; k < 12; ++k) m1[k] = V == 2 ? m[12 + k] : 0.0f;
  const float4 q = pts[d.first + i];
  uint32_t* z0 = zbuf + (size_t)b * V * H * W;
  project(q, m0, H, W, z_min, z_max, z0);
  if (V == 2) project(q, m1, H, W, z_min, z_max, z0 + H * W);
}

__device__ __forceinline__ float finish_value(uint32_t bits, bool keep, bool inverse) {
  if (!keep) return 0.0f;
  const float z = __uint_as_float(bits);
  return inverse ? __fdiv_rn(1.0f, z) : z;
}

__global__ __launch_bounds__(TPB) void finish_kernel(const uint32_t* __restrict__ zbuf, int n,
                                                     int inverse, float* __restrict__ out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t bits = zbuf[i];
  out[i] = finish_value(bits, bits != EMPTY, inverse != 0);
}

__global__ __launch_bounds__(TPB) void filter_kernel(const uint32_t* __restrict__ zbuf, int H,
                                                     int W, int tiles_y, int tiles_x, int win_y,
                                                     int win_x, float ratio, int inverse,
                                                     float* __restrict__ out) {
  __shared__ uint32_t raw[RAW_H * RAW_W];         // the tile and its halo
  __shared__ uint32_t hmin[RAW_H * TILE_W];       // minimum along the row window
  const int bid = blockIdx.x;
  const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y;
  const int img = bid / tiles_x / tiles_y;
  const int x0 = tile_x * TILE_W, y0 = tile_y * TILE_H;
  const int base = img * H * W;                   // (B V H W <= 2^27)
  const int rows = TILE_H + 2 * win_y, cols = TILE_W + 2 * win_x;

  for (int i = threadIdx.x; i < rows * cols; i += TPB) {
    const int r = i / cols, c = i % cols;
    const int gy = y0 - win_y + r, gx = x0 - win_x + c;
    const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
    raw[r * RAW_W + c] = inside ? zbuf[base + gy * W + gx] : EMPTY;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < rows * TILE_W; i += TPB) {
    const int r = i / TILE_W, c = i % TILE_W;
    uint32_t m = EMPTY;
    for (int k = 0; k <= 2 * win_x; ++k) m = min(m, raw[r * RAW_W + c + k]);
    hmin[i] = m;
  }
  __syncthreads();

  const int tx = threadIdx.x % TILE_W, ty = threadIdx.x / TILE_W;
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ry = ty + k * ROWS_PER_PASS;
    if (y0 + ry >= H || x0 + tx >= W) continue;
    uint32_t m = EMPTY;
    for (int j = 0; j <= 2 * win_y; ++j) m = min(m, hmin[(ry + j) * TILE_W + tx]);
    const uint32_t bits = raw[(ry + win_y) * RAW_W + tx + win_x];
    // a non-empty pixel is in its own window: m is a float's bits
    const bool keep = bits != EMPTY &&
                      !(__fmul_rn(__uint_as_float(m), ratio) < __uint_as_float(bits));
    out[base + (y0 + ry) * W + x0 + tx] = finish_value(bits, keep, inverse != 0);
  }
}

bool shape_ok(int32_t B, int32_t V, int32_t H, int32_t W, int32_t win_y, int32_t win_x) {
  if (B < 1 || B > 65535) return false;
  if (V != 1 && V != 2) return false;
  if (H < 1 || W < 1) return false;
  if ((int64_t)B * V * H > MAX_PIXELS || (int64_t)B * V * H * W > MAX_PIXELS) return false;
  return win_y >= 0 && win_y <= MAX_WIN && win_x >= 0 && win_x <= MAX_WIN;
}

}  // namespace

extern "C" {

size_t lsi_lidar_workspace_bytes(int32_t B, int32_t V, int32_t H, int32_t W, int32_t win_y,
                                 int32_t win_x) {
  if (!shape_ok(B, V, H, W, win_y, win_x)) return 0;
  return (size_t)B * V * H * W * sizeof(uint32_t);
}

int lsi_lidar_rasterize(int32_t B, int32_t V, int32_t H, int32_t W,
                        const LsiScanDesc* desc_host, const LsiScanDesc* desc_dev,
                        const float* pts, int64_t n_pts_total, const float* mats, float z_min,
                        float z_max, int32_t win_y, int32_t win_x, float occl_ratio,
                        uint32_t flags, float* out, void* workspace, size_t workspace_bytes,
                        lsi_stream_t stream) {
  if (!shape_ok(B, V, H, W, win_y, win_x)) return LSI_EINVAL;
  if (n_pts_total < 0 || n_pts_total > MAX_POINTS) return LSI_EINVAL;
  int32_t n_max = 0;
  if (desc_host) {
    for (int b = 0; b < B; ++b) {
      const LsiScanDesc& d = desc_host[b];
      if (d.n < 0 || d.first < 0 || d.first > n_pts_total - d.n || d.reserved != 0)
        return LSI_EINVAL;
      if (d.n > n_max) n_max = d.n;
    }
  }
  if (!isfinite(z_min) || !isfinite(z_max) || !(0.0f < z_min && z_min <= z_max))
    return LSI_EINVAL;
  const bool filtered = win_y > 0 || win_x > 0;
  if (filtered && !(occl_ratio >= 1.0f)) return LSI_EINVAL;
  if (flags & ~(uint32_t)LSI_LIDAR_INVERSE) return LSI_EINVAL;
  if (((uintptr_t)pts & 15) != 0) return LSI_EINVAL;
  if (!desc_host || !desc_dev || !mats || !out || !workspace) return LSI_ENULL;
  if (!pts && n_max > 0) return LSI_ENULL;
  const size_t need = lsi_lidar_workspace_bytes(B, V, H, W, win_y, win_x);
  if (workspace_bytes < need) return LSI_EWORKSPACE;

  hipStream_t s = (hipStream_t)stream;
  uint32_t* zbuf = (uint32_t*)workspace;
  const int n_pix = B * V * H * W;
  const int inverse = (flags & LSI_LIDAR_INVERSE) ? 1 : 0;
  if (hipMemsetAsync(zbuf, 0xff, need, s) != hipSuccess) return LSI_ELAUNCH;
  // (a call without points still launches one block per scan: the number of
  // launches does not depend on the data)
  const unsigned blocks = n_max > 0 ? (unsigned)((n_max + TPB - 1) / TPB) : 1u;
  hipLaunchKernelGGL(scatter_kernel, dim3(blocks, (unsigned)B), dim3(TPB), 0, s, desc_dev,
                     (const float4*)pts, mats, (int)V, (int)H, (int)W, z_min, z_max, zbuf);
  if (filtered) {
    const int tiles_y = (H + TILE_H - 1) / TILE_H, tiles_x = (W + TILE_W - 1) / TILE_W;
    // (at most 2^27 tiles)
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)(B * V * tiles_y * tiles_x)), dim3(TPB), 0,
                       s, (const uint32_t*)zbuf, (int)H, (int)W, tiles_y, tiles_x, (int)win_y,
                       (int)win_x, occl_ratio, inverse, out);
  } else {
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((n_pix + TPB - 1) / TPB)), dim3(TPB), 0, s,
                       (const uint32_t*)zbuf, n_pix, inverse, out);
  }
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
