// Edge-aware disparity smoothness loss (gfx950): DESIGN.md section 4.14, the
// contract in include/lsi_hip.h.  The reference has no counterpart.
//
//   forward   one thread per pixel, a grid-stride pass over ONE plane per block
//             (the grid is plane-aligned: BPP blocks per plane), three sums per
//             plane -- A = sum |sx| wx, B = sum |sy| wy, S = sum d -- as fp32
//             per thread, fp64 per block; the shared one-block finish
//             (lsi_reduce.h) writes the 3 L B plane sums and the loss, the mean
//             of the planes' EdgeTerm.
//   backward  the same pass in gather form: a pixel collects sign(s) w of the
//             stencils that touch it (2 per axis at order 1, 3 at order 2),
//             recomputing the weights from the guide, and subtracts the plane's
//             normalisation term, which it derives from the plane sums.
//
// Bound: HBM streaming.  A pixel's stencil neighbours are loaded directly: lanes
// are consecutive pixels of a row, so a neighbour's address is in the lines the
// wave has just fetched (a hit in the vector L1); HBM sees one read of disp and
// guide.  The contiguous layout (disp x-stride 1, guide pixel stride 3, channel
// stride 1) is compiled with those strides as constants.
// No atomics: the same inputs give the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_reduce.h"

using namespace lsi;

namespace {

constexpr int PPT = 4;  // pixels per thread the grid is sized for

inline int blocks_per_plane(long n) {
  long g = (n + (long)TPB * PPT - 1) / ((long)TPB * PPT);
  if (g > MAXBPP) g = MAXBPP;
  if (g < 1) g = 1;
  return (int)g;
}

struct EArgs {
  LsiEdgeSmoothDesc d;
  const float* disp;
  const float* guide;
  int bpp;
  float ca;  // alpha / 3 (order 1), alpha / 6 (order 2): exp(-ca * sum_c |dG|)
};

// One plane's disparities and guide.  FAST: the contiguous layout.
template <bool FAST>
struct Plane {
  const float* __restrict__ d;
  const float* __restrict__ g;
  long dsy, dsx, gsy, gsx, gsc;
  __device__ __forceinline__ float D(int y, int x) const {
    return d[(long)y * dsy + (FAST ? (long)x : (long)x * dsx)];
  }
  // sum over the channels of |G[ya, xa, c] - G[yb, xb, c]|
  __device__ __forceinline__ float E(int ya, int xa, int yb, int xb) const {
    const float* pa = g + (long)ya * gsy + (FAST ? (long)xa * 3 : (long)xa * gsx);
    const float* pb = g + (long)yb * gsy + (FAST ? (long)xb * 3 : (long)xb * gsx);
    const long c = FAST ? 1 : gsc;
    return (fabsf(pa[0] - pb[0]) + fabsf(pa[c] - pb[c])) + fabsf(pa[2 * c] - pb[2 * c]);
  }
};

template <bool FAST>
__device__ __forceinline__ Plane<FAST> plane_of(const EArgs& a, int p) {
  const int l = p / a.d.B, b = p - l * a.d.B;
  Plane<FAST> v;
  v.d = a.disp + (long)l * a.d.d_sl + (long)b * a.d.d_sb;
  v.g = a.guide + (long)l * a.d.g_sl + (long)b * a.d.g_sb;
  v.dsy = a.d.d_sy; v.dsx = a.d.d_sx;
  v.gsy = a.d.g_sy; v.gsx = a.d.g_sx; v.gsc = a.d.g_sc;
  return v;
}

// |s| w of the stencil anchored at position `pos` of an axis of extent n.
// Dk(k): the disparity k steps along the axis; Ek(i, j): the channel sum of
// |G| differences between the pixels i and j steps along it.
template <int ORDER, class FD, class FE>
__device__ __forceinline__ float axis_term(int pos, int n, float ca, FD Dk, FE Ek) {
  if (ORDER == 1) {
    if (pos + 1 >= n) return 0.0f;
    return fabsf(Dk(0) - Dk(1)) * expf(-ca * Ek(0, 1));
  }
  if (pos < 1 || pos + 1 >= n) return 0.0f;
  return fabsf((Dk(-1) - 2.0f * Dk(0)) + Dk(1)) * expf(-ca * Ek(1, -1));
}

// sum over the stencils that touch position `pos` of coefficient * sign(s) * w
template <int ORDER, class FD, class FE>
__device__ __forceinline__ float axis_grad(int pos, int n, float ca, FD Dk, FE Ek) {
  float g = 0.0f;
  if (ORDER == 1) {
    // s[pos] = d[pos] - d[pos + 1]: +1; s[pos - 1] = d[pos - 1] - d[pos]: -1
    if (pos + 1 < n) g += sgn(Dk(0) - Dk(1)) * expf(-ca * Ek(0, 1));
    if (pos >= 1) g -= sgn(Dk(-1) - Dk(0)) * expf(-ca * Ek(-1, 0));
    return g;
  }
  // the stencil centred at c = pos + k (1 <= c <= n - 2) holds d[pos] with +1
  // (k = -1, +1) or -2 (k = 0)
#pragma unroll
  for (int k = -1; k <= 1; ++k) {
    const int c = pos + k;
    if (c < 1 || c + 1 >= n) continue;
    const float t = sgn((Dk(k - 1) - 2.0f * Dk(k)) + Dk(k + 1)) *
                    expf(-ca * Ek(k + 1, k - 1));
    g += (k == 0) ? -2.0f * t : t;
  }
  return g;
}

template <int ORDER, bool FAST>
__global__ __launch_bounds__(TPB) void edge_fwd_kernel(EArgs a, double* part) {
  const int p = blockIdx.x / a.bpp, bx = blockIdx.x - p * a.bpp;
  const Plane<FAST> v = plane_of<FAST>(a, p);
  const int H = a.d.H, W = a.d.W;
  const int N = H * W;
  float acc[3] = {0.f, 0.f, 0.f};  // A, B, S
  for (int i = bx * TPB + threadIdx.x; i < N; i += a.bpp * TPB) {
    const int y = i / W, x = i - y * W;
    acc[0] += axis_term<ORDER>(
        x, W, a.ca, [&](int k) { return v.D(y, x + k); },
        [&](int i0, int i1) { return v.E(y, x + i0, y, x + i1); });
    acc[1] += axis_term<ORDER>(
        y, H, a.ca, [&](int k) { return v.D(y + k, x); },
        [&](int i0, int i1) { return v.E(y + i0, x, y + i1, x); });
    acc[2] += v.D(y, x);
  }
  plane_store_partials(acc, part, a.d.L * a.d.B, p, a.bpp, bx);
}

// A plane's term k_p [A_p / (H (W - o)) + B_p / ((H - o) W)] of its sums A, B, S;
// every plane enters the mean.
struct EdgeTerm {
  double n, nx, ny, eps;
  int normalise;
  __device__ bool counts(const double*) const { return true; }
  __device__ double term(const double* s) const {
    const double kp = normalise ? 1.0 / (s[2] / n + eps) : 1.0;
    return kp * (s[0] / nx + s[1] / ny);
  }
};

template <int ORDER, bool FAST>
__global__ __launch_bounds__(TPB) void edge_bwd_kernel(EArgs a,
                                                       const double* plane_sums,
                                                       const float* g_loss,
                                                       float* __restrict__ g_disp) {
  const int p = blockIdx.x / a.bpp, bx = blockIdx.x - p * a.bpp;
  const Plane<FAST> v = plane_of<FAST>(a, p);
  const int H = a.d.H, W = a.d.W;
  const int N = H * W;
  // the plane's three constants: g = cx gx + cy gy - c0
  const double planes = (double)a.d.L * a.d.B;
  const double nx = (double)H * (W - ORDER), ny = (double)(H - ORDER) * W;
  const double A = plane_sums[3 * (size_t)p], Bs = plane_sums[3 * (size_t)p + 1];
  const double S = plane_sums[3 * (size_t)p + 2];
  const double gl = (double)g_loss[0];
  const double kp = a.d.normalise ? 1.0 / (S / (double)N + (double)a.d.eps) : 1.0;
  const float cx = (float)(gl * kp / (planes * nx));
  const float cy = (float)(gl * kp / (planes * ny));
  const float c0 = a.d.normalise
                       ? (float)(gl * kp * kp / ((double)N * planes) * (A / nx + Bs / ny))
                       : 0.0f;
  float* const out = g_disp + (size_t)p * N;
  for (int i = bx * TPB + threadIdx.x; i < N; i += a.bpp * TPB) {
    const int y = i / W, x = i - y * W;
    const float gx = axis_grad<ORDER>(
        x, W, a.ca, [&](int k) { return v.D(y, x + k); },
        [&](int i0, int i1) { return v.E(y, x + i0, y, x + i1); });
    const float gy = axis_grad<ORDER>(
        y, H, a.ca, [&](int k) { return v.D(y + k, x); },
        [&](int i0, int i1) { return v.E(y + i0, x, y + i1, x); });
    out[i] = (cx * gx + cy * gy) - c0;
  }
}

bool desc_ok(const LsiEdgeSmoothDesc* d) {
  if (!d || d->L <= 0 || d->B <= 0 || d->H <= 0 || d->W <= 0) return false;
  if (d->order != 1 && d->order != 2) return false;
  if (d->H < d->order + 1 || d->W < d->order + 1) return false;
  if (!(d->alpha >= 0.0f) || !isfinite(d->alpha)) return false;
  // a plane is indexed with 32-bit pixel numbers, the planes with 32-bit blocks
  if ((long)d->H * d->W > 0x7fffffffL - (long)MAXBPP * TPB) return false;
  if ((long)d->L * d->B > 0x7fffffffL / MAXBPP) return false;
  return true;
}

bool fast_layout(const LsiEdgeSmoothDesc* d) {
  return d->d_sx == 1 && d->g_sc == 1 && d->g_sx == 3;
}

EArgs args_of(const LsiEdgeSmoothDesc* d, const float* disp, const float* guide) {
  EArgs a;
  a.d = *d; a.disp = disp; a.guide = guide;
  a.bpp = blocks_per_plane((long)d->H * d->W);
  a.ca = (float)((double)d->alpha / (d->order == 1 ? 3.0 : 6.0));
  return a;
}

}  // namespace

extern "C" {

size_t lsi_edge_smooth_workspace_bytes(const LsiEdgeSmoothDesc* d) {
  if (!desc_ok(d)) return 0;
  return plane_ws_doubles((size_t)d->L * d->B, blocks_per_plane((long)d->H * d->W)) *
         sizeof(double);
}

int lsi_edge_smooth_loss_fwd(const LsiEdgeSmoothDesc* d, const float* disp,
                             const float* guide, float* out_loss,
                             double* plane_sums, void* ws, size_t ws_bytes,
                             lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!disp || !guide || !out_loss || !plane_sums || !ws) return LSI_ENULL;
  if (ws_bytes < lsi_edge_smooth_workspace_bytes(d)) return LSI_EWORKSPACE;
  const EArgs a = args_of(d, disp, guide);
  const int planes = d->L * d->B;
  double* part = (double*)ws;
  const dim3 grid((unsigned)(planes * a.bpp)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  const bool fast = fast_layout(d);
  if (d->order == 1) {
    if (fast) hipLaunchKernelGGL((edge_fwd_kernel<1, true>), grid, block, 0, s, a, part);
    else hipLaunchKernelGGL((edge_fwd_kernel<1, false>), grid, block, 0, s, a, part);
  } else {
    if (fast) hipLaunchKernelGGL((edge_fwd_kernel<2, true>), grid, block, 0, s, a, part);
    else hipLaunchKernelGGL((edge_fwd_kernel<2, false>), grid, block, 0, s, a, part);
  }
  const EdgeTerm f = {(double)d->H * d->W, (double)d->H * (d->W - d->order),
                      (double)(d->H - d->order) * d->W, (double)d->eps, d->normalise};
  plane_finish(f, planes, a.bpp, ws, plane_sums, out_loss, s);
  return rc_of_launch();
}

int lsi_edge_smooth_loss_bwd(const LsiEdgeSmoothDesc* d, const float* disp,
                             const float* guide, const double* plane_sums,
                             const float* g_loss, float* g_disp,
                             lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!disp || !guide || !plane_sums || !g_loss || !g_disp) return LSI_ENULL;
  const EArgs a = args_of(d, disp, guide);
  const dim3 grid((unsigned)(d->L * d->B * a.bpp)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  const bool fast = fast_layout(d);
  if (d->order == 1) {
    if (fast)
      hipLaunchKernelGGL((edge_bwd_kernel<1, true>), grid, block, 0, s, a, plane_sums,
                         g_loss, g_disp);
    else
      hipLaunchKernelGGL((edge_bwd_kernel<1, false>), grid, block, 0, s, a, plane_sums,
                         g_loss, g_disp);
  } else {
    if (fast)
      hipLaunchKernelGGL((edge_bwd_kernel<2, true>), grid, block, 0, s, a, plane_sums,
                         g_loss, g_disp);
    else
      hipLaunchKernelGGL((edge_bwd_kernel<2, false>), grid, block, 0, s, a, plane_sums,
                         g_loss, g_disp);
  }
  return rc_of_launch();
}

}  // extern "C"
