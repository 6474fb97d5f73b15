// Sparse depth-supervision loss (gfx950): DESIGN.md section 4.20, the contract
// in include/lsi_hip.h.  The reference has no counterpart.
//
//   forward   a block covers a fixed span of rows of ONE plane (the grid is
//             plane-aligned: BPP blocks per plane), a thread four neighbouring
//             pixels of a row at a time; three sums per plane -- n (scored
//             pixels), A, Q -- in fp64 from the thread up; the shared one-block
//             finish (lsi_reduce.h) writes the 3 P plane sums and the loss,
//             the mean of DsupTerm over the planes with a scored pixel.
//   backward  the same pass; validity and d_i are recomputed from the inputs,
//             the plane's constants and S from the plane sums.
//
// Bound: HBM streaming, and at LiDAR density mostly of the ground truth: gt is
// read first, and the load of pred is issued only for a group of four pixels
// that holds a scored one.  Rows whose base is 16-byte aligned at x-stride 1 are
// read with 16-byte loads; the ragged row end and any other stride go pixel by
// pixel.  No atomics: the same inputs give the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_reduce.h"

using namespace lsi;

namespace {

constexpr int SPAN = 1024;  // pixels of a block's span, at least (whole rows)

inline int rows_per_block(int H, int W) {
  const int a = (SPAN + W - 1) / W, b = (H + MAXBPP - 1) / MAXBPP;
  return a > b ? a : b;
}

inline int blocks_per_plane(int H, int W) {
  const int r = rows_per_block(H, W);
  return (H + r - 1) / r;
}

struct DArgs {
  LsiDepthSupDesc d;
  const float* pred;
  const float* gt;
  const float* scale;  // gt_scale or NULL
  int rows, bpp;       // rows per block, blocks per plane
  int vec_p, vec_g;    // 16-byte loads of pred / gt rows
  int vec_o;           // 16-byte stores of g_pred rows (backward)
};

// The four pixels x .. x + 3 of row `y` of plane `p` (n of them inside the row):
// the ground truth g[] as inverse depth, which are scored, and -- only if one is
// -- the clamped predictions q[] and whether each was above eps.
struct Quad {
  float g[4], q[4];
  bool ok[4], live[4];
  bool any;
};

__device__ __forceinline__ Quad load_quad(const DArgs& a, int p, int y, int x, int n,
                                          float sc) {
  Quad v;
  const float* grow = a.gt + (long)p * a.d.g_sp + (long)y * a.d.g_sy;
  float raw[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.vec_g && n == 4) {
    const float4 t = *reinterpret_cast<const float4*>(grow + x);
    raw[0] = t.x; raw[1] = t.y; raw[2] = t.z; raw[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) raw[k] = grow[(long)(x + k) * a.d.g_sx];
  }
  v.any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v.g[k] = raw[k] * sc;
    // (a NaN fails every comparison)
    v.ok[k] = k < n && raw[k] > a.d.valid_above && v.g[k] >= a.d.g_min &&
              v.g[k] <= a.d.g_max;
    v.any = v.any || v.ok[k];
    v.q[k] = a.d.eps;
    v.live[k] = false;
  }
  if (!v.any) return v;
  const float* prow = a.pred + (long)p * a.d.p_sp + (long)y * a.d.p_sy;
  float pr[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.vec_p && n == 4) {
    const float4 t = *reinterpret_cast<const float4*>(prow + x);
    pr[0] = t.x; pr[1] = t.y; pr[2] = t.z; pr[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v.ok[k]) pr[k] = prow[(long)(x + k) * a.d.p_sx];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v.q[k] = fmaxf(pr[k], a.d.eps);  // NaN -> eps
    v.live[k] = v.ok[k] && pr[k] > a.d.eps;
  }
  return v;
}

template <int MODE>
__global__ __launch_bounds__(TPB) void dsup_fwd_kernel(DArgs a, double* part) {
  const int p = blockIdx.x / a.bpp, bx = blockIdx.x - p * a.bpp;
  const int W = a.d.W, WQ = (W + 3) >> 2;
  const int y0 = bx * a.rows;
  const int ny = min(a.rows, a.d.H - y0);
  const float sc = a.scale ? a.scale[p] : 1.0f;
  double acc[3] = {0.0, 0.0, 0.0};  // n, A, Q
  for (int i = threadIdx.x; i < ny * WQ; i += TPB) {
    const int r = i / WQ, x = (i - r * WQ) * 4;
    const Quad v = load_quad(a, p, y0 + r, x, min(4, W - x), sc);
    if (!v.any) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!v.ok[k]) continue;
      acc[0] += 1.0;
      if (MODE == LSI_DEPTH_SUP_SILOG) {
        const double d = (double)(logf(v.q[k]) - logf(v.g[k]));
        acc[1] += d;
        acc[2] += d * d;
      } else {
        acc[1] += (double)fabsf(v.q[k] - v.g[k]);
      }
    }
  }
  plane_store_partials(acc, part, a.d.P, p, a.bpp, bx);
}

// A plane's term D_p of its sums n, A, Q; a plane without a scored pixel does
// not enter the mean.
struct DsupTerm {
  int mode;
  double lam;
  __device__ bool counts(const double* s) const { return s[0] > 0.0; }
  __device__ double term(const double* s) const {
    const double m = s[1] / s[0];
    return mode == LSI_DEPTH_SUP_SILOG ? s[2] / s[0] - lam * m * m : m;
  }
};

template <int MODE>
__global__ __launch_bounds__(TPB) void dsup_bwd_kernel(DArgs a, const double* plane_sums,
                                                       const float* g_loss,
                                                       float* __restrict__ g_pred) {
  const int p = blockIdx.x / a.bpp, bx = blockIdx.x - p * a.bpp;
  const int W = a.d.W, WQ = (W + 3) >> 2;
  const int y0 = bx * a.rows;
  const int ny = min(a.rows, a.d.H - y0);
  const float sc = a.scale ? a.scale[p] : 1.0f;
  // S and the plane's constants (uniform: P is small)
  double S = 0.0;
  for (int i = 0; i < a.d.P; ++i) S += plane_sums[3 * (size_t)i] > 0.0 ? 1.0 : 0.0;
  const double n = plane_sums[3 * (size_t)p], A = plane_sums[3 * (size_t)p + 1];
  const double gl = (double)g_loss[0];
  // SILOG: g = (c1 d - c0) / q; L1: g = c1 sign(e)
  double c1 = 0.0, c0 = 0.0;
  if (n > 0.0) {
    if (MODE == LSI_DEPTH_SUP_SILOG) {
      c1 = gl * 2.0 / (S * n);
      c0 = gl * 2.0 * (double)a.d.lam * A / (S * n * n);
    } else {
      c1 = gl / (n * S);
    }
  }
  const float c1f = (float)c1;
  float* const out = g_pred + (size_t)p * a.d.H * W;
  for (int i = threadIdx.x; i < ny * WQ; i += TPB) {
    const int r = i / WQ, x = (i - r * WQ) * 4;
    const int nx = min(4, W - x);
    const Quad v = load_quad(a, p, y0 + r, x, nx, sc);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (v.any) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!v.live[k]) continue;
        if (MODE == LSI_DEPTH_SUP_SILOG) {
          const double d = (double)(logf(v.q[k]) - logf(v.g[k]));
          g[k] = (float)((c1 * d - c0) / (double)v.q[k]);
        } else {
          g[k] = c1f * sgn(v.q[k] - v.g[k]);
        }
      }
    }
    float* o = out + (size_t)(y0 + r) * W + x;
    if (a.vec_o && nx == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nx) o[k] = g[k];
    }
  }
}

bool desc_ok(const LsiDepthSupDesc* d) {
  if (!d) return false;
  if (d->mode != LSI_DEPTH_SUP_SILOG && d->mode != LSI_DEPTH_SUP_L1) return false;
  if (d->P <= 0 || d->H <= 0 || d->W <= 0) return false;
  if (!isfinite(d->valid_above) || !isfinite(d->g_min) || !isfinite(d->g_max) ||
      !isfinite(d->eps) || !isfinite(d->lam))
    return false;
  if (d->g_min <= 0.0f || d->g_max < d->g_min || d->valid_above < 0.0f) return false;
  if (d->eps <= 0.0f || d->lam < 0.0f || d->lam > 1.0f) return false;
  // a block's span is indexed with 32-bit numbers, the planes with 32-bit blocks
  if ((long)d->H * d->W > 0x7fffffffL - 4L * TPB) return false;
  if ((long)d->P > 0x7fffffffL / MAXBPP) return false;
  return true;
}

bool rows_aligned(const void* base, int64_t s_plane, int64_t s_y, int64_t s_x) {
  return s_x == 1 && s_plane % 4 == 0 && s_y % 4 == 0 && (uintptr_t)base % 16 == 0;
}

DArgs args_of(const LsiDepthSupDesc* d, const float* pred, const float* gt,
              const float* scale, const float* g_pred) {
  DArgs a;
  a.d = *d; a.pred = pred; a.gt = gt; a.scale = scale;
  a.rows = rows_per_block(d->H, d->W);
  a.bpp = blocks_per_plane(d->H, d->W);
  a.vec_p = rows_aligned(pred, d->p_sp, d->p_sy, d->p_sx);
  a.vec_g = rows_aligned(gt, d->g_sp, d->g_sy, d->g_sx);
  a.vec_o = g_pred && d->W % 4 == 0 && (uintptr_t)g_pred % 16 == 0;
  return a;
}

}  // namespace

extern "C" {

size_t lsi_depth_sup_workspace_bytes(const LsiDepthSupDesc* d) {
  if (!desc_ok(d)) return 0;
  return plane_ws_doubles((size_t)d->P, blocks_per_plane(d->H, d->W)) * sizeof(double);
}

int lsi_depth_sup_loss_fwd(const LsiDepthSupDesc* d, const float* pred,
                           const float* gt, const float* gt_scale, float* out_loss,
                           double* plane_sums, void* ws, size_t ws_bytes,
                           lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!pred || !gt || !out_loss || !plane_sums || !ws) return LSI_ENULL;
  if (ws_bytes < lsi_depth_sup_workspace_bytes(d)) return LSI_EWORKSPACE;
  const DArgs a = args_of(d, pred, gt, gt_scale, nullptr);
  double* part = (double*)ws;
  const dim3 grid((unsigned)(d->P * a.bpp)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  if (d->mode == LSI_DEPTH_SUP_SILOG)
    hipLaunchKernelGGL((dsup_fwd_kernel<LSI_DEPTH_SUP_SILOG>), grid, block, 0, s, a, part);
  else
    hipLaunchKernelGGL((dsup_fwd_kernel<LSI_DEPTH_SUP_L1>), grid, block, 0, s, a, part);
  const DsupTerm f = {d->mode, (double)d->lam};
  plane_finish(f, d->P, a.bpp, ws, plane_sums, out_loss, s);
  return rc_of_launch();
}

int lsi_depth_sup_loss_bwd(const LsiDepthSupDesc* d, const float* pred,
                           const float* gt, const float* gt_scale,
                           const double* plane_sums, const float* g_loss,
                           float* g_pred, lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!pred || !gt || !plane_sums || !g_loss || !g_pred) return LSI_ENULL;
  const DArgs a = args_of(d, pred, gt, gt_scale, g_pred);
  const dim3 grid((unsigned)(d->P * a.bpp)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  if (d->mode == LSI_DEPTH_SUP_SILOG)
    hipLaunchKernelGGL((dsup_bwd_kernel<LSI_DEPTH_SUP_SILOG>), grid, block, 0, s, a,
                       plane_sums, g_loss, g_pred);
  else
    hipLaunchKernelGGL((dsup_bwd_kernel<LSI_DEPTH_SUP_L1>), grid, block, 0, s, a,
                       plane_sums, g_loss, g_pred);
  return rc_of_launch();
}

}  // extern "C"
