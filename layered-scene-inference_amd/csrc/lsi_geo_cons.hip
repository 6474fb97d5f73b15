// Geometric-consistency loss between two views' inverse depths (gfx950):
// DESIGN.md section 4.21, the contract in include/lsi_hip.h.  The reference has
// no counterpart; the projection and the gather are lsi_disocclusion_mask's,
// from the same device primitives (lsi_common.h, lsi_layers.h).
//
//   forward   a block covers a fixed span of rows of ONE plane (the grid is
//             plane-aligned: BPP blocks per plane), a thread one pixel at a
//             time, the lanes of a wave consecutive x of a row.  A pixel's d is
//             projected by M[p], the partner plane r = (p + shift) mod P is
//             sampled where it lands; the sums of a plane -- sum e, N (scored
//             pixels), one spare -- are fp64 from the thread up, and the shared
//             one-block finish (lsi_reduce.h) writes the 3 P plane sums and the
//             loss, the mean of GeoTerm over the planes with a scored pixel.
//   backward  the same projection and taps again; a scored pixel adds its own
//             gradient (through dd and through the sample position) at its own
//             cell and g * de/ds * c_k at the partner's four taps, with fp32
//             global atomics into buffers the entry point zero-filled.  In the
//             paired form (E is D) both land in ONE buffer.
//
// Bound: the forward by the gather (4 taps per pixel, L2 hits for neighbouring
// lanes), the backward by the chip's fp32 atomic rate.  The forward has no
// atomics: the same inputs give the same bits.  The backward's sums depend on
// the order the adds arrive in, in their last bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_layers.h"
#include "lsi_reduce.h"

#pragma clang fp contract(off)

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

struct GArgs {
  LsiGeoConsDesc d;
  const float* D;
  const float* E;
  const float* M;
  int rows, bpp;  // rows per block, blocks per plane
  int e_flat;     // E's rows follow one another: offset = flat index * e_sx
};

// What the definition forms for one pixel.  Unscored: only `scored` is set.
struct Pix {
  bool scored;
  float q0, q1, q3, nden;  // pre-division terms (backward)
  float dd, s;
  float c[4];
  Taps t;
};

// Plane r of E at the flat tap index i = x + y*W.
struct EAt {
  const float* e;
  long sy, sx;
  int W, flat;
  __device__ __forceinline__ long off(int i) const {
    if (flat) return (long)i * sx;
    const int y = i / W;
    return (long)y * sy + (long)(i - y * W) * sx;
  }
  __device__ __forceinline__ float operator()(int i) const { return e[off(i)]; }
};

__device__ __forceinline__ EAt partner_of(const GArgs& a, int p) {
  const int r = (p + a.d.shift) % a.d.P;
  return EAt{a.E + (long)r * a.d.e_sp, (long)a.d.e_sy, (long)a.d.e_sx, a.d.W, a.e_flat};
}

__device__ __forceinline__ void score_px(const GArgs& a, const float* __restrict__ m,
                                         const EAt& at, float d, int x, int y, Pix& o) {
  const int H = a.d.H, W = a.d.W;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  o.scored = false;
  o.q0 = mrow(m, 0, px, py, d);
  o.q1 = mrow(m, 1, px, py, d);
  const float n = mrow(m, 2, px, py, d);
  o.q3 = mrow(m, 3, px, py, d);
  o.nden = safe_den(n);
  const float u = div_rn(o.q0, o.nden), v = div_rn(o.q1, o.nden);
  o.dd = div_rn(o.q3, o.nden);
  // (a NaN fails every comparison)
  if (!(finite_f(d) && finite_f(u) && finite_f(v) && finite_f(o.dd))) return;
  if (!(n > 0.0f && o.dd > 0.0f)) return;
  if (!(u >= 0.5f && u <= (float)W - 0.5f && v >= 0.5f && v <= (float)H - 0.5f)) return;
  taps_of(u, v, H, W, o.t);
  tap_weights(o.t, o.c);
  o.s = bilinear_gather_at(o.t, o.c, at);
  if (!(o.s > 0.0f)) return;
  if (a.d.occl_thresh > 0.0f && o.s - o.dd > a.d.occl_thresh * (o.s + o.dd)) return;
  o.scored = true;
}

template <int MODE>
__global__ __launch_bounds__(TPB) void geo_fwd_kernel(GArgs a, double* part,
                                                      float* __restrict__ out_map) {
  const int p = blockIdx.x / a.bpp, bx = blockIdx.x - p * a.bpp;
  const int W = a.d.W;
  const int y0 = bx * a.rows;
  const int ny = min(a.rows, a.d.H - y0);
  const float* m = a.M + 16 * (size_t)p;
  const EAt at = partner_of(a, p);
  const float* dp = a.D + (long)p * a.d.d_sp;
  double acc[3] = {0.0, 0.0, 0.0};  // sum e, N, spare
  for (int i = threadIdx.x; i < ny * W; i += TPB) {
    const int r = i / W, x = i - r * W, y = y0 + r;
    const float d = dp[(long)y * a.d.d_sy + (long)x * a.d.d_sx];
    Pix o;
    score_px(a, m, at, d, x, y, o);
    float ef = -1.0f;
    if (o.scored) {
      const double dd = (double)o.dd, s = (double)o.s;
      double e = fabs(dd - s);
      if (MODE == LSI_GEO_CONS_RATIO) e = e / (dd + s);
      acc[0] += e;
      acc[1] += 1.0;
      ef = (float)e;
    }
    if (out_map) out_map[((size_t)p * a.d.H + y) * W + x] = ef;
  }
  plane_store_partials(acc, part, a.d.P, p, a.bpp, bx);
}

// A plane's term of its sums (sum e, N, spare); a plane without a scored pixel
// does not enter the mean.
struct GeoTerm {
  __device__ bool counts(const double* s) const { return s[1] > 0.0; }
  __device__ double term(const double* s) const { return s[0] / s[1]; }
};

template <int MODE>
__global__ __launch_bounds__(TPB) void geo_bwd_kernel(GArgs a, const double* plane_sums,
                                                      const float* g_loss,
                                                      float* g_d, float* g_e) {
  const int p = blockIdx.x / a.bpp, bx = blockIdx.x - p * a.bpp;
  const int H = a.d.H, W = a.d.W;
  const int y0 = bx * a.rows;
  const int ny = min(a.rows, H - y0);
  const double n = plane_sums[3 * (size_t)p + 1];
  if (!(n > 0.0)) return;  // (uniform) nothing of this plane is scored
  // S (uniform: P is small) and the plane's constant g = g_loss / (S N_p)
  double S = 0.0;
  for (int i = 0; i < a.d.P; ++i) S += plane_sums[3 * (size_t)i + 1] > 0.0 ? 1.0 : 0.0;
  const float g = (float)((double)g_loss[0] / (S * n));
  const float* m = a.M + 16 * (size_t)p;
  const float m03 = m[3], m13 = m[7], m23 = m[11], m33 = m[15];
  const EAt at = partner_of(a, p);
  const float* dp = a.D + (long)p * a.d.d_sp;
  float* const own = g_d + (size_t)p * H * W;
  float* const taps = g_e + (size_t)((p + a.d.shift) % a.d.P) * H * W;
  for (int i = threadIdx.x; i < ny * W; i += TPB) {
    const int r = i / W, x = i - r * W, y = y0 + r;
    const float d = dp[(long)y * a.d.d_sy + (long)x * a.d.d_sx];
    Pix o;
    score_px(a, m, at, d, x, y, o);
    if (!o.scored) continue;
    const float sg = sgn(o.dd - o.s);
    if (sg == 0.0f) continue;  // sign(0) = 0: no gradient either way
    // de/ddd, de/ds
    float e_dd, e_s;
    if (MODE == LSI_GEO_CONS_RATIO) {
      const float b = o.dd + o.s, k = div_rn(2.0f * sg, b * b);
      e_dd = k * o.s;
      e_s = -(k * o.dd);
    } else {
      e_dd = sg;
      e_s = -sg;
    }
    // d(q_j / nden)/dd = (m_j3 nden - q_j m23) / nden^2
    const float rn2 = div_rn(1.0f, o.nden * o.nden);
    const float u_d = (m03 * o.nden - o.q0 * m23) * rn2;
    const float v_d = (m13 * o.nden - o.q1 * m23) * rn2;
    const float dd_d = (m33 * o.nden - o.q3 * m23) * rn2;
    // ds/du, ds/dv: the weights' derivatives are those of x1 - x and x - x0
    const Taps& t = o.t;
    const float e00 = at(t.i00), e01 = at(t.i01), e10 = at(t.i10), e11 = at(t.i11);
    const float s_u = t.vx1 * (t.vy0 * t.wy0 * e10 + t.vy1 * t.wy1 * e11) -
                      t.vx0 * (t.vy0 * t.wy0 * e00 + t.vy1 * t.wy1 * e01);
    const float s_v = t.vy1 * (t.vx0 * t.wx0 * e01 + t.vx1 * t.wx1 * e11) -
                      t.vy0 * (t.vx0 * t.wx0 * e00 + t.vx1 * t.wx1 * e10);
    const float gd = g * (e_dd * dd_d + e_s * (s_u * u_d + s_v * v_d));
    if (gd != 0.0f) atomic_add_f32(own + (size_t)y * W + x, gd);
    const float gs = g * e_s;
    const int idx[4] = {t.i00, t.i01, t.i10, t.i11};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float w = gs * o.c[k];
      if (w != 0.0f) atomic_add_f32(taps + idx[k], w);
    }
  }
}

bool desc_ok(const LsiGeoConsDesc* d) {
  if (!d) return false;
  if (d->mode != LSI_GEO_CONS_RATIO && d->mode != LSI_GEO_CONS_L1) return false;
  if (d->P <= 0 || d->H <= 0 || d->W <= 0 || d->P > 65535) return false;
  // tap indices are formed in fp32 (taps_of): exact below 2^24 pixels per plane
  if ((int64_t)d->H * d->W >= (1 << 24)) return false;
  if ((int64_t)d->P * d->H * d->W > (int64_t)INT32_MAX) return false;
  if (d->shift < 0 || d->shift >= d->P) return false;
  if (!(d->occl_thresh >= 0.0f && d->occl_thresh < 1.0f)) return false;
  return true;
}

GArgs args_of(const LsiGeoConsDesc* d, const float* D, const float* E, const float* M) {
  GArgs a;
  a.d = *d; a.D = D; a.E = E; a.M = M;
  a.rows = rows_per_block(d->H, d->W);
  a.bpp = blocks_per_plane(d->H, d->W);
  a.e_flat = d->e_sy == (int64_t)d->W * d->e_sx;
  return a;
}

}  // namespace

extern "C" {

size_t lsi_geo_cons_workspace_bytes(const LsiGeoConsDesc* d) {
  if (!desc_ok(d)) return 0;
  return plane_ws_doubles((size_t)d->P, blocks_per_plane(d->H, d->W)) * sizeof(double);
}

int lsi_geo_cons_loss_fwd(const LsiGeoConsDesc* d, const float* disp,
                          const float* partner, const float* M, float* out_loss,
                          double* plane_sums, float* out_map, void* ws,
                          size_t ws_bytes, lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!disp || !partner || !M || !out_loss || !plane_sums || !ws) return LSI_ENULL;
  if (ws_bytes < lsi_geo_cons_workspace_bytes(d)) return LSI_EWORKSPACE;
  const GArgs a = args_of(d, disp, partner, M);
  double* part = (double*)ws;
  const dim3 grid((unsigned)(d->P * a.bpp)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  if (d->mode == LSI_GEO_CONS_RATIO)
    hipLaunchKernelGGL((geo_fwd_kernel<LSI_GEO_CONS_RATIO>), grid, block, 0, s, a, part,
                       out_map);
  else
    hipLaunchKernelGGL((geo_fwd_kernel<LSI_GEO_CONS_L1>), grid, block, 0, s, a, part,
                       out_map);
  plane_finish(GeoTerm{}, d->P, a.bpp, ws, plane_sums, out_loss, s);
  return rc_of_launch();
}

int lsi_geo_cons_loss_bwd(const LsiGeoConsDesc* d, const float* disp,
                          const float* partner, const float* M,
                          const double* plane_sums, const float* g_loss,
                          float* g_disp, float* g_partner, lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!disp || !partner || !M || !plane_sums || !g_loss || !g_disp) return LSI_ENULL;
  const GArgs a = args_of(d, disp, partner, M);
  const dim3 grid((unsigned)(d->P * a.bpp)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)d->P * d->H * d->W * sizeof(float);
  if (hipMemsetAsync(g_disp, 0, bytes, s) != hipSuccess) return LSI_ELAUNCH;
  if (g_partner && g_partner != g_disp &&
      hipMemsetAsync(g_partner, 0, bytes, s) != hipSuccess)
    return LSI_ELAUNCH;
  float* const taps = g_partner ? g_partner : g_disp;
  if (d->mode == LSI_GEO_CONS_RATIO)
    hipLaunchKernelGGL((geo_bwd_kernel<LSI_GEO_CONS_RATIO>), grid, block, 0, s, a,
                       plane_sums, g_loss, g_disp, taps);
  else
    hipLaunchKernelGGL((geo_bwd_kernel<LSI_GEO_CONS_L1>), grid, block, 0, s, a,
                       plane_sums, g_loss, g_disp, taps);
  return rc_of_launch();
}

}  // extern "C"
