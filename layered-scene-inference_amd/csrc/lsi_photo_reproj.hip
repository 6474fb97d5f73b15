// Backward-warp photometric loss over the layers of an LDI (gfx950): DESIGN.md
// section 4.23, the contract in include/lsi_hip.h.  The reference has no
// counterpart; the projection is lsi_geo_cons.hip's score_px, the gather
// lsi_bilinear_fwd's, from the same device primitives (lsi_common.h,
// lsi_layers.h), the sums lsi_reduce.h's per-plane form.
//
//   forward   a block covers a fixed span of whole rows of ONE plane (the grid
//             is plane-aligned: BPP blocks per plane), a thread one pixel at a
//             time, the lanes of a wave consecutive x of a row.  A pixel's d is
//             projected by M[q], q = p mod Q; the image r = (q + shift) mod Q is
//             sampled where it lands, channel by channel, and compared with the
//             pixel's own texture.  The sums of a plane -- sum e, N (scored
//             pixels), one spare -- are fp64 from the thread up; the shared
//             one-block finish writes the 3 P plane sums and the loss.
//   backward  the same projection, taps and rule again; every thread writes the
//             gradient of its own texture cell and its own disparity cell, 0
//             where the pixel is not scored.  The sampled image is data: nothing
//             is scattered, there is no atomic and no zero-fill, and the same
//             inputs give the same bits.
//
// The texture (and its gradient) of the 256 pixels of a block's step is 256 C
// consecutive floats where tex's last two strides are (C, 1): those move as
// whole lines through LDS (thread t moves floats t, t + 256, ...), not as C
// strided accesses per lane.  Any other stride reads and writes per lane; the
// values are the same, so both routes give the same bits.
//
// Bound: bytes.  Per pixel of tex the forward reads 4 C (texture) + 4
// (disparity) bytes and the backward reads the same and writes 4 C + 4; the
// sampled image and the partner are read once per call, (4 C + 4) Q / P bytes
// per pixel, when the 4 (C + 1) taps of a pixel are cache hits -- neighbouring
// lanes land on neighbouring cells.  C = 3, P = 2 Q: forward 24, backward 40
// bytes per pixel.
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

struct PArgs {
  LsiPhotoReprojDesc d;
  const float* tex;
  const float* disp;
  const float* img;
  const float* M;
  const float* partner;  // NULL, or read only with occl_thresh > 0
  int rows, bpp;         // rows per block, blocks per plane
  int lines;             // tex's last two strides are (C, 1): whole lines via LDS
  int i_flat, e_flat;    // rows follow one another: offset = flat index * sx
};

// One channel of an image plane at the flat tap index i = x + y*W.
struct PlaneAt {
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

// What the definition forms for one pixel.  Unscored: only `scored` is set.
template <int C>
struct Pix {
  bool scored;
  float q0, q1, nden;  // pre-division terms (backward)
  float s[C];          // the samples
  float c[4];
  Taps t;
};

template <int C>
__device__ __forceinline__ void score_px(const PArgs& a, const float* __restrict__ m,
                                         const PlaneAt& im, const PlaneAt& pa, float d,
                                         const float (&tx)[C], int x, int y, Pix<C>& o) {
  const int H = a.d.H, W = a.d.W;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  o.scored = false;
  o.q0 = mrow(m, 0, px, py, d);
  o.q1 = mrow(m, 1, px, py, d);
  const float n = mrow(m, 2, px, py, d);
  const float q3 = mrow(m, 3, px, py, d);
  o.nden = safe_den(n);
  const float u = div_rn(o.q0, o.nden), v = div_rn(o.q1, o.nden);
  const float dd = div_rn(q3, o.nden);
  // (a NaN fails every comparison)
  if (!(finite_f(d) && finite_f(u) && finite_f(v) && finite_f(dd))) return;
  if (!(n > 0.0f && dd > 0.0f)) return;
  if (!(u >= 0.5f && u <= (float)W - 0.5f && v >= 0.5f && v <= (float)H - 0.5f)) return;
  taps_of(u, v, H, W, o.t);
  tap_weights(o.t, o.c);
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    PlaneAt ch = im;
    ch.e += (long)c * a.d.i_sc;
    o.s[c] = bilinear_gather_at(o.t, o.c, ch);
    fin = fin && finite_f(tx[c]) && finite_f(o.s[c]);
  }
  if (!fin) return;
  if (a.d.occl_thresh > 0.0f) {
    const float sd = bilinear_gather_at(o.t, o.c, pa);
    if (!(sd > 0.0f)) return;
    if (sd - dd > a.d.occl_thresh * (sd + dd)) return;
  }
  o.scored = true;
}

// The C texture values of pixel i0 + threadIdx.x of the block's span (npix
// pixels from row y0 of the plane tp), by every thread of the block.
template <int C>
__device__ __forceinline__ void load_tex(const PArgs& a, const float* __restrict__ tp,
                                         int y0, int i0, int npix, float* stage,
                                         float (&tx)[C]) {
  const int W = a.d.W, i = i0 + (int)threadIdx.x;
  if (a.lines) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const int j = k * TPB + (int)threadIdx.x, pj = j / C, pix = i0 + pj;
      if (pix < npix) {
        const int r = pix / W, x = pix - r * W;
        stage[j] = tp[(long)(y0 + r) * a.d.t_sy + (long)x * C + (j - pj * C)];
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) tx[c] = i < npix ? stage[threadIdx.x * C + c] : 0.0f;
    __syncthreads();
  } else {
    const int r = i < npix ? i / W : 0, x = i < npix ? i - r * W : 0;
    const float* q = tp + (long)(y0 + r) * a.d.t_sy + (long)x * a.d.t_sx;
#pragma unroll
    for (int c = 0; c < C; ++c) tx[c] = i < npix ? q[(long)c * a.d.t_sc] : 0.0f;
  }
}

// The reverse for the gradient: gp is the first float of the span's first pixel
// in the contiguous [P,H,W,C] gradient.
template <int C>
__device__ __forceinline__ void store_grad(const PArgs& a, float* __restrict__ gp, int i0,
                                           int npix, float* stage, const float (&gt)[C]) {
  const int i = i0 + (int)threadIdx.x;
  if (a.lines) {
#pragma unroll
    for (int c = 0; c < C; ++c) stage[threadIdx.x * C + c] = gt[c];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const int j = k * TPB + (int)threadIdx.x;
      if (i0 + j / C < npix) gp[(size_t)i0 * C + j] = stage[j];
    }
    __syncthreads();
  } else if (i < npix) {
#pragma unroll
    for (int c = 0; c < C; ++c) gp[(size_t)i * C + c] = gt[c];
  }
}

struct Span {
  int p, bx, y0, npix;
  const float* m;
  PlaneAt im, pa;
  const float* tp;
  const float* dp;
};

__device__ __forceinline__ Span span_of(const PArgs& a) {
  Span s;
  s.p = blockIdx.x / a.bpp;
  s.bx = blockIdx.x - s.p * a.bpp;
  s.y0 = s.bx * a.rows;
  s.npix = min(a.rows, a.d.H - s.y0) * a.d.W;
  const int q = s.p % a.d.Q, r = (q + a.d.shift) % a.d.Q;
  s.m = a.M + 16 * (size_t)q;
  s.im = PlaneAt{a.img + (long)r * a.d.i_sq, (long)a.d.i_sy, (long)a.d.i_sx, a.d.W, a.i_flat};
  s.pa = PlaneAt{a.partner ? a.partner + (long)r * a.d.e_sq : nullptr, (long)a.d.e_sy,
                 (long)a.d.e_sx, a.d.W, a.e_flat};
  const int l = s.p / a.d.Q;
  s.tp = a.tex + (long)l * a.d.t_sl + (long)q * a.d.t_sq;
  s.dp = a.disp + (long)l * a.d.d_sl + (long)q * a.d.d_sq;
  return s;
}

template <int C, int MODE>
__global__ __launch_bounds__(TPB) void photo_fwd_kernel(PArgs a, double* part,
                                                        float* __restrict__ out_map) {
  __shared__ float stage[TPB * C];
  const Span sp = span_of(a);
  const int W = a.d.W;
  const double eps = (double)a.d.eps;
  double acc[3] = {0.0, 0.0, 0.0};  // sum e, N, spare
  // (every thread takes every step: load_tex holds barriers)
  for (int i0 = 0; i0 < sp.npix; i0 += TPB) {
    const int i = i0 + (int)threadIdx.x;
    float tx[C];
    load_tex<C>(a, sp.tp, sp.y0, i0, sp.npix, stage, tx);
    if (i >= sp.npix) continue;
    const int r = i / W, x = i - r * W, y = sp.y0 + r;
    const float d = sp.dp[(long)y * a.d.d_sy + (long)x * a.d.d_sx];
    Pix<C> o;
    score_px<C>(a, sp.m, sp.im, sp.pa, d, tx, x, y, o);
    float ef = -1.0f;
    if (o.scored) {
      double e = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double df = (double)tx[c] - (double)o.s[c];
        e += MODE == LSI_PHOTO_CHARB ? sqrt(df * df + eps * eps) : fabs(df);
      }
      e = e / (double)C;
      acc[0] += e;
      acc[1] += 1.0;
      ef = (float)e;
    }
    if (out_map) out_map[((size_t)sp.p * a.d.H + y) * W + x] = ef;
  }
  plane_store_partials(acc, part, a.d.P, sp.p, a.bpp, sp.bx);
}

// A plane's term of its sums (sum e, N, spare); a plane without a scored pixel
// does not enter the mean.
struct PhotoTerm {
  __device__ bool counts(const double* s) const { return s[1] > 0.0; }
  __device__ double term(const double* s) const { return s[0] / s[1]; }
};

template <int C, int MODE>
__global__ __launch_bounds__(TPB) void photo_bwd_kernel(PArgs a, const double* plane_sums,
                                                        const float* g_loss,
                                                        float* __restrict__ g_tex,
                                                        float* __restrict__ g_disp) {
  __shared__ float stage[TPB * C];
  const Span sp = span_of(a);
  const int H = a.d.H, W = a.d.W;
  const double n = plane_sums[3 * (size_t)sp.p + 1];
  const bool any = n > 0.0;  // (uniform) else nothing of this plane is scored
  float gc = 0.0f;
  if (any) {
    // S (uniform: P is small) and the plane's constant g / C = g_loss / (S N_p C)
    double S = 0.0;
    for (int i = 0; i < a.d.P; ++i) S += plane_sums[3 * (size_t)i + 1] > 0.0 ? 1.0 : 0.0;
    gc = div_rn((float)((double)g_loss[0] / (S * n)), (float)C);
  }
  const float m03 = sp.m[3], m13 = sp.m[7], m23 = sp.m[11];
  const float eps = a.d.eps;
  const size_t first = ((size_t)sp.p * H + sp.y0) * W;  // the span's first pixel
  for (int i0 = 0; i0 < sp.npix; i0 += TPB) {
    const int i = i0 + (int)threadIdx.x;
    const bool in = i < sp.npix;
    float tx[C], gt[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gt[c] = 0.0f;
    float gd = 0.0f;
    if (any) {  // (uniform)
      load_tex<C>(a, sp.tp, sp.y0, i0, sp.npix, stage, tx);
      if (in) {
        const int r = i / W, x = i - r * W, y = sp.y0 + r;
        const float d = sp.dp[(long)y * a.d.d_sy + (long)x * a.d.d_sx];
        Pix<C> o;
        score_px<C>(a, sp.m, sp.im, sp.pa, d, tx, x, y, o);
        if (o.scored) {
          // d(q_j / nden)/dd = (m_j3 nden - q_j m23) / nden^2
          const float rn2 = div_rn(1.0f, o.nden * o.nden);
          const float u_d = (m03 * o.nden - o.q0 * m23) * rn2;
          const float v_d = (m13 * o.nden - o.q1 * m23) * rn2;
          const Taps& t = o.t;
          float su = 0.0f, sv = 0.0f;  // sum_c psi'_c ds_c/du, ... ds_c/dv
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float df = tx[c] - o.s[c];
            float ps;  // psi'(tex - s)
            if (MODE == LSI_PHOTO_CHARB)
              ps = div_rn(df, __fsqrt_rn(df * df + eps * eps));
            else
              ps = sgn(df);
            gt[c] = gc * ps;
            // ds/du, ds/dv: the weights' derivatives are those of x1 - x and x - x0
            PlaneAt at = sp.im;
            at.e += (long)c * a.d.i_sc;
            const float e00 = at(t.i00), e01 = at(t.i01), e10 = at(t.i10), e11 = at(t.i11);
            const float s_u = t.vx1 * (t.vy0 * t.wy0 * e10 + t.vy1 * t.wy1 * e11) -
                              t.vx0 * (t.vy0 * t.wy0 * e00 + t.vy1 * t.wy1 * e01);
            const float s_v = t.vy1 * (t.vx0 * t.wx0 * e01 + t.vx1 * t.wx1 * e11) -
                              t.vy0 * (t.vx0 * t.wx0 * e00 + t.vx1 * t.wx1 * e10);
            su = su + ps * s_u;
            sv = sv + ps * s_v;
          }
          gd = -(gc * (su * u_d + sv * v_d));
        }
      }
    }
    if (g_disp && in) g_disp[first + i] = gd;
    if (g_tex) store_grad<C>(a, g_tex + first * C, i0, sp.npix, stage, gt);
  }
}

bool desc_ok(const LsiPhotoReprojDesc* d) {
  if (!d) return false;
  if (d->mode != LSI_PHOTO_L1 && d->mode != LSI_PHOTO_CHARB) return false;
  if (d->P <= 0 || d->Q <= 0 || d->H <= 0 || d->W <= 0 || d->P > 65535) return false;
  if (d->C < 1 || d->C > 4) return false;
  if (d->P % d->Q) return false;
  // tap indices are formed in fp32 (taps_of): exact below 2^24 pixels per plane
  if ((int64_t)d->H * d->W >= (1 << 24)) return false;
  if ((int64_t)d->P * d->H * d->W > (int64_t)INT32_MAX) return false;
  if (d->shift < 0 || d->shift >= d->Q) return false;
  if (!(d->occl_thresh >= 0.0f && d->occl_thresh < 1.0f)) return false;
  if (!(d->eps > 0.0f && d->eps < __builtin_inff())) return false;
  return true;
}

PArgs args_of(const LsiPhotoReprojDesc* d, const float* tex, const float* disp,
              const float* img, const float* M, const float* partner) {
  PArgs a;
  a.d = *d; a.tex = tex; a.disp = disp; a.img = img; a.M = M; a.partner = partner;
  a.rows = rows_per_block(d->H, d->W);
  a.bpp = blocks_per_plane(d->H, d->W);
  a.lines = d->t_sx == d->C && d->t_sc == 1;
  a.i_flat = d->i_sy == (int64_t)d->W * d->i_sx;
  a.e_flat = d->e_sy == (int64_t)d->W * d->e_sx;
  return a;
}

template <int C, class... A>
void launch_fwd(int mode, dim3 grid, hipStream_t s, A... args) {
  if (mode == LSI_PHOTO_CHARB)
    hipLaunchKernelGGL((photo_fwd_kernel<C, LSI_PHOTO_CHARB>), grid, dim3(TPB), 0, s, args...);
  else
    hipLaunchKernelGGL((photo_fwd_kernel<C, LSI_PHOTO_L1>), grid, dim3(TPB), 0, s, args...);
}

template <int C, class... A>
void launch_bwd(int mode, dim3 grid, hipStream_t s, A... args) {
  if (mode == LSI_PHOTO_CHARB)
    hipLaunchKernelGGL((photo_bwd_kernel<C, LSI_PHOTO_CHARB>), grid, dim3(TPB), 0, s, args...);
  else
    hipLaunchKernelGGL((photo_bwd_kernel<C, LSI_PHOTO_L1>), grid, dim3(TPB), 0, s, args...);
}

}  // namespace

extern "C" {

size_t lsi_photo_reproj_workspace_bytes(const LsiPhotoReprojDesc* d) {
  if (!desc_ok(d)) return 0;
  return plane_ws_doubles((size_t)d->P, blocks_per_plane(d->H, d->W)) * sizeof(double);
}

int lsi_photo_reproj_loss_fwd(const LsiPhotoReprojDesc* d, const float* tex,
                              const float* disp, const float* img, const float* M,
                              const float* partner, float* out_loss, double* plane_sums,
                              float* out_map, void* ws, size_t ws_bytes,
                              lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!tex || !disp || !img || !M || !out_loss || !plane_sums || !ws) return LSI_ENULL;
  if (!partner && d->occl_thresh > 0.0f) return LSI_ENULL;
  if (ws_bytes < lsi_photo_reproj_workspace_bytes(d)) return LSI_EWORKSPACE;
  const PArgs a = args_of(d, tex, disp, img, M, partner);
  double* part = (double*)ws;
  const dim3 grid((unsigned)(d->P * a.bpp));
  hipStream_t s = (hipStream_t)stream;
  switch (d->C) {
    case 1: launch_fwd<1>(d->mode, grid, s, a, part, out_map); break;
    case 2: launch_fwd<2>(d->mode, grid, s, a, part, out_map); break;
    case 3: launch_fwd<3>(d->mode, grid, s, a, part, out_map); break;
    default: launch_fwd<4>(d->mode, grid, s, a, part, out_map); break;
  }
  plane_finish(PhotoTerm{}, d->P, a.bpp, ws, plane_sums, out_loss, s);
  return rc_of_launch();
}

int lsi_photo_reproj_loss_bwd(const LsiPhotoReprojDesc* d, const float* tex,
                              const float* disp, const float* img, const float* M,
                              const float* partner, const double* plane_sums,
                              const float* g_loss, float* g_tex, float* g_disp,
                              lsi_stream_t stream) {
  if (!desc_ok(d)) return LSI_EINVAL;
  if (!tex || !disp || !img || !M || !plane_sums || !g_loss || (!g_tex && !g_disp))
    return LSI_ENULL;
  if (!partner && d->occl_thresh > 0.0f) return LSI_ENULL;
  const PArgs a = args_of(d, tex, disp, img, M, partner);
  const dim3 grid((unsigned)(d->P * a.bpp));
  hipStream_t s = (hipStream_t)stream;
  switch (d->C) {
    case 1: launch_bwd<1>(d->mode, grid, s, a, plane_sums, g_loss, g_tex, g_disp); break;
    case 2: launch_bwd<2>(d->mode, grid, s, a, plane_sums, g_loss, g_tex, g_disp); break;
    case 3: launch_bwd<3>(d->mode, grid, s, a, plane_sums, g_loss, g_tex, g_disp); break;
    default: launch_bwd<4>(d->mode, grid, s, a, plane_sums, g_loss, g_tex, g_disp); break;
  }
  return rc_of_launch();
}

}  // extern "C"
