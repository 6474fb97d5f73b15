// Fused SSIM view-synthesis loss and evaluation metric (gfx950).  There is no
// reference counterpart: the contract is DESIGN.md section 4.13.
//   t = AREA box mean of target at Ht x Wt (area_mean<3>, as view_synth_kernel)
//   windows: win x win patches wholly inside the border crop, separable weights
//   g (Gaussian or box) from the host; per window, layer and channel the five
//   weighted means mu_x, mu_y, E_xx, E_yy, E_xy and
//     S = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2))
//   d = (1 - (S_0 + S_1 + S_2) / 3) / 2, loss = mean over windows of min_l d.
// Forward: a workgroup takes 32 x 16 window positions, stages their pixel
// footprint in LDS (the target AREA-averaged once per tile), forms the moments
// by a row pass and a column pass through LDS and keeps the running min over
// the layers in registers.  Backward, gather form: a workgroup owns 32 x 8
// pixels, recomputes the moments of every window that covers them, finds each
// window's minimum and tie count, recomputes every layer's d with the same
// instruction sequence and compares it for equality (as view_synth_kernel
// recomputes layer_l1), and convolves the three coefficient maps back with the
// same weights: g = A + 2 x B + y C.  No global intermediate, no atomics.
// Bound: LDS traffic of the separable passes.  Reductions: per-thread fp32,
// per-block and final sums in fp64 in a fixed order (lsi_reduce.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"
#include "lsi_layers.h"
#include "lsi_reduce.h"

// a layer's d is compared bit for bit with its own recomputation
#pragma clang fp contract(off)

using namespace lsi;

namespace {

constexpr int MAXWIN = 11;       // largest window
constexpr int HALO = MAXWIN - 1;

// A tile of WX x WY window positions and its (WX + HALO) x (WY + HALO) pixel
// footprint, sized for the largest window.  The planes are addressed with the
// run-time pitches wx (windows) and fw = wx + win - 1 (pixels).
template <int WX_, int WY_>
struct Geo {
  static constexpr int WX = WX_, WY = WY_;
  static constexpr int FW = WX + HALO, FH = WY + HALO;
  static constexpr int NPIX = FW * FH;  // one channel of the footprint
  static constexpr int RS = FH * WX;    // one plane of row-pass moments
  static constexpr int WPT = (WX * WY + TPB - 1) / TPB;  // windows per thread
  static constexpr int LDS_FLOATS = 6 * NPIX + 5 * RS;
};
using FwdGeo = Geo<32, 16>;                  // 42.9 KB
constexpr int PX = 32, PY = 8;               // backward: pixels per tile
using BwdGeo = Geo<PX + HALO, PY + HALO>;    // 58.5 KB
static_assert(FwdGeo::LDS_FLOATS * 4 + 64 <= 65536, "LDS budget");
static_assert(BwdGeo::LDS_FLOATS * 4 + 64 <= 65536, "LDS budget");
// the backward keeps 3 coefficient planes and 3 planes of PY x wx column sums
// in the row-pass buffer
static_assert(BwdGeo::WX * BwdGeo::WY <= BwdGeo::RS, "coefficient planes");
static_assert(3 * PY * BwdGeo::WX <= 2 * BwdGeo::RS, "column-sum planes");

struct SArgs {
  int nl, B, Ht, Wt, H, W, x_min, y_min, win;
  int hc, wc, Hv, Wv;        // crop and window grid
  float c1, c2;
  float g[MAXWIN];           // separable weights
  const float* recons;       // [nl, B, Ht, Wt, 3] contiguous
  const float* target;       // [B, H, W, 3] element strides below
  long t_sb, t_sy, t_sx, t_sc;
};

// The AREA-resized target of the footprint whose first pixel is (cy0, cx0) in
// crop coordinates; 0 outside the crop (only windows that are not scored read
// those).  The same area_mean<3> call as view_synth_kernel's area_px.
__device__ __forceinline__ void stage_target(const SArgs& a, int b, int cy0, int cx0,
                                             int fh, int fw, int npix, float* st) {
  const int fy = a.H / a.Ht, fx = a.W / a.Wt;
  for (int i = threadIdx.x; i < fh * fw; i += TPB) {
    const int cy = cy0 + i / fw, cx = cx0 + i % fw;
    float t[3] = {0.f, 0.f, 0.f};
    if (cy >= 0 && cy < a.hc && cx >= 0 && cx < a.wc) {
      const int yt = cy + a.y_min, xt = cx + a.x_min;
      area_mean<3>(a.target + (long)b * a.t_sb + (long)(yt * fy) * a.t_sy +
                       (long)(xt * fx) * a.t_sx,
                   a.t_sy, a.t_sx, a.t_sc, fy, fx, t);
    }
    st[i] = t[0]; st[npix + i] = t[1]; st[2 * npix + i] = t[2];
  }
}

__device__ __forceinline__ void stage_layer(const SArgs& a, int l, int b, int cy0,
                                            int cx0, int fh, int fw, int npix,
                                            float* sx) {
  const float* img = a.recons + ((long)l * a.B + b) * a.Ht * a.Wt * 3;
  for (int i = threadIdx.x; i < fh * fw; i += TPB) {
    const int cy = cy0 + i / fw, cx = cx0 + i % fw;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    if (cy >= 0 && cy < a.hc && cx >= 0 && cx < a.wc) {
      const float* r = img + ((long)(cy + a.y_min) * a.Wt + (cx + a.x_min)) * 3;
      r0 = r[0]; r1 = r[1]; r2 = r[2];
    }
    sx[i] = r0; sx[npix + i] = r1; sx[2 * npix + i] = r2;
  }
}

// The five moments of the tile's wy x wx windows, three channels: per channel a
// row pass (fh x wx sums of win pixels along x) into sr, then a column pass.
// Thread t holds windows t, t + TPB, ... (flat index v * wx + u).  Lanes run
// along x in both passes, so the 4-byte LDS reads of a 32-lane group fall on
// consecutive banks.  Ends synchronised: sr is free, sx / st are still read by
// nobody.
template <typename G>
__device__ __forceinline__ void tile_moments(const SArgs& a, const float* sx,
                                             const float* st, float* sr, int wy, int wx,
                                             float (&mom)[G::WPT][3][5]) {
  const int n = a.win, fw = wx + n - 1, fh = wy + n - 1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int i = threadIdx.x; i < fh * wx; i += TPB) {
      const int r = i / wx, u = i % wx;
      const float* xp = sx + c * G::NPIX + r * fw + u;
      const float* yp = st + c * G::NPIX + r * fw + u;
      float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
      for (int k = 0; k < n; ++k) {
        const float x = xp[k], y = yp[k], w = a.g[k];
        mx += w * x; my += w * y;
        xx += w * (x * x); yy += w * (y * y); xy += w * (x * y);
      }
      sr[i] = mx; sr[G::RS + i] = my; sr[2 * G::RS + i] = xx;
      sr[3 * G::RS + i] = yy; sr[4 * G::RS + i] = xy;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G::WPT; ++j) {
      const int w = threadIdx.x + j * TPB;
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (w < wy * wx) {
        for (int k = 0; k < n; ++k) {
          const float gk = a.g[k];
          const float* p = sr + w + k * wx;
#pragma unroll
          for (int q = 0; q < 5; ++q) m[q] += gk * p[q * G::RS];
        }
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) mom[j][c][q] = m[q];
    }
    __syncthreads();
  }
}

// SSIM of one window and channel from its moments (mu_x, mu_y, E_xx, E_yy, E_xy)
struct SsimTerms { float a1, a2, b1, b2, s; };
__device__ __forceinline__ SsimTerms ssim_terms(const float (&m)[5], float c1,
                                                float c2) {
  SsimTerms t;
  const float mx = m[0], my = m[1];
  const float vx = m[2] - mx * mx, vy = m[3] - my * my, cxy = m[4] - mx * my;
  t.a1 = 2.0f * (mx * my) + c1;
  t.a2 = 2.0f * cxy + c2;
  t.b1 = (mx * mx + my * my) + c1;
  t.b2 = (vx + vy) + c2;
  t.s = div_rn(t.a1 * t.a2, t.b1 * t.b2);
  return t;
}

// mean over the three channels (sum, then / 3)
__device__ __forceinline__ float ssim_mean(const float (&m)[3][5], float c1, float c2) {
  const float s0 = ssim_terms(m[0], c1, c2).s, s1 = ssim_terms(m[1], c1, c2).s,
              s2 = ssim_terms(m[2], c1, c2).s;
  return ((s0 + s1) + s2) / 3.0f;
}

__device__ __forceinline__ float dssim(const float (&m)[3][5], float c1, float c2) {
  return (1.0f - ssim_mean(m, c1, c2)) / 2.0f;
}

// part[0]: sum over the windows of min_l d; part[1]: sum of layer 0's mean SSIM.
// metric != 0 reads layer 0 only.
__global__ __launch_bounds__(TPB) void ssim_fwd_kernel(SArgs a, int metric,
                                                       double* part) {
  using G = FwdGeo;
  __shared__ float lds[G::LDS_FLOATS];
  float* sx = lds;
  float* st = lds + 3 * G::NPIX;
  float* sr = lds + 6 * G::NPIX;
  const int n = a.win, fw = G::WX + n - 1, fh = G::WY + n - 1;
  const int tx_n = (a.Wv + G::WX - 1) / G::WX, ty_n = (a.Hv + G::WY - 1) / G::WY;
  const int tiles = a.B * ty_n * tx_n;
  const int nl = metric ? 1 : a.nl;
  float acc[2] = {0.0f, 0.0f};
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int txi = tile % tx_n, q = tile / tx_n;
    const int tyi = q % ty_n, b = q / ty_n;
    const int v0 = tyi * G::WY, u0 = txi * G::WX;
    stage_target(a, b, v0, u0, fh, fw, G::NPIX, st);
    float best[G::WPT];
    for (int l = 0; l < nl; ++l) {
      stage_layer(a, l, b, v0, u0, fh, fw, G::NPIX, sx);
      __syncthreads();
      float mom[G::WPT][3][5];
      tile_moments<G>(a, sx, st, sr, G::WY, G::WX, mom);
#pragma unroll
      for (int j = 0; j < G::WPT; ++j) {
        const int w = threadIdx.x + j * TPB;
        const bool scored = v0 + w / G::WX < a.Hv && u0 + w % G::WX < a.Wv;
        const float d = dssim(mom[j], a.c1, a.c2);
        best[j] = l == 0 ? d : fminf(best[j], d);
        if (l == 0 && scored) acc[1] += ssim_mean(mom[j], a.c1, a.c2);
      }
    }
#pragma unroll
    for (int j = 0; j < G::WPT; ++j) {
      const int w = threadIdx.x + j * TPB;
      if (v0 + w / G::WX < a.Hv && u0 + w % G::WX < a.Wv) acc[0] += best[j];
    }
    // (tile_moments ended synchronised: the next tile may overwrite sx and st)
  }
  block_store_partials<2>(acc, part);
}

// out_loss = scale * sum of part[0]; acc2 += (sum of part[1], count)
__global__ __launch_bounds__(TPB) void ssim_finish_kernel(const double* part, int nblk,
                                                          double scale, float* out_loss,
                                                          double* acc2, double count) {
  __shared__ double sm[TPB];
  const double s0 = block_total(part, nblk, sm);
  const double s1 = block_total(part + MAXBLK, nblk, sm);
  if (threadIdx.x != 0) return;
  if (out_loss) out_loss[0] = (float)(s0 * scale);
  if (acc2) { acc2[0] += s1; acc2[1] += count; }
}

// Gradient w.r.t. recons; every element is written, exact 0 outside the crop.
__global__ __launch_bounds__(TPB) void ssim_bwd_kernel(SArgs a, const float* g_loss,
                                                       float* g_recons) {
  using G = BwdGeo;
  __shared__ float lds[G::LDS_FLOATS];
  float* sx = lds;
  float* st = lds + 3 * G::NPIX;
  float* sr = lds + 6 * G::NPIX;
  const int n = a.win;
  const int wx = PX + n - 1, wy = PY + n - 1;  // windows that cover the tile
  const int fw = wx + n - 1, fh = wy + n - 1;
  const int tx_n = (a.Wt + PX - 1) / PX, ty_n = (a.Ht + PY - 1) / PY;
  const int tiles = a.B * ty_n * tx_n;
  const float gs = g_loss[0] / (float)((long)a.B * a.Hv * a.Wv);
  const long P = (long)a.B * a.Ht * a.Wt;
  const int px = threadIdx.x % PX, py = threadIdx.x / PX;  // this thread's pixel
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int txi = tile % tx_n, q = tile / tx_n;
    const int tyi = q % ty_n, b = q / ty_n;
    const int Y = tyi * PY + py, X = txi * PX + px;
    const bool in_img = Y < a.Ht && X < a.Wt;
    const bool in_crop = in_img && Y >= a.y_min && Y < a.Ht - a.y_min &&
                         X >= a.x_min && X < a.Wt - a.x_min;
    const long cell = ((long)b * a.Ht + Y) * a.Wt + X;
    // crop coordinates of the first window that reaches the tile
    const int v0 = tyi * PY - a.y_min - (n - 1), u0 = txi * PX - a.x_min - (n - 1);
    // a tile no window reaches (block-uniform): zeros
    if (v0 + wy <= 0 || v0 >= a.Hv || u0 + wx <= 0 || u0 >= a.Wv) {
      if (in_img)
        for (int l = 0; l < a.nl; ++l) {
          float* g = g_recons + ((long)l * P + cell) * 3;
          g[0] = 0.0f; g[1] = 0.0f; g[2] = 0.0f;
        }
      continue;
    }
    stage_target(a, b, v0, u0, fh, fw, G::NPIX, st);
    bool scored[G::WPT];
#pragma unroll
    for (int j = 0; j < G::WPT; ++j) {
      const int w = threadIdx.x + j * TPB;
      const int v = v0 + w / wx, u = u0 + w % wx;
      scored[j] = w < wy * wx && v >= 0 && v < a.Hv && u >= 0 && u < a.Wv;
    }
    // each window's minimum over the layers and the number of layers at it
    float best[G::WPT];
    int ties[G::WPT];
#pragma unroll
    for (int j = 0; j < G::WPT; ++j) { best[j] = 0.0f; ties[j] = 1; }
    if (a.nl > 1) {
      for (int l = 0; l < a.nl; ++l) {
        stage_layer(a, l, b, v0, u0, fh, fw, G::NPIX, sx);
        __syncthreads();
        float mom[G::WPT][3][5];
        tile_moments<G>(a, sx, st, sr, wy, wx, mom);
#pragma unroll
        for (int j = 0; j < G::WPT; ++j) {
          const float d = dssim(mom[j], a.c1, a.c2);
          if (l == 0 || d < best[j]) { best[j] = d; ties[j] = 1; }
          else if (d == best[j]) ties[j] += 1;
        }
      }
    }
    for (int l = 0; l < a.nl; ++l) {
      stage_layer(a, l, b, v0, u0, fh, fw, G::NPIX, sx);
      __syncthreads();
      float mom[G::WPT][3][5];
      tile_moments<G>(a, sx, st, sr, wy, wx, mom);
      // upstream weight of each window: d(loss)/d(S_c) = -1/6 of the window's
      // share, which goes to the layers whose d IS the minimum
      float up[G::WPT];
#pragma unroll
      for (int j = 0; j < G::WPT; ++j) {
        const bool hit = scored[j] &&
                         (a.nl == 1 || dssim(mom[j], a.c1, a.c2) == best[j]);
        up[j] = hit ? -(gs / (float)ties[j]) / 6.0f : 0.0f;
      }
      float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // coefficient maps: up * dS/d(mu_x), dS/d(E_xx), dS/d(E_xy)
#pragma unroll
        for (int j = 0; j < G::WPT; ++j) {
          const int w = threadIdx.x + j * TPB;
          if (w < wy * wx) {
            float ca = 0.f, cb = 0.f, cc = 0.f;
            if (up[j] != 0.0f) {
              const SsimTerms t = ssim_terms(mom[j][c], a.c1, a.c2);
              const float mx = mom[j][c][0], my = mom[j][c][1];
              const float rb = div_rn(1.0f, t.b1 * t.b2);
              const float s_b1 = div_rn(t.s, t.b1), s_b2 = div_rn(t.s, t.b2);
              ca = up[j] * (2.0f * my * (t.a2 - t.a1) * rb +
                            2.0f * mx * (s_b2 - s_b1));
              cb = up[j] * -s_b2;
              cc = up[j] * (2.0f * t.a1 * rb);
            }
            sr[w] = ca; sr[G::RS + w] = cb; sr[2 * G::RS + w] = cc;
          }
        }
        __syncthreads();
        // back through the column pass: pixel row r of the tile takes window
        // rows r .. r + n - 1 with weight g[r + n - 1 - row]
        float* cs = sr + 3 * G::RS;
        for (int i = threadIdx.x; i < 3 * PY * wx; i += TPB) {
          const int m = i / (PY * wx), rem = i % (PY * wx);
          const int r = rem / wx, u = rem % wx;
          const float* p = sr + m * G::RS + r * wx + u;
          float s = 0.0f;
          for (int k = 0; k < n; ++k) s += a.g[n - 1 - k] * p[k * wx];
          cs[i] = s;
        }
        __syncthreads();
        // ... and through the row pass, then g = A + 2 x B + y C
        {
          const float* p = cs + py * wx + px;
          float ga = 0.f, gb = 0.f, gc = 0.f;
          for (int k = 0; k < n; ++k) {
            const float gk = a.g[n - 1 - k];
            ga += gk * p[k]; gb += gk * p[PY * wx + k]; gc += gk * p[2 * PY * wx + k];
          }
          const int o = c * G::NPIX + (py + n - 1) * fw + (px + n - 1);
          g[c] = ga + 2.0f * sx[o] * gb + st[o] * gc;
        }
        // (the next channel's maps go to planes 0-2, which nobody reads now;
        // its column sums are written after its first barrier)
      }
      if (in_img) {
        float* go = g_recons + ((long)l * P + cell) * 3;
        go[0] = in_crop ? g[0] : 0.0f;
        go[1] = in_crop ? g[1] : 0.0f;
        go[2] = in_crop ? g[2] : 0.0f;
      }
      __syncthreads();  // sx is restaged, st by the next tile
    }
  }
}

// win weights in double, normalised, rounded to fp32; sigma <= 0: the box
bool window_weights(int win, float sigma, float* out) {
  if (win < 3 || win > MAXWIN || win % 2 == 0) return false;
  double w[MAXWIN], sum = 0.0;
  for (int i = 0; i < win; ++i) {
    const double x = (double)i - (double)(win - 1) / 2.0;
    w[i] = sigma > 0.0f ? exp(-(x * x) / (2.0 * (double)sigma * (double)sigma)) : 1.0;
    sum += w[i];
  }
  for (int i = 0; i < win; ++i) out[i] = (float)(w[i] / sum);
  return true;
}

int sargs_of(const LsiSsimDesc* d, const float* recons, const float* target,
             SArgs* a) {
  if (!d || d->nl <= 0 || d->B <= 0 || d->Ht <= 0 || d->Wt <= 0 || d->H <= 0 ||
      d->W <= 0 || d->H % d->Ht || d->W % d->Wt || d->x_min < 0 || d->y_min < 0)
    return LSI_EINVAL;
  for (int i = 0; i < MAXWIN; ++i) a->g[i] = 0.0f;
  if (!window_weights(d->win, d->sigma, a->g)) return LSI_EINVAL;
  a->nl = d->nl; a->B = d->B; a->Ht = d->Ht; a->Wt = d->Wt; a->H = d->H; a->W = d->W;
  a->x_min = d->x_min; a->y_min = d->y_min; a->win = d->win;
  a->hc = d->Ht - 2 * d->y_min; a->wc = d->Wt - 2 * d->x_min;
  a->Hv = a->hc - d->win + 1; a->Wv = a->wc - d->win + 1;
  if (a->Hv < 1 || a->Wv < 1) return LSI_EINVAL;
  // tiles and pixels are counted in int
  if ((int64_t)d->B * d->Ht * d->Wt >= ((int64_t)1 << 31)) return LSI_EINVAL;
  a->c1 = d->c1; a->c2 = d->c2;
  a->recons = recons; a->target = target;
  a->t_sb = d->t_sb; a->t_sy = d->t_sy; a->t_sx = d->t_sx; a->t_sc = d->t_sc;
  return LSI_OK;
}

int fwd_grid(const SArgs& a) {
  const long tiles = (long)a.B * ((a.Hv + FwdGeo::WY - 1) / FwdGeo::WY) *
                     ((a.Wv + FwdGeo::WX - 1) / FwdGeo::WX);
  return (int)(tiles < MAXBLK ? tiles : MAXBLK);
}

}  // namespace

extern "C" {

int lsi_ssim_window(int32_t win, float sigma, float* out) {
  if (win < 3 || win > MAXWIN || win % 2 == 0) return LSI_EINVAL;
  if (!out) return LSI_ENULL;
  window_weights(win, sigma, out);
  return LSI_OK;
}

int lsi_ssim_loss_fwd(const LsiSsimDesc* d, const float* recons, const float* target,
                      float* out_loss, void* ws, size_t ws_bytes,
                      lsi_stream_t stream) {
  SArgs a;
  const int rc = sargs_of(d, recons, target, &a);
  if (rc != LSI_OK) return rc;
  if (!recons || !target || !out_loss || !ws) return LSI_ENULL;
  if (ws_bytes < lsi_loss_workspace_bytes()) return LSI_EWORKSPACE;
  const int g = fwd_grid(a);
  hipLaunchKernelGGL(ssim_fwd_kernel, dim3(g), dim3(TPB), 0, (hipStream_t)stream, a,
                     0, (double*)ws);
  const double N = (double)a.B * a.Hv * a.Wv;
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream,
                     (const double*)ws, g, 1.0 / N, out_loss, (double*)nullptr, 0.0);
  return rc_of_launch();
}

int lsi_ssim_loss_bwd(const LsiSsimDesc* d, const float* recons, const float* target,
                      const float* g_loss, float* g_recons, lsi_stream_t stream) {
  SArgs a;
  const int rc = sargs_of(d, recons, target, &a);
  if (rc != LSI_OK) return rc;
  if (!recons || !target || !g_loss || !g_recons) return LSI_ENULL;
  const long tiles = (long)a.B * ((a.Ht + PY - 1) / PY) * ((a.Wt + PX - 1) / PX);
  const int g = (int)(tiles < MAXBLK ? tiles : MAXBLK);
  hipLaunchKernelGGL(ssim_bwd_kernel, dim3(g), dim3(TPB), 0, (hipStream_t)stream, a,
                     g_loss, g_recons);
  return rc_of_launch();
}

int lsi_eval_ssim(const LsiSsimDesc* d, const float* recons, const float* target,
                  double* acc2, void* ws, size_t ws_bytes, lsi_stream_t stream) {
  SArgs a;
  const int rc = sargs_of(d, recons, target, &a);
  if (rc != LSI_OK) return rc;
  if (!recons || !target || !acc2 || !ws) return LSI_ENULL;
  if (ws_bytes < lsi_loss_workspace_bytes()) return LSI_EWORKSPACE;
  const int g = fwd_grid(a);
  hipLaunchKernelGGL(ssim_fwd_kernel, dim3(g), dim3(TPB), 0, (hipStream_t)stream, a,
                     1, (double*)ws);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream,
                     (const double*)ws, g, 0.0, (float*)nullptr, acc2,
                     (double)a.B * a.Hv * a.Wv);
  return rc_of_launch();
}

}  // extern "C"
