// Fused renderer of planar scenes on MI355X (gfx950): lsi_render_planes.
//
// One launch renders B worlds x V views.  Per view pixel and plane, in
// registers: homography (helpers.transform_pts), divide_safe, the four
// bilinear taps of the RGBA texel (sampling.py:41-168), the analytic plane
// disparity (homography.trg_disp_maps); then over the P + 1 layers the soft
// z-buffer, layers.compose (hard or soft) and layers.compose_depth
// (bg_layer=False) -- optionally a second time with the masks of the object
// planes [n_box, P) taken as 0 (the room alone).  The warped P x H x W x 5
// layers of the op route never exist in memory.
//
// The arithmetic is the op route's, operation for operation: taps_of and
// layer_logp_of are the code lsi_sampling.hip / lsi_loss.hip compile
// (lsi_layers.h); the max / sum / div_rn(expf, sum) / first-maximum sequence is
// compose_kernel's.
//
// Mapping: one thread per view pixel, pixels numbered along rows, so a wave
// covers a run of 64 pixels of one row (W % 64 == 0) and its taps fall on
// neighbouring 16-byte texels.  The 12 floats of a plane are addressed by
// blockIdx and the (unrolled) plane index only: wave-uniform loads through the
// constant cache, no per-lane traffic.  Workgroups are renumbered so that the
// blocks of one world (all its views) run on one XCD -- workgroup i runs on XCD
// i % 8, every XCD takes a contiguous run of (world, view, block) ids -- and a
// texel is brought into one L2 instead of eight.  No atomics, no LDS, no
// workspace.
//
// lsi_render_planes_bwd is TF autodiff of that op graph on
// the same mapping: pass 1 is the forward's per-pixel code (plane_px_of,
// compose_px -- one copy, so the winning layer is the forward's bit for bit),
// pass 2 walks the planes again, recomputes their taps and sends the texture
// gradient out with float atomics; the 12 sums per (world, view, plane) of the
// homography / disparity-matrix gradients are reduced in the wave, then in the
// workgroup, written as one partial per workgroup into the caller's workspace
// and added in a fixed order by a second kernel (run-to-run reproducible).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"
#include "lsi_layers.h"

#pragma clang fp contract(off)

using namespace lsi;

namespace {

constexpr int TPB = 256;

struct SArgs {
  int P, Hs, Ws, H, W, n_box, soft;
  int nblk;            // workgroups per view
  unsigned outputs;
  float min_disp, temp;
  const float4* tex;   // [B, P, Hs, Ws] RGBA
  const float* hom;    // [B, V, P, 9]
  const float* dmat;   // [B, V, P, 3]
  float* img; float* disp; float* img_room; float* disp_room;
  int V;
};

// One composition of the pixel's P + 1 layers (compose_kernel's sequence,
// csrc/lsi_loss.hip): lp[] the planes' log-probabilities, lp_bg the background
// layer's.  Every index is a compile-time constant after unrolling, the winner
// is carried by selects: nothing is addressed by a lane's own index.  o_mx and
// o_sum are the softmax's shift and normaliser, o_win the selected layer (P:
// the background) -- what the backward needs to form the same probabilities.
template <int PB>
__device__ __forceinline__ void compose_px(int P, const float (&lp)[PB], float lp_bg,
                                           const float (&d)[PB],
                                           const float (&col)[PB][3], int soft,
                                           float min_disp, float (&o_img)[3],
                                           float& o_disp, float& o_mx, float& o_sum,
                                           int& o_win) {
  float mx = lp[0];
#pragma unroll
  for (int l = 1; l < PB; ++l)
    if (l < P) mx = fmaxf(mx, lp[l]);
  mx = fmaxf(mx, lp_bg);
  float sum = 0.0f;
#pragma unroll
  for (int l = 0; l < PB; ++l)
    if (l < P) sum += expf(lp[l] - mx);
  sum += expf(lp_bg - mx);
  float pbest = div_rn(expf(lp[0] - mx), sum);
  int win = 0;
  float bd = d[0], b0 = col[0][0], b1 = col[0][1], b2 = col[0][2];
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  if (soft) { s0 += pbest * col[0][0]; s1 += pbest * col[0][1]; s2 += pbest * col[0][2]; }
#pragma unroll
  for (int l = 1; l < PB; ++l) {
    if (l < P) {
      const float pl = div_rn(expf(lp[l] - mx), sum);
      if (pl > pbest) {
        pbest = pl; bd = d[l]; b0 = col[l][0]; b1 = col[l][1]; b2 = col[l][2];
        win = l;
      }
      if (soft) { s0 += pl * col[l][0]; s1 += pl * col[l][1]; s2 += pl * col[l][2]; }
    }
  }
  {
    const float pl = div_rn(expf(lp_bg - mx), sum);
    if (pl > pbest) { pbest = pl; bd = min_disp; b0 = b1 = b2 = 1.0f; win = P; }
    if (soft) { s0 += pl * 1.0f; s1 += pl * 1.0f; s2 += pl * 1.0f; }
  }
  o_img[0] = soft ? s0 : b0; o_img[1] = soft ? s1 : b1; o_img[2] = soft ? s2 : b2;
  o_disp = bd; o_mx = mx; o_sum = sum; o_win = win;
}

// XCD-aware numbering (as lsi_splat_stream2.hip): workgroup `lin` runs on XCD
// lin % 8 and takes the (lin / 8)-th id of that XCD's contiguous run
__device__ __forceinline__ unsigned xcd_wg_id() {
  const unsigned nwg = gridDim.x, lin = blockIdx.x;
  const unsigned xcd = lin & 7u, q = nwg >> 3, r8 = nwg & 7u;
  const unsigned base = xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q;
  return base + (lin >> 3);
}

// One plane seen from one view pixel (x, y): the warped coordinate, its taps
// and texels, the sampled colour / mask and the plane's disparity.
struct PlanePx {
  float den, u, v;             // safe_den(q2), q0 / den, q1 / den
  Taps t;
  float c00, c01, c10, c11;    // masked tap weights
  float4 t00, t01, t10, t11;   // texels (00: x0,y0  01: x0,y1  10: x1,y0)
  float col[3], m;             // sampled RGB and mask (0 when !t.ok)
  float dd;                    // dmat (x, y, 1), before the relu
};

__device__ __forceinline__ void plane_px_of(const float* __restrict__ h,
                                            const float* __restrict__ dm,
                                            const float4* __restrict__ tp, float x,
                                            float y, int Hs, int Ws, PlanePx& o) {
  // helpers.transform_pts (seq_matmul): ((x h0) + (y h1)) + 1 h2
  const float q0 = (x * h[0] + y * h[1]) + h[2];
  const float q1 = (x * h[3] + y * h[4]) + h[5];
  const float q2 = (x * h[6] + y * h[7]) + h[8];
  o.den = safe_den(q2);                           // homography.normalize_homogeneous
  o.u = div_rn(q0, o.den); o.v = div_rn(q1, o.den);
  taps_of(o.u, o.v, Hs, Ws, o.t);
  const Taps& t = o.t;
  o.c00 = t.vx0 * t.vy0 * t.wx0 * t.wy0;
  o.c01 = t.vx0 * t.vy1 * t.wx0 * t.wy1;
  o.c10 = t.vx1 * t.vy0 * t.wx1 * t.wy0;
  o.c11 = t.vx1 * t.vy1 * t.wx1 * t.wy1;
  // (indices are clamped into the texture by taps_of, 0 when !t.ok)
  o.t00 = tp[t.i00]; o.t01 = tp[t.i01]; o.t10 = tp[t.i10]; o.t11 = tp[t.i11];
  o.col[0] = o.col[1] = o.col[2] = 0.0f; o.m = 0.0f;
  if (t.ok) {   // a non-finite coordinate samples 0 (bilinear_fwd_kernel)
    o.col[0] = ((o.c00 * o.t00.x + o.c01 * o.t01.x) + o.c10 * o.t10.x) + o.c11 * o.t11.x;
    o.col[1] = ((o.c00 * o.t00.y + o.c01 * o.t01.y) + o.c10 * o.t10.y) + o.c11 * o.t11.y;
    o.col[2] = ((o.c00 * o.t00.z + o.c01 * o.t01.z) + o.c10 * o.t10.z) + o.c11 * o.t11.z;
    o.m = ((o.c00 * o.t00.w + o.c01 * o.t01.w) + o.c10 * o.t10.w) + o.c11 * o.t11.w;
  }
  // homography.trg_disp_maps: ((D0 x) + (D1 y)) + D2 1
  o.dd = (dm[0] * x + dm[1] * y) + dm[2];
}

template <int PB, bool ROOM>
__global__ __launch_bounds__(TPB) void render_planes_kernel(SArgs a) {
  const unsigned id = xcd_wg_id();
  const int bv = (int)(id / (unsigned)a.nblk);        // b * V + v
  const int blk = (int)(id - (unsigned)bv * (unsigned)a.nblk);
  const int b = bv / a.V;
  const int pix = blk * TPB + (int)threadIdx.x;
  if (pix >= a.H * a.W) return;
  const int iy = pix / a.W, ix = pix - iy * a.W;
  const float x = (float)ix + 0.5f, y = (float)iy + 0.5f;   // helpers.pixel_coords

  const int P = a.P;
  const float* __restrict__ hom = a.hom + (size_t)bv * P * 9;
  const float* __restrict__ dmat = a.dmat + (size_t)bv * P * 3;
  const size_t plane_px = (size_t)a.Hs * a.Ws;
  const float4* __restrict__ tex = a.tex + (size_t)b * P * plane_px;

  float lp[PB], lpr[PB], d[PB], col[PB][3];  // (lpr: dead without ROOM)
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    lp[p] = 0.0f; d[p] = 0.0f; col[p][0] = col[p][1] = col[p][2] = 0.0f;
    lpr[p] = 0.0f;
    if (p < P) {
      PlanePx px;
      plane_px_of(hom + p * 9, dmat + p * 3, tex + (size_t)p * plane_px, x, y, a.Hs,
                  a.Ws, px);
      col[p][0] = px.col[0]; col[p][1] = px.col[1]; col[p][2] = px.col[2];
      d[p] = fmaxf(px.dd, 0.0f);                      // relu (compose_kernel)
      const float m = px.m;
      lp[p] = layer_logp_of(m, d[p], a.temp);
      if (ROOM)  // the room alone: an object plane's mask is 0 everywhere
        lpr[p] = p < a.n_box ? lp[p] : layer_logp_of(0.0f, d[p], a.temp);
    }
  }
  const float lp_bg = layer_logp_of(1.0f, a.min_disp, a.temp);
  const size_t o = (size_t)bv * a.H * a.W + pix;
  float oi[3], od, mx, sum;
  int win;
  compose_px<PB>(P, lp, lp_bg, d, col, a.soft, a.min_disp, oi, od, mx, sum, win);
  if (a.outputs & LSI_SCENE_IMG) {
    a.img[3 * o] = oi[0]; a.img[3 * o + 1] = oi[1]; a.img[3 * o + 2] = oi[2];
  }
  if (a.outputs & LSI_SCENE_DISP) a.disp[o] = od;
  if constexpr (ROOM) {
    compose_px<PB>(P, lpr, lp_bg, d, col, a.soft, a.min_disp, oi, od, mx, sum, win);
    if (a.outputs & LSI_SCENE_IMG_ROOM) {
      a.img_room[3 * o] = oi[0]; a.img_room[3 * o + 1] = oi[1];
      a.img_room[3 * o + 2] = oi[2];
    }
    if (a.outputs & LSI_SCENE_DISP_ROOM) a.disp_room[o] = od;
  }
}

template <int PB>
void launch_pb(const SArgs& a, bool room, unsigned grid, hipStream_t st) {
  if (room)
    hipLaunchKernelGGL((render_planes_kernel<PB, true>), dim3(grid), dim3(TPB), 0, st, a);
  else
    hipLaunchKernelGGL((render_planes_kernel<PB, false>), dim3(grid), dim3(TPB), 0, st, a);
}

// ---------------------------------------------------------------------------
// lsi_render_planes_bwd
// ---------------------------------------------------------------------------
constexpr int NW = TPB / 64;   // waves per workgroup
constexpr int NSUM = 12;       // sums per (world, view, plane): g_hom 9 + g_dmat 3

struct BArgs {
  int P, Hs, Ws, H, W, V, soft;
  int nblk;             // workgroups per view
  float min_disp, temp;
  const float4* tex;    // [B, P, Hs, Ws] RGBA
  const float* hom;     // [B, V, P, 9]
  const float* dmat;    // [B, V, P, 3]
  const float* g_img;   // [B, V, H, W, 3] or NULL
  const float* g_disp;  // [B, V, H, W] or NULL
  float* g_tex;         // [B, P, Hs, Ws, 4] or NULL (accumulated into)
  float* part;          // [B * V * P, nblk, NSUM] partial sums (RED)
};

// RED: the homography / disparity-matrix gradients are wanted (every thread of
// the workgroup then stays to the end: the block-wide sums need all of them).
template <int PB, bool RED>
__global__ __launch_bounds__(TPB) void render_planes_bwd_kernel(BArgs a) {
  __shared__ float red[RED ? PB * NW * NSUM : 1];
  const unsigned id = xcd_wg_id();
  const int bv = (int)(id / (unsigned)a.nblk);        // b * V + v
  const int blk = (int)(id - (unsigned)bv * (unsigned)a.nblk);
  const int b = bv / a.V;
  const int npix = a.H * a.W;
  const bool valid = blk * TPB + (int)threadIdx.x < npix;
  if (!RED && !valid) return;
  // (a lane past the view's end works on the last pixel with zero gradients)
  const int pix = valid ? blk * TPB + (int)threadIdx.x : npix - 1;
  const int iy = pix / a.W, ix = pix - iy * a.W;
  const float x = (float)ix + 0.5f, y = (float)iy + 0.5f;   // helpers.pixel_coords

  const int P = a.P;
  const float* __restrict__ hom = a.hom + (size_t)bv * P * 9;
  const float* __restrict__ dmat = a.dmat + (size_t)bv * P * 3;
  const size_t plane_px = (size_t)a.Hs * a.Ws;
  const float4* __restrict__ tex = a.tex + (size_t)b * P * plane_px;

  // pass 1: the forward
  float lp[PB], d[PB], col[PB][3];
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    lp[p] = 0.0f; d[p] = 0.0f; col[p][0] = col[p][1] = col[p][2] = 0.0f;
    if (p < P) {
      PlanePx px;
      plane_px_of(hom + p * 9, dmat + p * 3, tex + (size_t)p * plane_px, x, y, a.Hs,
                  a.Ws, px);
      col[p][0] = px.col[0]; col[p][1] = px.col[1]; col[p][2] = px.col[2];
      d[p] = fmaxf(px.dd, 0.0f);
      lp[p] = layer_logp_of(px.m, d[p], a.temp);
    }
  }
  const float lp_bg = layer_logp_of(1.0f, a.min_disp, a.temp);
  float oi[3], od, mx, sum;
  int win;
  compose_px<PB>(P, lp, lp_bg, d, col, a.soft, a.min_disp, oi, od, mx, sum, win);

  const size_t o = (size_t)bv * npix + pix;
  float g[3] = {0.0f, 0.0f, 0.0f}, gd = 0.0f;
  if (valid && a.g_img) { g[0] = a.g_img[3 * o]; g[1] = a.g_img[3 * o + 1]; g[2] = a.g_img[3 * o + 2]; }
  if (valid && a.g_disp) gd = a.g_disp[o];
  const float sgo = (g[0] * oi[0] + g[1] * oi[1]) + g[2] * oi[2];

  // pass 2: the planes again, taps recomputed
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    if (p < P) {
      PlanePx px;
      plane_px_of(hom + p * 9, dmat + p * 3, tex + (size_t)p * plane_px, x, y, a.Hs,
                  a.Ws, px);
      // gradients of the layer's colour, mask and (pre-relu) disparity
      float gc[3] = {0.0f, 0.0f, 0.0f}, gm = 0.0f, gdd = 0.0f;
      if (a.soft) {
        const float pl = div_rn(expf(lp[p] - mx), sum);
        gc[0] = pl * g[0]; gc[1] = pl * g[1]; gc[2] = pl * g[2];
        const float gz =
            pl * (((g[0] * col[p][0] + g[1] * col[p][1]) + g[2] * col[p][2]) - sgo);
        gm = div_rn(gz, px.m + 1e-8f);
        // d z / d d = 1 / (temp d^2) for d > 0 (relu'(0) = 0, the indicator of
        // divide_safe has no gradient); p_l -> 0 faster than d^2: 0 at gz == 0
        if (d[p] > 0.0f && gz != 0.0f) gdd = div_rn(gz, a.temp * (d[p] * d[p]));
      } else if (p == win) {
        gc[0] = g[0]; gc[1] = g[1]; gc[2] = g[2];
      }
      if (p == win && d[p] > 0.0f) gdd += gd;          // compose_depth's selection
      if (!valid) { gc[0] = gc[1] = gc[2] = gm = gdd = 0.0f; }
      const Taps& t = px.t;
      if (a.g_tex && t.ok) {
        float* gt = a.g_tex + ((size_t)b * P + p) * plane_px * 4;
        const float cw[4] = {px.c00, px.c01, px.c10, px.c11};
        const int ci[4] = {t.i00, t.i01, t.i10, t.i11};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float* q = gt + (size_t)ci[k] * 4;
          const float u0 = cw[k] * gc[0], u1 = cw[k] * gc[1], u2 = cw[k] * gc[2],
                      u3 = cw[k] * gm;
          if (u0 != 0.0f) atomic_add_f32(q, u0);
          if (u1 != 0.0f) atomic_add_f32(q + 1, u1);
          if (u2 != 0.0f) atomic_add_f32(q + 2, u2);
          if (u3 != 0.0f) atomic_add_f32(q + 3, u3);
        }
      }
      if constexpr (RED) {
        float gq0 = 0.0f, gq1 = 0.0f, gq2 = 0.0f;
        if (t.ok) {
          // bilinear_bwd_kernel: d wx0 / dx = -1, d wx1 / dx = +1 (floor, clip and
          // equal carry no gradient)
          const float m00 = t.vx0 * t.vy0, m01 = t.vx0 * t.vy1, m10 = t.vx1 * t.vy0,
                      m11 = t.vx1 * t.vy1;
          const float gch[4] = {gc[0], gc[1], gc[2], gm};
          const float a00[4] = {px.t00.x, px.t00.y, px.t00.z, px.t00.w};
          const float a01[4] = {px.t01.x, px.t01.y, px.t01.z, px.t01.w};
          const float a10[4] = {px.t10.x, px.t10.y, px.t10.z, px.t10.w};
          const float a11[4] = {px.t11.x, px.t11.y, px.t11.z, px.t11.w};
          float gx = 0.0f, gy = 0.0f;
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) {
            gx += gch[ch] * (-(m00 * t.wy0 * a00[ch] + m01 * t.wy1 * a01[ch]) +
                             (m10 * t.wy0 * a10[ch] + m11 * t.wy1 * a11[ch]));
            gy += gch[ch] * (-(m00 * t.wx0 * a00[ch] + m10 * t.wx1 * a10[ch]) +
                             (m01 * t.wx0 * a01[ch] + m11 * t.wx1 * a11[ch]));
          }
          // u = q0 / den, v = q1 / den, den = q2 + 1e-8 [q2 == 0]
          gq0 = div_rn(gx, px.den);
          gq1 = div_rn(gy, px.den);
          gq2 = -div_rn(gx * px.u + gy * px.v, px.den);
        }
        float acc[NSUM] = {gq0 * x, gq0 * y, gq0, gq1 * x, gq1 * y, gq1,
                           gq2 * x, gq2 * y, gq2, gdd * x, gdd * y, gdd};
#pragma unroll
        for (int k = 0; k < NSUM; ++k) {
          float v = acc[k];
#pragma unroll
          for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
          if (lane == 0) red[(p * NW + wave) * NSUM + k] = v;
        }
      }
    }
  }
  if constexpr (RED) {
    __syncthreads();
    const int tid = (int)threadIdx.x;     // PB * NSUM <= 192 < TPB
    if (tid < P * NSUM) {
      const int p = tid / NSUM, k = tid - p * NSUM;
      float v = red[(p * NW) * NSUM + k];
#pragma unroll
      for (int w = 1; w < NW; ++w) v = v + red[(p * NW + w) * NSUM + k];
      a.part[(((size_t)bv * P + p) * a.nblk + blk) * NSUM + k] = v;
    }
  }
}

// g_hom / g_dmat: the workgroups' partials of one (world, view, plane), added
// one after the other.
__global__ __launch_bounds__(TPB) void render_planes_bwd_finish_kernel(
    const float* __restrict__ part, int n, int nblk, float* g_hom, float* g_dmat) {
  const int i = blockIdx.x * TPB + (int)threadIdx.x;   // (b, v, p, k)
  if (i >= n * NSUM) return;
  const int bvp = i / NSUM, k = i - bvp * NSUM;
  const float* q = part + (size_t)bvp * nblk * NSUM + k;
  float v = 0.0f;
  for (int j = 0; j < nblk; ++j) v = v + q[(size_t)j * NSUM];
  if (k < 9) { if (g_hom) g_hom[(size_t)bvp * 9 + k] = v; }
  else if (g_dmat) g_dmat[(size_t)bvp * 3 + (k - 9)] = v;
}

template <int PB>
void launch_bwd_pb(const BArgs& a, bool red, unsigned grid, hipStream_t st) {
  if (red)
    hipLaunchKernelGGL((render_planes_bwd_kernel<PB, true>), dim3(grid), dim3(TPB), 0, st, a);
  else
    hipLaunchKernelGGL((render_planes_bwd_kernel<PB, false>), dim3(grid), dim3(TPB), 0, st, a);
}

// The checks the forward and the backward share; 0 or an LSI_E* code.
int scene_desc_rc(const LsiSceneDesc* d, int64_t* nblk, int64_t* grid) {
  if (!d) return LSI_ENULL;
  if (d->B <= 0 || d->V <= 0 || d->P <= 0 || d->P > LSI_SCENE_MAX_PLANES ||
      d->Hs <= 0 || d->Ws <= 0 || d->H <= 0 || d->W <= 0 || d->n_box < 0 ||
      d->n_box > d->P)
    return LSI_EINVAL;
  const unsigned all = LSI_SCENE_IMG | LSI_SCENE_DISP | LSI_SCENE_IMG_ROOM |
                       LSI_SCENE_DISP_ROOM;
  if (d->outputs == 0 || (d->outputs & ~all)) return LSI_EINVAL;
  // tap indices are formed in fp32 (taps_of): exact up to 2^24 texels per plane
  if ((int64_t)d->Hs * d->Ws > (1 << 24) || (int64_t)d->H * d->W > (1 << 30))
    return LSI_EINVAL;
  *nblk = ((int64_t)d->H * d->W + TPB - 1) / TPB;
  *grid = *nblk * d->B * d->V;
  if (*grid > 0x7fffffffLL) return LSI_EINVAL;
  return LSI_OK;
}

}  // namespace

extern "C" {

int lsi_render_planes(const LsiSceneDesc* d, const float* tex_rgba, const float* hom,
                      const float* dmat, float* img, float* disp, float* img_room,
                      float* disp_room, lsi_stream_t stream) {
  int64_t nblk, grid;
  const int rc = scene_desc_rc(d, &nblk, &grid);
  if (rc != LSI_OK) return rc;
  if (!tex_rgba || !hom || !dmat) return LSI_ENULL;
  if (((d->outputs & LSI_SCENE_IMG) && !img) || ((d->outputs & LSI_SCENE_DISP) && !disp) ||
      ((d->outputs & LSI_SCENE_IMG_ROOM) && !img_room) ||
      ((d->outputs & LSI_SCENE_DISP_ROOM) && !disp_room))
    return LSI_ENULL;
  if ((uintptr_t)tex_rgba & 15u) return LSI_EINVAL;   // one 16-byte load per tap
  SArgs a;
  a.P = d->P; a.Hs = d->Hs; a.Ws = d->Ws; a.H = d->H; a.W = d->W; a.V = d->V;
  a.n_box = d->n_box; a.soft = d->soft != 0; a.nblk = (int)nblk;
  a.outputs = d->outputs; a.min_disp = d->min_disp; a.temp = d->temp;
  a.tex = reinterpret_cast<const float4*>(tex_rgba); a.hom = hom; a.dmat = dmat;
  a.img = img; a.disp = disp; a.img_room = img_room; a.disp_room = disp_room;
  const bool room = (d->outputs & (LSI_SCENE_IMG_ROOM | LSI_SCENE_DISP_ROOM)) != 0;
  hipStream_t st = (hipStream_t)stream;
  // the plane loop is unrolled to a compile-time bound: the smallest that holds P
  if (d->P <= 2) launch_pb<2>(a, room, (unsigned)grid, st);
  else if (d->P <= 5) launch_pb<5>(a, room, (unsigned)grid, st);
  else if (d->P <= 9) launch_pb<9>(a, room, (unsigned)grid, st);
  else launch_pb<16>(a, room, (unsigned)grid, st);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

size_t lsi_render_planes_bwd_workspace_bytes(const LsiSceneDesc* d) {
  int64_t nblk, grid;
  if (scene_desc_rc(d, &nblk, &grid) != LSI_OK) return 0;
  return (size_t)grid * d->P * NSUM * sizeof(float);
}

int lsi_render_planes_bwd(const LsiSceneDesc* d, const float* tex_rgba, const float* hom,
                          const float* dmat, const float* g_img, const float* g_disp,
                          float* g_tex, float* g_hom, float* g_dmat, void* workspace,
                          size_t workspace_bytes, lsi_stream_t stream) {
  int64_t nblk, grid;
  const int rc = scene_desc_rc(d, &nblk, &grid);
  if (rc != LSI_OK) return rc;
  // the room variants exist for data generation: forward only
  if (d->outputs & (LSI_SCENE_IMG_ROOM | LSI_SCENE_DISP_ROOM)) return LSI_EINVAL;
  if (!tex_rgba || !hom || !dmat || (!g_img && !g_disp)) return LSI_ENULL;
  if (((uintptr_t)tex_rgba & 15u) || ((uintptr_t)g_tex & 3u)) return LSI_EINVAL;
  const bool red = g_hom || g_dmat;
  if (red) {
    if (!workspace) return LSI_ENULL;
    if (((uintptr_t)workspace & 3u)) return LSI_EINVAL;
    if (workspace_bytes < lsi_render_planes_bwd_workspace_bytes(d)) return LSI_EWORKSPACE;
  }
  if (!red && !g_tex) return LSI_OK;     // nothing asked for
  BArgs a;
  a.P = d->P; a.Hs = d->Hs; a.Ws = d->Ws; a.H = d->H; a.W = d->W; a.V = d->V;
  a.soft = d->soft != 0; a.nblk = (int)nblk;
  a.min_disp = d->min_disp; a.temp = d->temp;
  a.tex = reinterpret_cast<const float4*>(tex_rgba); a.hom = hom; a.dmat = dmat;
  a.g_img = g_img; a.g_disp = g_disp; a.g_tex = g_tex;
  a.part = static_cast<float*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (d->P <= 2) launch_bwd_pb<2>(a, red, (unsigned)grid, st);
  else if (d->P <= 5) launch_bwd_pb<5>(a, red, (unsigned)grid, st);
  else if (d->P <= 9) launch_bwd_pb<9>(a, red, (unsigned)grid, st);
  else launch_bwd_pb<16>(a, red, (unsigned)grid, st);
  if (red) {
    const int n = d->B * d->V * d->P;
    hipLaunchKernelGGL(render_planes_bwd_finish_kernel, dim3((n * NSUM + TPB - 1) / TPB),
                       dim3(TPB), 0, st, a.part, n, (int)nblk, g_hom, g_dmat);
  }
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
