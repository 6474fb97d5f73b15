// Per-pixel arithmetic shared by the planar-layer kernels (gfx950): the bilinear
// gather's taps (lsi_sampling.hip), the soft z-buffer log-probability of one
// layer (lsi_loss.hip: compose / compose_depth) and the fused scene renderer
// (lsi_scene.hip), which must reproduce the other two bit for bit -- they
// compile this one copy.
#pragma once
#include "lsi_common.h"

#pragma clang fp contract(off)

namespace lsi {

// sampling.py:54-107: the four taps of one sampling point on an Hs x Ws image.
struct Taps {
  float wx0, wx1, wy0, wy1;  // un-masked interpolation weights
  float vx0, vx1, vy0, vy1;  // validity masks
  int i00, i01, i10, i11;    // flat x + y*Ws (00: x0,y0  01: x0,y1  10: x1,y0)
  bool ok;
};

__device__ __forceinline__ void taps_of(float u, float v, int Hs, int Ws,
                                        Taps& t) {
  const float x = u - 0.5f, y = v - 0.5f;
  t.ok = finite_f(x) && finite_f(y);
  const float x0 = floorf(x), x1 = x0 + 1.0f, y0 = floorf(y), y1 = y0 + 1.0f;
  const float xm = (float)(Ws - 1), ym = (float)(Hs - 1);
  const float x0s = fminf(fmaxf(x0, 0.f), xm), x1s = fminf(fmaxf(x1, 0.f), xm);
  const float y0s = fminf(fmaxf(y0, 0.f), ym), y1s = fminf(fmaxf(y1, 0.f), ym);
  t.wx0 = x1 - x; t.wx1 = x - x0; t.wy0 = y1 - y; t.wy1 = y - y0;
  t.vx0 = x0 == x0s ? 1.f : 0.f; t.vx1 = x1 == x1s ? 1.f : 0.f;
  t.vy0 = y0 == y0s ? 1.f : 0.f; t.vy1 = y1 == y1s ? 1.f : 0.f;
  const float w = (float)Ws;
  if (t.ok) {
    t.i00 = (int)(x0s + y0s * w); t.i01 = (int)(x0s + y1s * w);
    t.i10 = (int)(x1s + y0s * w); t.i11 = (int)(x1s + y1s * w);
  } else {
    t.i00 = t.i01 = t.i10 = t.i11 = 0;
  }
}

// sampling.py:118-123 (compose=True): valid_x * valid_y * wt_x * wt_y per tap,
// in the order 00, 01, 10, 11 ...
__device__ __forceinline__ void tap_weights(const Taps& t, float (&c)[4]) {
  c[0] = t.vx0 * t.vy0 * t.wx0 * t.wy0;
  c[1] = t.vx0 * t.vy1 * t.wx0 * t.wy1;
  c[2] = t.vx1 * t.vy0 * t.wx1 * t.wy0;
  c[3] = t.vx1 * t.vy1 * t.wx1 * t.wy1;
}

// ... and the sample, summed in that order; 0 for a non-finite point.  at(i) is
// the image's value at the flat tap index i = x + y*Ws.  (The one gather of
// lsi_bilinear_fwd, lsi_disocclusion_mask, lsi_geo_cons_loss_* and
// lsi_photo_reproj_loss_*.)
template <class At>
__device__ __forceinline__ float bilinear_gather_at(const Taps& t, const float (&c)[4],
                                                    At at) {
  float o = 0.0f;
  if (t.ok) {
    o = c[0] * at(t.i00);
    o = o + c[1] * at(t.i01);
    o = o + c[2] * at(t.i10);
    o = o + c[3] * at(t.i11);
  }
  return o;
}

// Channel ch of the sample of ib [Hs*Ws, C].
__device__ __forceinline__ float bilinear_gather(const Taps& t, const float (&c)[4],
                                                 const float* __restrict__ ib, int C,
                                                 int ch) {
  return bilinear_gather_at(t, c, [=](int i) { return ib[(size_t)i * C + ch]; });
}

// AREA resize for integer factors, one output cell: the box mean of the fy x fx
// block whose first element is p (element strides sy, sx), rows then columns in
// order, then one multiply by 1 / (fy fx).  NC channels sc apart.
template <int NC, typename T>
__device__ __forceinline__ void area_mean(const T* __restrict__ p, long sy, long sx,
                                          long sc, int fy, int fx, float (&t)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) t[c] = 0.0f;
  for (int dy = 0; dy < fy; ++dy)
    for (int dx = 0; dx < fx; ++dx) {
      const T* q = p + (long)dy * sy + (long)dx * sx;
#pragma unroll
      for (int c = 0; c < NC; ++c) t[c] += (float)q[c * sc];
    }
  const float inv = 1.0f / (float)(fy * fx);
#pragma unroll
  for (int c = 0; c < NC; ++c) t[c] *= inv;
}

// helpers.py:140-160: log-probability of a layer with mask value m whose
// (selection) disparity is dsel: log(m + 1e-8) - divide_safe(1, relu(dsel)) / temp.
__device__ __forceinline__ float layer_logp_of(float m, float dsel, float temp) {
  dsel = fmaxf(dsel, 0.0f);                                   // helpers.py:152
  const float depth = div_rn(1.0f, safe_den(dsel));           // divide_safe(1, d)
  const float lp = div_rn(-depth, temp);
  return logf(m + 1e-8f) + lp;
}

}  // namespace lsi
