// Push-pull (pyramid) hole filling of a rendered image (gfx950): pixels carry a
// confidence, confident colour is summed down a pyramid of 2 x 2 boxes (push),
// and every pixel receives, in proportion to what it lacks, the bilinear
// up-sample of the level above (pull).  No reference counterpart; the
// definition is DESIGN.md section 4.22 and the header's comment.  All
// arithmetic is fp32 in the stated order without contraction (explicit
// __f*_rn, correctly rounded division), there are no atomics and every value
// has one writer, so the result is a function of the input alone, bit for bit.
//
// Kernels and what bounds them (one call, in launch order; LT = min(5, Lmax)):
//   push_kernel   a workgroup per 32 x 32 tile of level 0.  The tile's rows of
//                 img and w are staged in LDS by contiguous loads (stage_tile), level 1 is
//                 formed by a thread per pixel from its 2 x 2 children, levels
//                 2 .. LT by the first 64, 16, 4, 1 threads from LDS; every
//                 level is stored to the workspace as (p[C], c) per pixel.
//                 Bound by the one read of img and w (the stores are 1/3 of it).
//   mid_kernel    a workgroup per image: the level-LT map in LDS, pushed to
//                 1 x 1 and pulled back in place; stores F_LT.  A few KB per
//                 image: launch latency.
//   pull_kernel   a workgroup per tile: F_LT and then F of levels LT-1 .. 1 over
//                 the tile and a halo of one pixel in LDS (3^2, 4^2, 6^2, 10^2,
//                 18^2 pixels), level 0 recomputed from the staged inputs, F_0
//                 formed in place in the staged tile and stored as whole rows.
//                 Bound by the second read of img and w and the write of out.
// A 1 x 1 image (Lmax = 0) is pull_kernel alone.  The number of launches
// follows from the shape, never from the data.  No host synchronisation, no
// allocation, no state, plain vector stores only.
//
// LDS: push 32*32*(C + 1) + 341 (C + 1) floats (26.7 KB at C = 4), pull
// 32*32*(C + 1) + 485 C floats (27.6 KB), mid (C + 1) floats per pixel of the
// levels LT .. Lmax, at most MID_MAX_PIXELS pixels (50 KB at C = 4).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int TILE = LSI_FILL_TILE;               // 32
constexpr int TILE_LEVELS = 5;                    // 32 >> 5 = 1
constexpr int MID_MAX_PIXELS = LSI_FILL_MID_MAX_PIXELS;
// pixels of the tile's levels 1 .. 5: 256 + 64 + 16 + 4 + 1
constexpr int PUSH_PIXELS = 341;
// pixels of the tile's levels 5 .. 1 with a halo of one: 9 + 16 + 36 + 100 + 324
constexpr int PULL_PIXELS = 485;

static_assert(TILE == 1 << TILE_LEVELS && TPB * 4 == TILE * TILE, "tile shape");

struct Level {
  int h, w;                 // size
  int64_t off;              // floats: the pushed level in an image's block of workspace
};

struct FillArgs {
  const float* img;
  const float* w;
  float* out;
  float* ws;
  int H, W;
  int LT;                   // the tile kernels' top level, min(5, Lmax)
  int mode;
  int vec_img, vec_w;       // rows of img and out / of w start on 16 bytes in every full tile
  float bg_wt, bg_value, conf_min;
  Level lv[TILE_LEVELS + 1];      // level l (0: the image; its off is unused)
  int64_t foff;                   // floats: F_LT in an image's block
  int64_t block;                  // floats of workspace per image
};

// offset (pixels) of level l's region in pull_kernel's LDS, filled 5, 4, .. 1
__device__ __forceinline__ int pull_offset(int l) {
  return l == 5 ? 0 : l == 4 ? 9 : l == 3 ? 25 : l == 2 ? 61 : 161;
}

// Level l >= 1 of the plan, without indexing the kernel arguments by a register
// (that would move them to scratch memory).
__device__ __forceinline__ Level level_of(const FillArgs& a, int l) {
  Level r = a.lv[1];
#pragma unroll
  for (int k = 2; k <= TILE_LEVELS; ++k)
    if (l == k) r = a.lv[k];
  return r;
}

// Level 0 of a pixel: (p[C], c) from its colour and weight.
template <int C>
__device__ __forceinline__ float level0(const FillArgs& a, const float* v, float w, float* p) {
  float c;
  if (a.mode == LSI_FILL_CONF) {
    c = w > 0.0f ? fminf(w, 1.0f) : 0.0f;          // (a NaN fails the compare)
#pragma unroll
    for (int k = 0; k < C; ++k) p[k] = __fmul_rn(v[k], c);
  } else {
    c = w > a.bg_wt ? __fdiv_rn(__fsub_rn(w, a.bg_wt), w) : 0.0f;
    const float canvas = __fmul_rn(__fsub_rn(1.0f, c), a.bg_value);
#pragma unroll
    for (int k = 0; k < C; ++k) p[k] = __fsub_rn(v[k], canvas);
  }
  if (c < a.conf_min) c = 0.0f;
  if (c == 0.0f) {
#pragma unroll
    for (int k = 0; k < C; ++k) p[k] = 0.0f;       // selected, not multiplied
  }
  return c;
}

__device__ __forceinline__ float sum4(float a, float b, float c, float d) {
  return __fadd_rn(__fadd_rn(a, b), __fadd_rn(c, d));
}

// The push of one pixel from its four children (p[C], c) at s00 .. s11; a NULL
// child is out of range and counts as 0.
template <int C>
__device__ __forceinline__ void push4(const float* s00, const float* s01, const float* s10,
                                      const float* s11, float* d) {
  float s[C + 1];
#pragma unroll
  for (int k = 0; k <= C; ++k)
    s[k] = sum4(s00 ? s00[k] : 0.0f, s01 ? s01[k] : 0.0f, s10 ? s10[k] : 0.0f,
                s11 ? s11[k] : 0.0f);
  if (s[C] > 1.0f) {
#pragma unroll
    for (int k = 0; k < C; ++k) d[k] = __fdiv_rn(s[k], s[C]);
    d[C] = 1.0f;
  } else {
#pragma unroll
    for (int k = 0; k <= C; ++k) d[k] = s[k];
  }
}

// One channel of the 2 x bilinear up-sample from its four taps.
__device__ __forceinline__ float up4(float f00, float f01, float f10, float f11) {
  return __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(9.0f, f00), __fmul_rn(3.0f, f01)),
                             __fadd_rn(__fmul_rn(3.0f, f10), f11)),
                   0.0625f);
}

// the other tap of pixel y along an axis whose upper level has n pixels
__device__ __forceinline__ int neighbour(int y, int n) {
  const int v = (y >> 1) + ((y & 1) ? 1 : -1);
  return min(max(v, 0), n - 1);
}

// Stages the tile's rows of img (TILE x TILE x C) and w in LDS, zeros outside
// the image.  A tile of full width whose rows start on 16 bytes (vec_img,
// vec_w: judged on the host) moves as float4, a wave-instruction covering 1 KB
// of whole rows; any other by single floats, 256 contiguous bytes each.
template <int C>
__device__ __forceinline__ void stage_tile(const FillArgs& a, int n, int y0, int x0,
                                           float* s_img, float* s_w) {
  const int cols = min(TILE, a.W - x0);
  const int64_t base = ((int64_t)n * a.H + y0) * a.W + x0;
  if (a.vec_img && cols == TILE) {
#pragma unroll
    for (int j = 0; j < C; ++j) {                // TILE * TILE * C / 4 = TPB * C
      const int i = threadIdx.x + j * TPB, r = i / (8 * C), q = i - r * (8 * C);
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (y0 + r < a.H) v = reinterpret_cast<const float4*>(a.img + (base + (int64_t)r * a.W) * C)[q];
      reinterpret_cast<float4*>(s_img)[i] = v;
    }
  } else {
    for (int i = threadIdx.x; i < TILE * TILE * C; i += TPB) {
      const int r = i / (TILE * C), q = i - r * (TILE * C);
      s_img[i] = (y0 + r < a.H && q < cols * C) ? a.img[(base + (int64_t)r * a.W) * C + q] : 0.0f;
    }
  }
  if (a.vec_w && cols == TILE) {
    const int i = threadIdx.x, r = i >> 3, q = i & 7;    // TILE * TILE / 4 = TPB
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (y0 + r < a.H) v = reinterpret_cast<const float4*>(a.w + base + (int64_t)r * a.W)[q];
    reinterpret_cast<float4*>(s_w)[i] = v;
  } else {
    for (int i = threadIdx.x; i < TILE * TILE; i += TPB) {
      const int r = i / TILE, q = i - r * TILE;
      s_w[i] = (y0 + r < a.H && q < cols) ? a.w[base + (int64_t)r * a.W + q] : 0.0f;
    }
  }
}

template <int C>
__global__ __launch_bounds__(TPB) void push_kernel(FillArgs a) {
  constexpr int CP = C + 1;
  __shared__ __attribute__((aligned(16))) float s_img[TILE * TILE * C];
  __shared__ __attribute__((aligned(16))) float s_w[TILE * TILE];
  __shared__ float s_lv[PUSH_PIXELS * CP];
  const int n = blockIdx.z, ty0 = blockIdx.y, tx0 = blockIdx.x;
  stage_tile<C>(a, n, ty0 * TILE, tx0 * TILE, s_img, s_w);
  __syncthreads();
  float* ws = a.ws + (int64_t)n * a.block;
  // level 1: a thread per pixel, its children from the staged tile (a pixel
  // outside the image was staged with weight 0: c = 0 and p = 0 in both modes)
  {
    const int t = threadIdx.x, ly = t >> 4, lx = t & 15;
    float ch[4][CP];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = (2 * ly + (j >> 1)) * TILE + 2 * lx + (j & 1);
      ch[j][C] = level0<C>(a, s_img + q * C, s_w[q], ch[j]);
    }
    float d[CP];
    push4<C>(ch[0], ch[1], ch[2], ch[3], d);
#pragma unroll
    for (int k = 0; k < CP; ++k) s_lv[t * CP + k] = d[k];
    const int gy = ty0 * 16 + ly, gx = tx0 * 16 + lx;
    if (gy < a.lv[1].h && gx < a.lv[1].w) {
      float* o = ws + a.lv[1].off + ((int64_t)gy * a.lv[1].w + gx) * CP;
#pragma unroll
      for (int k = 0; k < CP; ++k) o[k] = d[k];
    }
  }
  // levels 2 .. LT from LDS
  int src = 0;                                 // pixels: level l - 1 in s_lv
  for (int l = 2; l <= a.LT; ++l) {            // (uniform: a kernel argument)
    __syncthreads();
    const int T = TILE >> l, dst = src + 4 * T * T;
    const int t = threadIdx.x;
    if (t < T * T) {
      const int ly = t / T, lx = t - ly * T;
      const float* s = s_lv + (src + 2 * ly * 2 * T + 2 * lx) * CP;
      float d[CP];
      push4<C>(s, s + CP, s + 2 * T * CP, s + (2 * T + 1) * CP, d);
#pragma unroll
      for (int k = 0; k < CP; ++k) s_lv[(dst + t) * CP + k] = d[k];
      const int gy = ty0 * T + ly, gx = tx0 * T + lx;
      const Level lv = level_of(a, l);
      if (gy < lv.h && gx < lv.w) {
        float* o = ws + lv.off + ((int64_t)gy * lv.w + gx) * CP;
#pragma unroll
        for (int k = 0; k < CP; ++k) o[k] = d[k];
      }
    }
    src = dst;
  }
}

// The levels LT .. Lmax of one image in LDS: (p[C], c) per pixel, level after
// level; the pull overwrites p by F.
template <int C>
__global__ __launch_bounds__(TPB) void mid_kernel(FillArgs a) {
  constexpr int CP = C + 1;
  extern __shared__ float s_mid[];
  __shared__ int s_h[32], s_w[32], s_off[32];   // per level from LT up; offsets in pixels
  __shared__ int s_levels;
  if (threadIdx.x == 0) {
    int h = level_of(a, a.LT).h, w = level_of(a, a.LT).w, off = 0, j = 0;
    for (;; ++j) {
      s_h[j] = h, s_w[j] = w, s_off[j] = off;
      if (h == 1 && w == 1) break;
      off += h * w;
      h = (h + 1) >> 1, w = (w + 1) >> 1;
    }
    s_levels = j + 1;
  }
  __syncthreads();
  const int levels = s_levels;
  float* ws = a.ws + (int64_t)blockIdx.x * a.block;
  const float* in = ws + level_of(a, a.LT).off;
  for (int i = threadIdx.x; i < s_h[0] * s_w[0] * CP; i += TPB) s_mid[i] = in[i];
  // push
  for (int j = 1; j < levels; ++j) {
    __syncthreads();
    const int h = s_h[j - 1], w = s_w[j - 1], nh = s_h[j], nw = s_w[j];
    const float* s = s_mid + s_off[j - 1] * CP;
    float* d = s_mid + s_off[j] * CP;
    for (int i = threadIdx.x; i < nh * nw; i += TPB) {
      const int y = i / nw, x = i - y * nw;
      const bool y1 = 2 * y + 1 < h, x1 = 2 * x + 1 < w;
      const float* s00 = s + (2 * y * w + 2 * x) * CP;
      push4<C>(s00, x1 ? s00 + CP : nullptr, y1 ? s00 + w * CP : nullptr,
               y1 && x1 ? s00 + (w + 1) * CP : nullptr, d + i * CP);
    }
  }
  __syncthreads();
  // pull: the coarsest level is one pixel
  if (threadIdx.x == 0) {
    float* d = s_mid + s_off[levels - 1] * CP;
    const float c = d[C];
#pragma unroll
    for (int k = 0; k < C; ++k) d[k] = c > 0.0f ? __fdiv_rn(d[k], c) : a.bg_value;
  }
  for (int j = levels - 2; j >= 0; --j) {
    __syncthreads();
    const int h = s_h[j], w = s_w[j], uh = s_h[j + 1], uw = s_w[j + 1];
    const float* u = s_mid + s_off[j + 1] * CP;
    float* d = s_mid + s_off[j] * CP;
    for (int i = threadIdx.x; i < h * w; i += TPB) {
      const int y = i / w, x = i - y * w;
      const int cy = y >> 1, cx = x >> 1, ny = neighbour(y, uh), nx = neighbour(x, uw);
      const float rest = __fsub_rn(1.0f, d[i * CP + C]);
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const float up = up4(u[(cy * uw + cx) * CP + k], u[(cy * uw + nx) * CP + k],
                             u[(ny * uw + cx) * CP + k], u[(ny * uw + nx) * CP + k]);
        d[i * CP + k] = __fadd_rn(d[i * CP + k], __fmul_rn(rest, up));
      }
    }
  }
  __syncthreads();
  float* out = ws + a.foff;
  for (int i = threadIdx.x; i < s_h[0] * s_w[0] * C; i += TPB) {
    const int q = i / C;
    out[i] = s_mid[q * CP + (i - q * C)];
  }
}

template <int C>
__global__ __launch_bounds__(TPB) void pull_kernel(FillArgs a) {
  constexpr int CP = C + 1;
  __shared__ __attribute__((aligned(16))) float s_img[TILE * TILE * C];
  __shared__ __attribute__((aligned(16))) float s_w[TILE * TILE];
  __shared__ float s_f[PULL_PIXELS * C];
  const int n = blockIdx.z, ty0 = blockIdx.y, tx0 = blockIdx.x;
  const int y0 = ty0 * TILE, x0 = tx0 * TILE;
  stage_tile<C>(a, n, y0, x0, s_img, s_w);
  const float* ws = a.ws + (int64_t)n * a.block;
  const int LT = a.LT;
  if (LT > 0) {
    // F_LT over the tile and its halo (entries outside the map are never read)
    const int T = TILE >> LT, R = T + 2, h = level_of(a, LT).h, w = level_of(a, LT).w;
    float* f = s_f + pull_offset(LT) * C;
    for (int i = threadIdx.x; i < R * R; i += TPB) {
      const int ly = i / R, lx = i - ly * R;
      const int gy = ty0 * T - 1 + ly, gx = tx0 * T - 1 + lx;
      const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
      const float* s = ws + a.foff + ((int64_t)gy * w + gx) * C;
#pragma unroll
      for (int k = 0; k < C; ++k) f[i * C + k] = in ? s[k] : 0.0f;
    }
  }
  for (int l = LT - 1; l >= 1; --l) {          // (uniform: a kernel argument)
    __syncthreads();
    const Level lv = level_of(a, l), up = level_of(a, l + 1);
    const int T = TILE >> l, R = T + 2, UR = T / 2 + 2, h = lv.h, w = lv.w;
    const int uy0 = ty0 * (T / 2) - 1, ux0 = tx0 * (T / 2) - 1;   // the upper region's origin
    const float* u = s_f + pull_offset(l + 1) * C;
    float* f = s_f + pull_offset(l) * C;
    for (int i = threadIdx.x; i < R * R; i += TPB) {
      const int ly = i / R, lx = i - ly * R;
      const int gy = ty0 * T - 1 + ly, gx = tx0 * T - 1 + lx;
      if (gy < 0 || gy >= h || gx < 0 || gx >= w) continue;
      const int cy = (gy >> 1) - uy0, cx = (gx >> 1) - ux0;
      const int ny = neighbour(gy, up.h) - uy0, nx = neighbour(gx, up.w) - ux0;
      const float* pc = ws + lv.off + ((int64_t)gy * w + gx) * CP;
      const float rest = __fsub_rn(1.0f, pc[C]);
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const float us = up4(u[(cy * UR + cx) * C + k], u[(cy * UR + nx) * C + k],
                             u[(ny * UR + cx) * C + k], u[(ny * UR + nx) * C + k]);
        f[i * C + k] = __fadd_rn(pc[k], __fmul_rn(rest, us));
      }
    }
  }
  __syncthreads();
  // level 0 from the staged inputs, F_0 in place of the staged colour
  const float* u = s_f + pull_offset(1) * C;
  const int uy0 = ty0 * 16 - 1, ux0 = tx0 * 16 - 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = threadIdx.x + j * TPB, ly = q >> 5, lx = q & 31;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= a.H || gx >= a.W) continue;
    float p[C];
    const float c = level0<C>(a, s_img + q * C, s_w[q], p);
    if (LT == 0) {                               // a 1 x 1 image: the coarsest level
#pragma unroll
      for (int k = 0; k < C; ++k) s_img[q * C + k] = c > 0.0f ? __fdiv_rn(p[k], c) : a.bg_value;
      continue;
    }
    const int cy = (gy >> 1) - uy0, cx = (gx >> 1) - ux0;
    const int ny = neighbour(gy, a.lv[1].h) - uy0, nx = neighbour(gx, a.lv[1].w) - ux0;
    const float rest = __fsub_rn(1.0f, c);
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float up = up4(u[(cy * 18 + cx) * C + k], u[(cy * 18 + nx) * C + k],
                           u[(ny * 18 + cx) * C + k], u[(ny * 18 + nx) * C + k]);
      s_img[q * C + k] = __fadd_rn(p[k], __fmul_rn(rest, up));
    }
  }
  __syncthreads();
  const int cols = min(TILE, a.W - x0);
  const int64_t base = ((int64_t)n * a.H + y0) * a.W + x0;
  if (a.vec_img && cols == TILE) {
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const int i = threadIdx.x + j * TPB, r = i / (8 * C), q = i - r * (8 * C);
      if (y0 + r < a.H)
        reinterpret_cast<float4*>(a.out + (base + (int64_t)r * a.W) * C)[q] =
            reinterpret_cast<const float4*>(s_img)[i];
    }
  } else {
    for (int i = threadIdx.x; i < TILE * TILE * C; i += TPB) {
      const int r = i / (TILE * C), q = i - r * (TILE * C);
      if (y0 + r < a.H && q < cols * C) a.out[(base + (int64_t)r * a.W) * C + q] = s_img[i];
    }
  }
}

// The plan of a shape: level sizes, workspace layout, mid_kernel's pixels.
// false for a shape the call refuses.
bool plan(int32_t N, int32_t H, int32_t W, int32_t C, FillArgs* a, int* mid_pixels) {
  if (N < 1 || N > 65535 || H < 1 || W < 1 || C < 1 || C > 4) return false;
  if ((int64_t)N * H * W > (1ll << 28)) return false;
  int h = H, w = W, lmax = 0;
  int64_t off = 0;
  a->H = H, a->W = W;
  a->lv[0].h = H, a->lv[0].w = W, a->lv[0].off = 0;
  while (h > 1 || w > 1) {
    h = (h + 1) >> 1, w = (w + 1) >> 1;
    ++lmax;
    if (lmax <= TILE_LEVELS) {
      a->lv[lmax].h = h, a->lv[lmax].w = w, a->lv[lmax].off = off;
      off += (int64_t)h * w * (C + 1);
    }
  }
  a->LT = lmax < TILE_LEVELS ? lmax : TILE_LEVELS;
  a->foff = off;
  a->block = off + (int64_t)a->lv[a->LT].h * a->lv[a->LT].w * C;
  int64_t pixels = 0;
  h = a->lv[a->LT].h, w = a->lv[a->LT].w;
  for (;;) {
    pixels += (int64_t)h * w;
    if (pixels > MID_MAX_PIXELS) return false;
    if (h == 1 && w == 1) break;
    h = (h + 1) >> 1, w = (w + 1) >> 1;
  }
  *mid_pixels = (int)pixels;
  return true;
}

template <int C>
int launch(const FillArgs& a, int32_t N, int mid_pixels, hipStream_t stream) {
  const dim3 tiles((a.W + TILE - 1) / TILE, (a.H + TILE - 1) / TILE, N);
  if (a.LT > 0) {
    hipLaunchKernelGGL(push_kernel<C>, tiles, dim3(TPB), 0, stream, a);
    hipLaunchKernelGGL(mid_kernel<C>, dim3(N), dim3(TPB),
                       (size_t)mid_pixels * (C + 1) * sizeof(float), stream, a);
  }
  hipLaunchKernelGGL(pull_kernel<C>, tiles, dim3(TPB), 0, stream, a);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // namespace

extern "C" {

size_t lsi_fill_holes_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
  FillArgs a;
  int mid_pixels;
  if (!plan(N, H, W, C, &a, &mid_pixels)) return 0;
  const size_t bytes = (size_t)N * (size_t)a.block * sizeof(float);
  return bytes < 16 ? 16 : bytes;
}

int lsi_fill_holes(int32_t N, int32_t H, int32_t W, int32_t C, const float* img,
                   const float* w, int32_t mode, float bg_wt, float bg_value,
                   float conf_min, float* out, void* workspace, size_t workspace_bytes,
                   lsi_stream_t stream) {
  FillArgs a;
  int mid_pixels;
  if (!plan(N, H, W, C, &a, &mid_pixels)) return LSI_EINVAL;
  if (mode != LSI_FILL_CONF && mode != LSI_FILL_SPLAT) return LSI_EINVAL;
  if (!isfinite(bg_value) || !isfinite(conf_min) || conf_min < 0.0f) return LSI_EINVAL;
  if (mode == LSI_FILL_SPLAT && !(isfinite(bg_wt) && bg_wt >= 0.0f)) return LSI_EINVAL;
  if (!img || !w || !out || !workspace) return LSI_ENULL;
  if (((uintptr_t)workspace & 3) != 0) return LSI_EINVAL;
  if (workspace_bytes < lsi_fill_holes_workspace_bytes(N, H, W, C)) return LSI_EWORKSPACE;
  a.img = img, a.w = w, a.out = out, a.ws = static_cast<float*>(workspace);
  a.mode = mode, a.bg_wt = bg_wt, a.bg_value = bg_value, a.conf_min = conf_min;
  // a full tile's row starts (n H W + y W + 32 k) C floats into img and out
  a.vec_img = (int64_t)W * C % 4 == 0 && (((uintptr_t)img | (uintptr_t)out) & 15) == 0;
  a.vec_w = W % 4 == 0 && ((uintptr_t)w & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: return launch<1>(a, N, mid_pixels, s);
    case 2: return launch<2>(a, N, mid_pixels, s);
    case 3: return launch<3>(a, N, mid_pixels, s);
    default: return launch<4>(a, N, mid_pixels, s);
  }
}

}  // extern "C"
