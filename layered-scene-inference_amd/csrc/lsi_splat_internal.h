// Internal (non-ABI) declarations shared by the splat translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"

struct SplatArgs {
  LsiSplatDesc d;
  const float* tex;
  const float* disp;
  const float* mask;
  const float* M;
  float* out_img;
  float* out_wts;
  float* out_disp;
  float* canvas;  // caller's workspace: ATOMIC canvases / STREAM exchange area
  size_t ws_bytes;
  int nch;        // canvas channels (4, or 5 with disparity)
  int ncanv;      // canvases per batch element (1 or L)
  int shared;     // 1: compose without disparity, all layers share a canvas
  int band_rows;  // ROWBAND: target rows per workgroup
  // lsi_splat_fwd_both: the composed outputs next to the per-layer ones (NULL
  // otherwise)
  float* out_img_c;
  float* out_wts_c;
};

// lsi_stream_ok's return value (kept in LsiSplatDesc.tune_window): window cells,
// plus this bit when every batch element has M rows 2, 3 = (0,0,1,0), (0,0,0,1).
constexpr int LSI_STREAM_SIMPLE_BIT = 1 << 20;
// (also set by lsi_stream_ok) every batch element's vertical magnification
// M[1][1] is >= 1: a band of R target rows reads at most ceil((R + 1) / s)
// source rows, what the launchers plan their tables for
constexpr int LSI_STREAM_ROWS_BIT = 1 << 21;
constexpr int LSI_STREAM_FLAG_BITS = LSI_STREAM_SIMPLE_BIT | LSI_STREAM_ROWS_BIT;

// LSI_PATH_STREAM launcher and workspace need (lsi_splat_stream.hip).
size_t lsi_stream_workspace_bytes(const LsiSplatDesc* d);
int lsi_stream_launch(const SplatArgs& a, hipStream_t stream);
// The compact STREAM instance (lsi_splat_stream2.hip): compose mode, no mask,
// unit normaliser, channels-last textures or RGBD pixels, W % 4 == 0.
bool lsi_stream2_applies(const SplatArgs& a, bool simple, int layout);
// disp_pass: the per-layer-tile instance as the disparity pass (only output:
// a.out_disp = max over layers of each layer's normalised splatted disparity)
int lsi_stream2_launch(const SplatArgs& a, int wmax, hipStream_t stream,
                       bool disp_pass = false);

// The streamed backward for rectified pairs (lsi_splat_bwd_stream.hip).  It
// derives the gradient canvas from the forward's outputs and their incoming
// gradients itself (no pre-pass): `ci` the per-layer (or the only) canvases,
// `cc` lsi_splat_bwd_both's composed one; either may be NULL / have g_img NULL.
struct LsiBwdCanvas {
  const float* img;
  const float* wts;
  const float* g_img;
  const float* g_wts;  // may be NULL
};
bool lsi_bwd_stream_applies(const LsiSplatDesc* d, const float* tex,
                            const float* disp, const float* mask,
                            const float* g_tex, const float* g_disp,
                            const float* g_mask);
// gm_part != NULL (LSI_GRAD_M): every workgroup also writes its 16-float share
// of dL/dM there, `*gm_nper` of them per batch element (b-major).
// gd != NULL (lsi_splat_bwd_disp): the per-layer (gS, gW) canvases of the
// target disparity, [L][B][Ht * Wt], read from memory at each corner.
int lsi_bwd_stream_launch(const LsiSplatDesc* d, const float* tex,
                          const float* disp, const float* mask, const float* M,
                          const LsiBwdCanvas* ci, const LsiBwdCanvas* cc,
                          float* g_tex, float* g_disp, float* g_mask,
                          float* gm_part, int* gm_nper, hipStream_t stream,
                          const float2* gd = nullptr);

// LSI_PATH_TILE launcher and workspace need (lsi_splat_tile.hip).
size_t lsi_tile_workspace_bytes(const LsiSplatDesc* d);
int lsi_tile_launch(const SplatArgs& a, hipStream_t stream);

// The any-pose sweep kernel (lsi_splat_sweep.hip), launched by lsi_tile_launch
// after the disparity ranges (range[(l * B + b) * LSI_RANGE_SLICES + k] =
// {min, max} of a slice of rows) are on the stream.
#define LSI_RANGE_SLICES 8
#define LSI_SWEEP_MAXL 16
int lsi_sweep_launch(const SplatArgs& a, const float2* range, hipStream_t stream);

// ---- device primitives of the STREAM kernels --------------------------------
// One definition for lsi_splat_stream.hip, its compact instance
// lsi_splat_stream2.hip and the sweep / backward kernels: the two STREAM kernels
// promise identical index and clamp decisions, and these are what decides them.
// (Index-critical products below rely on lsi_common.h's fp contract(off).)

// compiler-only memory barrier: orders a wave's plain LDS accesses in the code
#define LSI_COMPILER_FENCE() asm volatile("" ::: "memory")
#define LSI_RFL(x) __builtin_amdgcn_readfirstlane(x)

namespace lsi {

// (host) 16-byte alignment, what the kernels' dwordx4 accesses need
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// n / d for 0 <= n < 2^22, d > 0, rcp = fl(1/d): no integer-division sequence
__device__ __forceinline__ int div_small(int n, int d, float rcp) {
  int q = (int)((float)n * rcp);
  const int r = n - q * d;
  q += (r >= d) ? 1 : 0;
  q -= (r < 0) ? 1 : 0;
  return q;
}

// n-th float above / below a positive finite float
__device__ __forceinline__ float next_up(float t) {
  return __int_as_float(__float_as_int(t) + 1);
}
__device__ __forceinline__ float next_down(float t) {
  return __int_as_float(__float_as_int(t) - 1);
}

// Smallest side weight w with fl(w * wy) > 1e-3f (sampling.py:218-222 keeps a
// corner iff its rounded weight product exceeds 1e-3).  fp32 rounding is
// monotone, so "w >= threshold" is EXACTLY "fl(w*wy) > 1e-3f" for every w:
// one compare instead of a multiply and a compare in the hot loop.  +Inf when
// no weight <= 1 qualifies.
__device__ __forceinline__ float clamp_threshold(float wy) {
  if (!(wy > 0.0f)) return __builtin_inff();
  float t = div_rn(1.0e-3f, wy);
  if (!(t < 4.0f)) return __builtin_inff();
  for (int k = 0; k < 8; ++k) {
    const float p = next_down(t);
    if (p * wy > 1.0e-3f) t = p; else break;
  }
  for (int k = 0; k < 8; ++k) {
    if (!(t * wy > 1.0e-3f)) t = next_up(t); else break;
  }
  return t;
}

// lane l-1's value by DPP wave_shr:1 (VALU, no LDS round trip); lane 0 gets 0
__device__ __forceinline__ float lane_below(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xf,
                                                 0xf, true));
}

// accumulations are not index-critical: fused multiply-add
__device__ __forceinline__ float4 f4_fma(float4 t, float4 v, float w) {
  t.x = __fmaf_rn(v.x, w, t.x); t.y = __fmaf_rn(v.y, w, t.y);
  t.z = __fmaf_rn(v.z, w, t.z); t.w = __fmaf_rn(v.w, w, t.w);
  return t;
}

// Try-lock / unlock of one LDS lock word (byte address): writes 1, returns what
// was there (0 = acquired).  Integer LDS exchanges are cheap; `ds_add_f32` is not.
__device__ __forceinline__ void cell_try2(unsigned a0, unsigned a1, int& o0, int& o1) {
  const int one = 1;
  asm volatile(
      "ds_wrxchg_rtn_b32 %0, %2, %4\n\tds_wrxchg_rtn_b32 %1, %3, %4\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(o0), "=&v"(o1)
      : "v"(a0), "v"(a1), "v"(one)
      : "memory");
}
__device__ __forceinline__ int cell_try1(unsigned a0) {
  int o;
  const int one = 1;
  asm volatile("ds_wrxchg_rtn_b32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(o) : "v"(a0), "v"(one) : "memory");
  return o;
}
__device__ __forceinline__ void cell_unlock(unsigned a0) {
  const int zero = 0;
  asm volatile("ds_write_b32 %0, %1" : : "v"(a0), "v"(zero) : "memory");
}

// Folded fields: several lanes of a wave name the same window cell and must add
// one after the other.  `cnt` is the wave's table of one byte per window cell
// (four cells per word, zero between uses): ONE returning integer LDS add per
// lane yields its rank among the lanes of its cell (a wave has 64 lanes: a byte
// never carries into its neighbour); the caller runs rounds k = 0, 1, ... in
// which the lanes of rank k add (distinct cells within a round), then clears
// the words it touched.  (Round 3 elected one lane per cell and round through a
// byte written and read back: two more LDS operations per round.)
__device__ __forceinline__ int cell_rank(unsigned char* cnt, int cell, bool act) {
  if (!act) return -1;
  const unsigned sh = 8u * ((unsigned)cell & 3u);
  const unsigned old = atomicAdd(reinterpret_cast<unsigned*>(cnt + (cell & ~3)), 1u << sh);
  return (int)((old >> sh) & 0xffu);
}
__device__ __forceinline__ void cell_rank_reset(unsigned char* cnt, int cell, bool act) {
  if (act) *reinterpret_cast<unsigned*>(cnt + (cell & ~3)) = 0u;
}

}  // namespace lsi
