// Skinny-M fully-connected layer (+ batch norm + ReLU), forward and backward,
// for the FC-bottleneck network (nets.py: SlimFC, and `upcnv8` -- a 4 x 4
// stride-2 transposed convolution on a 1 x 1 map, which is a fully-connected
// layer over its four centre taps).  gfx950, v_mfma_f32_16x16x32_bf16.
//
// M = batch rows (<= 32), K and N in the thousands: the work is streaming the
// fp32 weight once per product.  The weight is the PARAMETER ITSELF, read in
// place through element strides (w_sn, w_sk) and up to four tap offsets, rounded
// to bf16 (nearest even) in registers -- no packed copy exists, so none can go
// stale behind an optimiser step.
//
// Arithmetic contract (what bf16 autocast does on the library route): operands
// rounded to bf16, products exact in fp32, fp32 accumulation; batch-norm
// statistics and normalisation in fp32; one rounding to bf16 at the output.
//
// Decomposition
//   fc_stream_kernel   one workgroup = one tile of 16 output columns x one chunk
//                      of the reduction; its four waves take the chunk's 32-deep
//                      steps in turn, each lane fetching 8 weights per step (two
//                      16-byte loads where the reduction runs along the unit
//                      stride, 8 strided dwords otherwise), four steps in flight.
//                      The activations (a few KB, L2-resident) are read once per
//                      workgroup straight into the A operand: a workgroup owns one
//                      column tile, so staging them in LDS would buy no reuse.
//                      The waves' tiles are summed through LDS in wave order and
//                      the chunk's partial tile goes to the workspace.
//                      The same kernel computes Z = X W^T (reduction over K) and
//                      dX = dZ W (reduction over N).
//   fc_fold_fwd_kernel sums the chunks in chunk order (no float atomics: bitwise
//                      reproducible), one thread per column holding the <= 32
//                      rows: mean / variance per batch-norm group, + beta, ReLU,
//                      one rounding.  fc_fold_kernel: the plain sum for dX.
//   fc_prep_bwd_kernel ReLU mask, dbeta, batch-norm backward per (group, column)
//                      -> dZ rounded once to bf16.
//   fc_dw_kernel       dW = dZ^T X is an outer-product sum over <= 32 rows: a
//                      write stream of the weight's size.  One lane owns four
//                      consecutive elements along the weight's unit stride (one
//                      16-byte store) for 8 positions of the other dimension;
//                      the <= 32-term sums run on the vector ALU (products of
//                      bf16 values are exact in fp32, as on the matrix cores).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_conv_device.h"   // (the vector types)

using namespace lsi;

namespace {

constexpr int kMaxM = 32;
constexpr int kWaves = 4;         // waves of a streaming workgroup
constexpr int kUnroll = 4;        // reduction steps a wave keeps in flight
constexpr int kTargetGroups = 512;  // workgroups aimed at (256 CUs, two each)
constexpr int kDwSlow = 8;        // positions of the slow dimension per lane (K, N % 8 == 0)

struct WeightView {
  int64_t sn, sk;
  int64_t tap_off[4];
  int32_t nt;   // output features per tap
};

__device__ __forceinline__ int64_t n_offset(const WeightView& v, int n) {
  const int t = n / v.nt;
  return v.tap_off[t] + (int64_t)(n - t * v.nt) * v.sn;
}

__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }

__device__ __forceinline__ float bf16_bits_to_float(unsigned short b) {
  return __uint_as_float((unsigned int)b << 16);
}

struct StreamArgs {
  const void* a;     // [M][R] row-major: bf16, or fp32 (a_f32) rounded on load
  const float* w;
  float* part;       // [splits][M][C]
  WeightView v;
  int32_t M, R, C;
  int32_t red_is_k;  // 1: R = K, C = N (forward); 0: R = N, C = K (dX)
  int32_t steps, steps_per_split;
  int32_t a_f32, vec;
};

// A operand of one step: 8 consecutive reduction elements of row `row`.
__device__ __forceinline__ bf16x8 load_a(const StreamArgs& s, int row, int r0, bool ok) {
  bf16x8 out;
  ok = ok && row < s.M;
  const size_t off = ok ? (size_t)row * s.R + r0 : 0;
  if (s.a_f32) {
    const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(s.a) + off);
    const f32x4 lo = p[0], hi = p[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[j] = (__bf16)(ok ? lo[j] : 0.0f);
      out[4 + j] = (__bf16)(ok ? hi[j] : 0.0f);
    }
  } else {
    u32x4 raw = *reinterpret_cast<const u32x4*>(static_cast<const __bf16*>(s.a) + off);
    if (!ok) raw = u32x4{0u, 0u, 0u, 0u};
    out = __builtin_bit_cast(bf16x8, raw);
  }
  return out;
}

template <int MT>
__global__ __launch_bounds__(kWaves * 64) void fc_stream_kernel(StreamArgs s) {
  __shared__ float red[kWaves][MT * 16][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, col = lane & 15;
  const int c0 = blockIdx.x * 16;
  const int c = c0 + col;
  const bool c_ok = c < s.C;
  const int cc = c_ok ? c : 0;
  // the lane's column part of the weight offset, and the stride of the reduction
  const int64_t cbase = s.red_is_k ? n_offset(s.v, cc) : (int64_t)cc * s.v.sk;
  const int64_t sr = s.red_is_k ? s.v.sk : s.v.sn;
  const int64_t safe = s.v.tap_off[0];   // an element that exists, for masked lanes

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int first = blockIdx.y * s.steps_per_split;
  const int last = min(first + s.steps_per_split, s.steps);
  for (int st0 = first + wave; st0 < last; st0 += kWaves * kUnroll) {
    float wv[kUnroll][8];
    bf16x8 av[kUnroll][MT];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int st = st0 + u * kWaves;
      const int r0 = st * 32 + q * 8;
      const bool r_ok = st < last && r0 < s.R;   // R is a multiple of 8
      ok[u] = r_ok && c_ok;
      const int rr = r_ok ? r0 : 0;
      const int64_t rbase = s.red_is_k ? (int64_t)rr * s.v.sk : n_offset(s.v, rr);
      const int64_t off = ok[u] ? cbase + rbase : safe;
      if (s.vec) {
        const f32x4* p = reinterpret_cast<const f32x4*>(s.w + (ok[u] ? off : 0));
        const f32x4 lo = p[0], hi = p[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) { wv[u][j] = lo[j]; wv[u][4 + j] = hi[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          wv[u][j] = s.w[off + (ok[u] ? j * sr : 0)];
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) av[u][t] = load_a(s, t * 16 + col, rr, r_ok);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      bf16x8 b;
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = (__bf16)(ok[u] ? wv[u][j] : 0.0f);
#pragma unroll
      for (int t = 0; t < MT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[u][t], b, acc[t], 0, 0, 0);
    }
  }
  // D layout: column = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[wave][t * 16 + q * 4 + e][col] = acc[t][e];
  __syncthreads();
  for (int i = threadIdx.x; i < MT * 256; i += kWaves * 64) {
    const int m = i >> 4, x = i & 15;
    float v = red[0][m][x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = v + red[w][m][x];
    if (m < s.M && c0 + x < s.C)
      s.part[((size_t)blockIdx.y * s.M + m) * s.C + c0 + x] = v;
  }
}

struct FoldFwdArgs {
  const float* part;
  const float* beta;
  void* y;
  float* z;
  float* mean_rstd;   // [groups][2][N]
  int32_t M, N, splits, groups, bn, out_f32;
  float eps;
};

__device__ __forceinline__ void store_out(void* y, size_t i, float v, int f32) {
  if (f32) static_cast<float*>(y)[i] = v;
  else static_cast<__bf16*>(y)[i] = (__bf16)v;
}

__global__ __launch_bounds__(64) void fc_fold_fwd_kernel(FoldFwdArgs a) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= a.N) return;
  float z[kMaxM];
#pragma unroll
  for (int m = 0; m < kMaxM; ++m) {
    z[m] = 0.0f;
    if (m < a.M) {
      float v = a.part[(size_t)m * a.N + n];
      for (int s = 1; s < a.splits; ++s) v = v + a.part[((size_t)s * a.M + m) * a.N + n];
      z[m] = v;
      if (a.z) a.z[(size_t)m * a.N + n] = v;
    }
  }
  if (!a.bn) {
#pragma unroll
    for (int m = 0; m < kMaxM; ++m)
      if (m < a.M) store_out(a.y, (size_t)m * a.N + n, z[m], a.out_f32);
    return;
  }
  const int rows = a.M / a.groups;
  const float inv = 1.0f / (float)rows;
  const float beta = a.beta[n];
  for (int g = 0; g < a.groups; ++g) {
    const int lo = g * rows, hi = lo + rows;
    float sum = 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxM; ++m)
      if (m >= lo && m < hi) sum = sum + z[m];
    const float mean = sum * inv;
    float sq = 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxM; ++m)
      if (m >= lo && m < hi) { const float d = z[m] - mean; sq = sq + d * d; }
    // one row per group: variance 0, (x - x) * rsqrt(eps) + beta -- TF's result
    const float rstd = 1.0f / sqrtf(sq * inv + a.eps);
    a.mean_rstd[((size_t)g * 2 + 0) * a.N + n] = mean;
    a.mean_rstd[((size_t)g * 2 + 1) * a.N + n] = rstd;
#pragma unroll
    for (int m = 0; m < kMaxM; ++m)
      if (m >= lo && m < hi) {
        const float v = (z[m] - mean) * rstd + beta;
        store_out(a.y, (size_t)m * a.N + n, fmaxf(v, 0.0f), a.out_f32);
      }
  }
}

__global__ __launch_bounds__(256) void fc_fold_kernel(const float* part, void* out, int64_t total,
                                                      int32_t splits, int32_t out_f32) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = part[i];
  for (int s = 1; s < splits; ++s) v = v + part[(int64_t)s * total + i];
  store_out(out, (size_t)i, v, out_f32);
}

struct PrepArgs {
  const void* dy;
  const void* y;
  const float* z;
  const float* mean_rstd;
  __bf16* dz;
  float* dbeta;
  int32_t M, N, groups, bn, io_f32;
};

__device__ __forceinline__ float load_io(const void* p, size_t i, int f32) {
  return f32 ? static_cast<const float*>(p)[i]
             : bf16_bits_to_float(static_cast<const unsigned short*>(p)[i]);
}

__global__ __launch_bounds__(64) void fc_prep_bwd_kernel(PrepArgs a) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= a.N) return;
  if (!a.bn) {
    for (int m = 0; m < a.M; ++m)
      a.dz[(size_t)m * a.N + n] = (__bf16)load_io(a.dy, (size_t)m * a.N + n, a.io_f32);
    return;
  }
  float g[kMaxM], z[kMaxM];
  float db = 0.0f;
#pragma unroll
  for (int m = 0; m < kMaxM; ++m) {
    g[m] = 0.0f;
    z[m] = 0.0f;
    if (m < a.M) {
      const size_t i = (size_t)m * a.N + n;
      const float yv = load_io(a.y, i, a.io_f32);
      const float dv = load_io(a.dy, i, a.io_f32);
      g[m] = yv > 0.0f ? dv : 0.0f;
      z[m] = a.z[i];
      db = db + g[m];
    }
  }
  a.dbeta[n] = db;
  const int rows = a.M / a.groups;
  const float inv = 1.0f / (float)rows;
  for (int gi = 0; gi < a.groups; ++gi) {
    const int lo = gi * rows, hi = lo + rows;
    const float mean = a.mean_rstd[((size_t)gi * 2 + 0) * a.N + n];
    const float rstd = a.mean_rstd[((size_t)gi * 2 + 1) * a.N + n];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxM; ++m)
      if (m >= lo && m < hi) {
        s1 = s1 + g[m];
        s2 = s2 + g[m] * ((z[m] - mean) * rstd);
      }
    s1 = s1 * inv;
    s2 = s2 * inv;
#pragma unroll
    for (int m = 0; m < kMaxM; ++m)
      if (m >= lo && m < hi) {
        const float xh = (z[m] - mean) * rstd;
        a.dz[(size_t)m * a.N + n] = (__bf16)(rstd * ((g[m] - s1) - xh * s2));
      }
  }
}

struct DwArgs {
  const void* x;      // [M][K] bf16 | fp32
  const __bf16* dz;   // [M][N]
  float* dw;
  WeightView v;
  int32_t M, K, N, x_f32, vec;
};

// FAST_K: the weight's unit stride runs along K (nn.Linear); else along N (a
// channels-last transposed-convolution weight).  Without a unit stride either
// orientation is right and the four elements are stored one by one.
template <bool FAST_K>
__global__ __launch_bounds__(64) void fc_dw_kernel(DwArgs a) {
  const int F = FAST_K ? a.K : a.N, S = FAST_K ? a.N : a.K;
  const int f = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int s0 = blockIdx.y * kDwSlow;
  const bool f_ok = f < F;     // F is a multiple of 8: the four go together
  const int ff = f_ok ? f : 0;
  float acc[kDwSlow][4];
#pragma unroll
  for (int r = 0; r < kDwSlow; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[r][i] = 0.0f;
  const unsigned short* dzb = reinterpret_cast<const unsigned short*>(a.dz);
  for (int m = 0; m < a.M; ++m) {
    float p[4];
    if (FAST_K) {
      if (a.x_f32) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(
            static_cast<const float*>(a.x) + (size_t)m * a.K + ff);
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = bf16_round(t[i]);
      } else {
        const u32x2 t = *reinterpret_cast<const u32x2*>(
            static_cast<const unsigned short*>(a.x) + (size_t)m * a.K + ff);
        p[0] = __uint_as_float(t[0] << 16); p[1] = __uint_as_float(t[0] & 0xffff0000u);
        p[2] = __uint_as_float(t[1] << 16); p[3] = __uint_as_float(t[1] & 0xffff0000u);
      }
    } else {
      const u32x2 t = *reinterpret_cast<const u32x2*>(dzb + (size_t)m * a.N + ff);
      p[0] = __uint_as_float(t[0] << 16); p[1] = __uint_as_float(t[0] & 0xffff0000u);
      p[2] = __uint_as_float(t[1] << 16); p[3] = __uint_as_float(t[1] & 0xffff0000u);
    }
    // the 8 slow positions of this block are 8 consecutive elements of row m
    // (S is a multiple of 8): one or two 16-byte loads, wave-uniform
    float qv[kDwSlow];
    if (!FAST_K && a.x_f32) {
      const f32x4* q4 = reinterpret_cast<const f32x4*>(
          static_cast<const float*>(a.x) + (size_t)m * a.K + s0);
      const f32x4 lo = q4[0], hi = q4[1];
#pragma unroll
      for (int i = 0; i < 4; ++i) { qv[i] = bf16_round(lo[i]); qv[4 + i] = bf16_round(hi[i]); }
    } else {
      const unsigned short* qb = FAST_K ? dzb + (size_t)m * a.N + s0
                                        : static_cast<const unsigned short*>(a.x) +
                                              (size_t)m * a.K + s0;
      const u32x4 t = *reinterpret_cast<const u32x4*>(qb);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qv[2 * i] = __uint_as_float(t[i] << 16);
        qv[2 * i + 1] = __uint_as_float(t[i] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int r = 0; r < kDwSlow; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[r][i] = __fmaf_rn(qv[r], p[i], acc[r][i]);
  }
  if (!f_ok) return;
#pragma unroll
  for (int r = 0; r < kDwSlow; ++r) {
    const int s = s0 + r;
    if (s >= S) break;
    const int64_t off = FAST_K ? n_offset(a.v, s) + (int64_t)f * a.v.sk
                               : n_offset(a.v, f) + (int64_t)s * a.v.sk;
    const int64_t sf = FAST_K ? a.v.sk : a.v.sn;
    if (a.vec) {
      *reinterpret_cast<f32x4*>(a.dw + off) = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) a.dw[off + i * sf] = acc[r][i];
    }
  }
}

// ---- host side -------------------------------------------------------------

bool desc_ok(const LsiFcDesc* d) {
  if (!d) return false;
  if (d->M < 1 || d->M > kMaxM || d->K < 8 || d->N < 8 || d->K > (1 << 20) || d->N > (1 << 20))
    return false;
  if (d->K % 8 || d->N % 8) return false;
  if (d->taps < 1 || d->taps > 4 || d->N % d->taps || (d->N / d->taps) % 8) return false;
  if (d->groups < 1 || d->M % d->groups) return false;
  if (d->w_sn < 1 || d->w_sk < 1) return false;
  for (int t = 0; t < d->taps; ++t)
    if (d->tap_off[t] < 0) return false;
  if (d->flags & ~(uint32_t)(LSI_FC_BN | LSI_FC_X_F32 | LSI_FC_OUT_F32)) return false;
  if (!(d->eps >= 0.0f)) return false;
  return true;
}

WeightView view_of(const LsiFcDesc* d) {
  WeightView v;
  v.sn = d->w_sn;
  v.sk = d->w_sk;
  v.nt = d->N / d->taps;
  for (int t = 0; t < 4; ++t) v.tap_off[t] = t < d->taps ? d->tap_off[t] : d->tap_off[0];
  return v;
}

// 16-byte accesses along a unit stride need every other offset a multiple of 4
bool vec_ok(const LsiFcDesc* d, int64_t unit, int64_t other, const void* w) {
  if (unit != 1 || other % 4 || ((uintptr_t)w & 15)) return false;
  for (int t = 0; t < d->taps; ++t)
    if (d->tap_off[t] % 4) return false;
  return true;
}

struct Split { int steps, per, splits; };

// chunks of the reduction: enough workgroups for the device, at least two steps
// per wave; a function of the shape alone, so the fold order is too
Split split_of(int R, int C) {
  Split s;
  s.steps = (R + 31) / 32;
  const int tiles = (C + 15) / 16;
  int want = (kTargetGroups + tiles - 1) / tiles;
  const int cap = s.steps / (2 * kWaves) > 1 ? s.steps / (2 * kWaves) : 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  s.per = (s.steps + want - 1) / want;
  s.splits = (s.steps + s.per - 1) / s.per;
  return s;
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

size_t fwd_bytes(const LsiFcDesc* d) {
  return align256((size_t)split_of(d->K, d->N).splits * d->M * d->N * sizeof(float));
}

size_t dz_bytes(const LsiFcDesc* d) { return align256((size_t)d->M * d->N * 2); }

size_t bwd_bytes(const LsiFcDesc* d) {
  return dz_bytes(d) +
         align256((size_t)split_of(d->N, d->K).splits * d->M * d->K * sizeof(float));
}

int launch_stream(const LsiFcDesc* d, const void* a, int a_f32, const float* w, float* part,
                  bool red_is_k, hipStream_t st) {
  StreamArgs s;
  s.a = a;
  s.w = w;
  s.part = part;
  s.v = view_of(d);
  s.M = d->M;
  s.R = red_is_k ? d->K : d->N;
  s.C = red_is_k ? d->N : d->K;
  s.red_is_k = red_is_k;
  const Split sp = split_of(s.R, s.C);
  s.steps = sp.steps;
  s.steps_per_split = sp.per;
  s.a_f32 = a_f32;
  s.vec = red_is_k ? vec_ok(d, d->w_sk, d->w_sn, w) : vec_ok(d, d->w_sn, d->w_sk, w);
  const dim3 grid((s.C + 15) / 16, sp.splits), blk(kWaves * 64);
  if (d->M > 16) hipLaunchKernelGGL(fc_stream_kernel<2>, grid, blk, 0, st, s);
  else hipLaunchKernelGGL(fc_stream_kernel<1>, grid, blk, 0, st, s);
  return sp.splits;
}

}  // namespace

extern "C" size_t lsi_fc_desc_bytes(void) { return sizeof(LsiFcDesc); }

extern "C" int lsi_fc_supported(const LsiFcDesc* d) { return desc_ok(d) ? 1 : 0; }

extern "C" size_t lsi_fc_workspace_bytes(const LsiFcDesc* d) {
  if (!desc_ok(d)) return 0;
  const size_t f = fwd_bytes(d), b = bwd_bytes(d);
  return f > b ? f : b;
}

extern "C" int lsi_fc_fwd(const LsiFcDesc* d, const void* x, const float* w, const float* beta,
                          void* y, float* z, float* mean_rstd, void* workspace,
                          size_t workspace_bytes, lsi_stream_t stream_) {
  if (!d) return LSI_ENULL;
  if (!desc_ok(d)) return LSI_EINVAL;
  const bool bn = d->flags & LSI_FC_BN;
  if (!x || !w || !y || !workspace || (bn && (!beta || !mean_rstd))) return LSI_ENULL;
  if (((uintptr_t)x & 15) || ((uintptr_t)workspace & 15)) return LSI_EINVAL;
  if (workspace_bytes < lsi_fc_workspace_bytes(d)) return LSI_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream_;
  float* part = static_cast<float*>(workspace);
  const int splits = launch_stream(d, x, (d->flags & LSI_FC_X_F32) ? 1 : 0, w, part, true, st);
  FoldFwdArgs f;
  f.part = part;
  f.beta = beta;
  f.y = y;
  f.z = z;
  f.mean_rstd = mean_rstd;
  f.M = d->M;
  f.N = d->N;
  f.splits = splits;
  f.groups = d->groups;
  f.bn = bn;
  f.out_f32 = (d->flags & LSI_FC_OUT_F32) ? 1 : 0;
  f.eps = d->eps;
  hipLaunchKernelGGL(fc_fold_fwd_kernel, dim3((d->N + 63) / 64), dim3(64), 0, st, f);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

extern "C" int lsi_fc_bwd(const LsiFcDesc* d, const void* x, const float* w, const void* dy,
                          const void* y, const float* z, const float* mean_rstd, void* dx,
                          float* dw, float* dbeta, void* workspace, size_t workspace_bytes,
                          lsi_stream_t stream_) {
  if (!d) return LSI_ENULL;
  if (!desc_ok(d)) return LSI_EINVAL;
  const bool bn = d->flags & LSI_FC_BN;
  if (!x || !w || !dy || !workspace) return LSI_ENULL;
  if (bn && (!y || !z || !mean_rstd || !dbeta)) return LSI_ENULL;
  if (((uintptr_t)x & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)dy & 15))
    return LSI_EINVAL;
  if (workspace_bytes < lsi_fc_workspace_bytes(d)) return LSI_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream_;
  const int io_f32 = (d->flags & LSI_FC_OUT_F32) ? 1 : 0;
  const int x_f32 = (d->flags & LSI_FC_X_F32) ? 1 : 0;
  const __bf16* dz = static_cast<const __bf16*>(dy);
  if (bn || io_f32) {     // (a bf16 dY without batch norm is dZ already)
    PrepArgs p;
    p.dy = dy;
    p.y = y;
    p.z = z;
    p.mean_rstd = mean_rstd;
    p.dz = static_cast<__bf16*>(workspace);
    p.dbeta = dbeta;
    p.M = d->M;
    p.N = d->N;
    p.groups = d->groups;
    p.bn = bn;
    p.io_f32 = io_f32;
    hipLaunchKernelGGL(fc_prep_bwd_kernel, dim3((d->N + 63) / 64), dim3(64), 0, st, p);
    dz = p.dz;
  }
  if (dw) {
    DwArgs a;
    a.x = x;
    a.dz = dz;
    a.dw = dw;
    a.v = view_of(d);
    a.M = d->M;
    a.K = d->K;
    a.N = d->N;
    a.x_f32 = x_f32;
    const bool fast_n = d->w_sn == 1 && d->w_sk != 1;
    const int F = fast_n ? d->N : d->K, S = fast_n ? d->K : d->N;
    const dim3 grid((F / 4 + 63) / 64, (S + kDwSlow - 1) / kDwSlow), blk(64);
    if (fast_n) {
      a.vec = vec_ok(d, d->w_sn, d->w_sk, dw);
      hipLaunchKernelGGL(fc_dw_kernel<false>, grid, blk, 0, st, a);
    } else {
      a.vec = vec_ok(d, d->w_sk, d->w_sn, dw);
      hipLaunchKernelGGL(fc_dw_kernel<true>, grid, blk, 0, st, a);
    }
  }
  if (dx) {
    float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + dz_bytes(d));
    const int splits = launch_stream(d, dz, 0, w, part, false, st);
    const int64_t total = (int64_t)d->M * d->K;
    hipLaunchKernelGGL(fc_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       part, dx, total, splits, x_f32);
  }
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}
