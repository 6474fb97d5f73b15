// Device code that the convolution kernels share (lsi_conv*.hip; lsi_fc.hip
// takes the vector types): the fragment types, the DPP row sum, the transposing
// fragment read, the batch-norm statistics epilogue and its hand-over to
// lsi_bn_relu_norm, the fold of per-workgroup partial sums and the weight pack.
// One definition each: these carry protocols (workspace slots, K order,
// summation order) that the kernels on both sides must agree on.  The kernels'
// main loops, argument structs and launch shapes stay in their own files.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lsi_hip.h"
#include "lsi_bn_ws.h"

namespace lsi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// sum over the 16 lanes of a DPP row (every lane gets it)
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));  // row_mirror
  return v;
}

// The fragment of 16 channels x 32 pixels whose first pixel / channel `p`
// points at (pixel-major LDS rows, pixel pitch STRIDE elements): lane
// (t = lane % 16, g = lane / 16) gets channel t of its 8 pixels
// 16 (g / 2) + 4 (g % 2) + 8 h + r (the K order, the same for A and B; see
// lsi_conv_wgrad.hip on the bank layout).
template <int STRIDE>
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p, int t, int g) {
  const __bf16* q = p + (16 * (g >> 1) + 4 * (g & 1) + (t >> 2)) * STRIDE + 4 * (t & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)q);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(q + 8 * STRIDE));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ---- batch-norm statistics left by a convolution (lsi_bn_ws.h) -----------------
// The hand-over tag of group `grp`, which lsi_bn_relu_norm checks: stored by one
// thread of the producer's first workgroup of the group.
__device__ __forceinline__ void bn_stats_tag(float* ws, int grp, int C, int groups) {
  __hip_atomic_store(reinterpret_cast<int*>(ws + (size_t)grp * LSI_BN_WS_STRIDE) + LSI_BN_WS_TAG,
                     LSI_BN_TAG(C, groups), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// v added to the sum (q = 0: of y, 1: of y * y) of channel `ch` of C, in the
// accumulator slot of workgroup `f` (f mod ns): fire and forget.
__device__ __forceinline__ void bn_stats_add(float* ws, int grp, int f, int ns, int C, int q,
                                             int ch, float v) {
  __hip_atomic_fetch_add(ws + (size_t)grp * LSI_BN_WS_STRIDE + LSI_BN_WS_ACC +
                             (f % ns) * 2 * C + q * C + ch,
                         v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The epilogue of a workgroup of 4 waves whose lanes hold MFMA accumulators
// acc[r][c]: output channels co0 + 16 c + 4 (lane / 16) + e of pixel lane % 16
// of the wave's row r.  Sums of y and y * y of the bf16-ROUNDED outputs over the
// pixels with valid(r), per channel: over the lane's rows, the 16 pixels of a
// DPP row, then the four waves through red ([4 waves][2][16 NCT] floats of LDS
// that nobody reads any more: the caller's barrier, where it reuses memory),
// and one add per channel into the group's accumulators.  `first`: this is the
// group's first workgroup (it leaves the tag).  Every thread must call it.
template <int RW, int NCT, class Valid>
__device__ __forceinline__ void bn_stats_epilogue(const f32x4 (&acc)[RW][NCT], Valid valid,
                                                  float* red, float* ws, int grp, int groups,
                                                  int ns, int C, int co0, bool first) {
  constexpr int BN = 16 * NCT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pxl = lane & 15, kg = lane >> 4;
  float ss[NCT][4], qq[NCT][4];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) { ss[c][e] = 0.f; qq[c][e] = 0.f; }
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    if (valid(r)) {
#pragma unroll
      for (int c = 0; c < NCT; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = (float)(__bf16)acc[r][c][e];
          ss[c][e] += v;
          qq[c][e] = __builtin_fmaf(v, v, qq[c][e]);
        }
    }
  }
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) { ss[c][e] = row16_sum(ss[c][e]); qq[c][e] = row16_sum(qq[c][e]); }
  if (pxl == 0) {
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        red[(wave * 2 + 0) * BN + 16 * c + 4 * kg + e] = ss[c][e];
        red[(wave * 2 + 1) * BN + 16 * c + 4 * kg + e] = qq[c][e];
      }
  }
  __syncthreads();
  if (tid == 0 && first) bn_stats_tag(ws, grp, C, groups);
  if (tid < 2 * BN) {
    const int q = tid / BN, ch = tid - q * BN;
    const float v = (red[(0 * 2 + q) * BN + ch] + red[(1 * 2 + q) * BN + ch]) +
                    (red[(2 * 2 + q) * BN + ch] + red[(3 * 2 + q) * BN + ch]);
    const int f = (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
    bn_stats_add(ws, grp, f, ns, C, q, co0 + ch, v);
  }
}

// ---- the fold of per-workgroup partial sums ------------------------------------
// part[blk][n] -> one sum per entry, in a fixed order: workgroup = 64 entries x
// 16 groups of partials; group g sums partials g, g + 16, ... with four loads in
// flight, added to s[0..3] (the running sums of partials g + 64 i, + 16, + 32,
// + 48; the tail goes to s[0]); the caller combines the four -- the order is
// its own -- and hands the group's sum to part_fold_groups.
__device__ __forceinline__ void part_fold_sums(const float* part, int nblk, size_t n, int o,
                                               int grp, float (&s)[4]) {
  int w = grp;
  for (; w + 48 < nblk; w += 64) {
    s[0] += part[(size_t)w * n + o];
    s[1] += part[(size_t)(w + 16) * n + o];
    s[2] += part[(size_t)(w + 32) * n + o];
    s[3] += part[(size_t)(w + 48) * n + o];
  }
  for (; w < nblk; w += 16) s[0] += part[(size_t)w * n + o];
}
// The 16 group sums of entry `col` of the workgroup added in order through LDS:
// the sum in group 0's threads (0 elsewhere).  Every thread must call it.
__device__ __forceinline__ float part_fold_groups(float (*red)[64], int grp, int col, float s) {
  red[grp][col] = s;
  __syncthreads();
  float v = 0.0f;
  if (grp == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) v += red[k][col];
  }
  return v;
}

// ---- the weight pack -------------------------------------------------------------
// Weights into the implicit-GEMM kernels' operand order: dst[t][o][i] =
// W[o][i][ky_t][kx_t] (tr & 1 == 0) or W[i][o][ky_t][kx_t] (tr & 1: the data
// gradients), as T (bf16: rounded as torch.autocast rounds them).  W is the
// layer's fp32 parameter D0 x D1 x KH x KW.  A workgroup moves a 32 x 32 tile of
// (d0, d1) per tap through LDS, so that reads and (transposed) writes are both
// contiguous runs.  GUARD: D0, D1 need not be multiples of 32 (the edge tiles
// are guarded).
// PACK_TC taps per round: their 4 x PACK_TC loads per thread are in flight
// together and a round costs one pair of barriers (one tap per round was 338 us
// for the 36 M parameters x 2 directions of the networks: a chain of load
// latencies; the trainer packs after every optimiser step).
constexpr int PACK_TC = 8;
template <class T, bool GUARD>
__device__ __forceinline__ void pack_tile(const LsiPackJob& a, int bx, int by,
                                          float (*tile)[32][33]) {
  const int a0 = by * 32, b0 = bx * 32;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  const size_t per = (size_t)a.D0 * a.D1;
  T* const dst = reinterpret_cast<T*>(a.dst);
  for (int t0 = 0; t0 < a.ntaps; t0 += PACK_TC) {
    float v[PACK_TC][4];
#pragma unroll
    for (int tt = 0; tt < PACK_TC; ++tt) {
      const int tap = a.tap[min(t0 + tt, a.ntaps - 1)];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = r0 + 8 * j;
        // (the parameter D0 x D1 x KH x KW as torch stores it: contiguous, or --
        // tr & 2 -- channels-last strides, D0 x KH x KW x D1 in memory: what
        // module.to(memory_format=torch.channels_last) leaves)
        v[tt][j] = (GUARD && (a0 + r >= a.D0 || b0 + c >= a.D1)) ? 0.f
                   : (a.tr & 2) ? a.w[((size_t)(a0 + r) * a.khw + tap) * a.D1 + b0 + c]
                                : a.w[((size_t)(a0 + r) * a.D1 + b0 + c) * a.khw + tap];
      }
    }
#pragma unroll
    for (int tt = 0; tt < PACK_TC; ++tt)
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[tt][r0 + 8 * j][c] = v[tt][j];
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < PACK_TC; ++tt) {
      const int t = t0 + tt;
      if (t < a.ntaps) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = r0 + 8 * j;
          if (a.tr & 1) {   // dst[t][d1][d0]
            if (!GUARD || (b0 + r < a.D1 && a0 + c < a.D0))
              dst[(size_t)t * per + (size_t)(b0 + r) * a.D0 + a0 + c] = (T)tile[tt][c][r];
          } else if (!GUARD || (a0 + r < a.D0 && b0 + c < a.D1)) {   // dst[t][d0][d1]
            dst[(size_t)t * per + (size_t)(a0 + r) * a.D1 + b0 + c] = (T)tile[tt][r][c];
          }
        }
      }
    }
    __syncthreads();
  }
}
// Many layers in one launch: job j owns blocks [block0_j, block0_{j+1}) (the
// table lives in device memory and is read in place; the last entry's block0 +
// its blocks = grid); `which`: a word of LDS.
// (tile and which are the calling kernel's own __shared__ variables: declared in
// here, conv_pack_kernel takes 256 registers instead of 188.)
template <class T, bool GUARD>
__device__ __forceinline__ void pack_job_tile(const LsiPackJob* jobs, int njobs,
                                              float (*tile)[32][33], int* which) {
  if (threadIdx.x == 0) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].block0) ++j;
    *which = j;
  }
  __syncthreads();
  const LsiPackJob& a = jobs[*which];
  const int lb = (int)blockIdx.x - a.block0, nbx = (a.D1 + 31) / 32;
  pack_tile<T, GUARD>(a, lb % nbx, lb / nbx, tile);
}

}  // namespace lsi
