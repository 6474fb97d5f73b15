// Depth accuracy of a predicted inverse-depth map against ground truth on the
// device (gfx950): the seven figures of the protocol of Eigen et al. 2014
// (abs-rel, sq-rel, RMSE, RMSE-log, delta < 1.25^k) per image, with the optional
// per-image median scaling, added to a caller-owned device array of
// LSI_DEPTH_SLOTS doubles.  No reference counterpart; the definition is
// DESIGN.md section 4.16 and the header's comment.
// Bound: HBM streaming of 2-3 maps (pred, gt, mask), a few MB per call -- launch
// latency in practice: 2 launches, 10 with median scaling (4 digit passes of a
// radix select, each a histogram and a scan kernel), whatever the data.
// Loads: one dword per lane, a wave reads 256 contiguous bytes of a crop row
// run (the crop starts at any column, so wider loads would not be aligned),
// four pixels per thread in flight.
// Reductions: per-thread fp32, per-block and final sums in fp64 in a fixed
// order (lsi_reduce.h); the select counts with integer LDS atomics and stores
// per-block histograms, so nothing depends on the order of arrival.  The
// accumulator is updated by thread 0 of a one-block finishing kernel, images
// in index order: a sequence of calls is reproducible bit for bit.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"
#include "lsi_reduce.h"

// thresholds and clamps are compared in fp32 exactly as written
#pragma clang fp contract(off)

using namespace lsi;

namespace {

constexpr int DEPTH_MAXBPI = 64;  // blocks per image (and partial sums per scalar)
constexpr int NSEL = 4;           // selections: (dg, dp_raw) x (lower, upper middle rank)
constexpr int NBIN = 256;         // one 8-bit digit per pass
constexpr int NPASS = 4;
static_assert(TPB == NBIN, "a histogram block has one thread per digit");

enum { D_ABS_REL, D_SQ_REL, D_SE, D_SE_LOG, D_A1, D_A2, D_A3, D_N, D_NSUM };

struct DepthArgs {
  int H, W, y0, x0, ch, cw;  // the crop: ch x cw pixels from (y0, x0)
  const float* pred;         // [B, H, W]
  const float* gt;           // [B, H, W]
  const void* mask;          // [B, H, W] float or uint8, or NULL
  const float* gt_scale;     // [B]
  int mask_u8;
  float valid_above, depth_min, depth_max;
};

// The state of one image's select between the passes.
struct SelState {
  uint32_t prefix[NSEL];  // the digits decided so far, in place
  uint32_t rank[NSEL];    // the rank wanted among the keys that share them
  uint32_t n;             // |V_b|
  float s;                // the scale the metric pass applies
};

inline int blocks_per_image(long n) {
  long g = (n + TPB - 1) / TPB;
  return (int)(g > DEPTH_MAXBPI ? DEPTH_MAXBPI : g);
}

// f(dg, dp_raw) for every scored pixel of image b that this block's grid-stride
// pass over the crop meets: dg the true depth, dp_raw the unscaled predicted
// depth.  Whether a pixel is scored is a function of the ground truth (and the
// mask) alone.  UNROLL pixels at a time, their loads issued before any is
// judged: with one block per CU the pass is bound by load latency, not bytes.
constexpr int UNROLL = 4;

template <class F>
__device__ __forceinline__ void for_scored_pixels(const DepthArgs& a, int b, F f) {
  const float scale = a.gt_scale[b];
  const int n = a.ch * a.cw, step = gridDim.x * TPB;
  for (int i0 = blockIdx.x * TPB + threadIdx.x; i0 < n; i0 += UNROLL * step) {
    float g[UNROLL], pr[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int i = i0 + u * step;
      g[u] = 0.0f;  // (never above valid_above >= 0: not scored)
      pr[u] = 0.0f;
      if (i < n) {
        const int y = a.y0 + i / a.cw, x = a.x0 + i % a.cw;
        const long p = ((long)b * a.H + y) * a.W + x;
        g[u] = a.gt[p];
        pr[u] = a.pred[p];
        if (a.mask) {
          const bool m = a.mask_u8 ? ((const uint8_t*)a.mask)[p] != 0
                                   : ((const float*)a.mask)[p] != 0.0f;
          if (!m) g[u] = 0.0f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (!(g[u] > a.valid_above)) continue;
      const float dg = div_rn(1.0f, g[u] * scale);
      if (!(dg >= a.depth_min && dg <= a.depth_max)) continue;
      // fmaxf drops a NaN operand: zero, negative and NaN predictions become a
      // huge finite depth (a +Inf prediction is depth 0: see the header)
      f(dg, div_rn(1.0f, fmaxf(pr[u], FLT_MIN)));
    }
  }
}

// ---------------------------------------------------------------------------
// median scaling: radix select of the middle ranks, one 8-bit digit per pass.
// Positive floats order as their bit patterns do.
// ---------------------------------------------------------------------------
// Counts, per block, the digit `pass` of the keys that share every selection's
// decided digits: hist[((b * gridDim.x + block) * NSEL + j) * NBIN + digit].
__global__ __launch_bounds__(TPB) void depth_select_hist_kernel(
    DepthArgs a, int pass, const SelState* st, uint32_t* hist) {
  __shared__ uint32_t h[NSEL][NBIN];
  const int b = blockIdx.y;
  uint32_t prefix[NSEL];
#pragma unroll
  for (int j = 0; j < NSEL; ++j) prefix[j] = 0u;
  if (pass > 0) {
    if (st[b].n == 0u) return;  // (uniform: the scan skips this image as well)
#pragma unroll
    for (int j = 0; j < NSEL; ++j) prefix[j] = st[b].prefix[j];
  }
  for (int j = 0; j < NSEL; ++j) h[j][threadIdx.x] = 0u;  // TPB == NBIN
  __syncthreads();
  // the lower and the upper middle rank share their digits until the two values
  // part (for an odd count they never do): one count then serves both
  const bool twin_g = prefix[1] == prefix[0], twin_p = prefix[3] == prefix[2];
  const int shift = 24 - 8 * pass;
  const uint32_t decided = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
  for_scored_pixels(a, b, [&](float dg, float dp_raw) {
    const uint32_t kg = __float_as_uint(dg), kp = __float_as_uint(dp_raw);
#pragma unroll
    for (int j = 0; j < NSEL; ++j) {
      if ((j == 1 && twin_g) || (j == 3 && twin_p)) continue;
      const uint32_t key = j < 2 ? kg : kp;
      if ((key & decided) == prefix[j]) atomicAdd(&h[j][(key >> shift) & 255u], 1u);
    }
  });
  __syncthreads();
  uint32_t* out = hist + ((size_t)b * gridDim.x + blockIdx.x) * NSEL * NBIN;
  for (int j = 0; j < NSEL; ++j) {
    const int src = (j == 1 && twin_g) || (j == 3 && twin_p) ? j - 1 : j;
    out[j * NBIN + threadIdx.x] = h[src][threadIdx.x];
  }
}

// One block per image, one thread per selection and digit: sums the nblk partial
// histograms, finds the digit that holds each wanted rank and records it; the
// last pass turns the four selected values into the image's scale.
__global__ __launch_bounds__(NSEL * NBIN) void depth_select_scan_kernel(
    int pass, int nblk, const uint32_t* hist, SelState* st) {
  __shared__ uint32_t cum[NSEL][NBIN];
  __shared__ uint32_t chosen[NSEL];
  const int b = blockIdx.x, t = threadIdx.x % NBIN, j = threadIdx.x / NBIN;
  // the state is read here, before the barriers of the scan, and written after
  uint32_t n = 0u, prefix = 0u, want = 0u;
  if (pass > 0) {
    n = st[b].n;
    if (n == 0u) return;
    prefix = st[b].prefix[j];
    want = st[b].rank[j];
  }
  const uint32_t* hp = hist + ((size_t)b * nblk * NSEL + j) * NBIN + t;
  uint32_t c = 0u;
#pragma unroll 8
  for (int k = 0; k < nblk; ++k) c += hp[(size_t)k * NSEL * NBIN];
  cum[j][t] = c;
  __syncthreads();
  // inclusive scan over the 256 digits (Hillis-Steele), the four side by side
  for (int off = 1; off < NBIN; off <<= 1) {
    const uint32_t add = t >= off ? cum[j][t - off] : 0u;
    __syncthreads();
    cum[j][t] += add;
    __syncthreads();
  }
  if (pass == 0) {
    n = cum[0][NBIN - 1];
    if (n == 0u) {  // nothing scored: the later passes and the metrics skip it
      if (threadIdx.x == 0) {
        st[b].n = 0u;
        st[b].s = 1.0f;
      }
      return;
    }
    // the lower middle rank for even j, the upper for odd j (equal for odd n)
    want = (j & 1) ? n / 2u : (n - 1u) / 2u;
  }
  const uint32_t incl = cum[j][t], excl = incl - c;
  if (excl <= want && want < incl) {  // exactly one digit holds the rank
    const uint32_t p = prefix | ((uint32_t)t << (24 - 8 * pass));
    chosen[j] = p;
    st[b].prefix[j] = p;
    st[b].rank[j] = want - excl;
  }
  if (pass == 0 && threadIdx.x == 0) st[b].n = n;
  if (pass != NPASS - 1) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mg = 0.5 * ((double)__uint_as_float(chosen[0]) +
                             (double)__uint_as_float(chosen[1]));
    const double mp = 0.5 * ((double)__uint_as_float(chosen[2]) +
                             (double)__uint_as_float(chosen[3]));
    st[b].s = (float)(mg / mp);
  }
}

// ---------------------------------------------------------------------------
// the metric pass and its finishing kernel
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void depth_metrics_kernel(DepthArgs a, const SelState* st,
                                                            double* part) {
  const int b = blockIdx.y;
  const float s = st ? st[b].s : 1.0f;
  float acc[D_NSUM];
#pragma unroll
  for (int k = 0; k < D_NSUM; ++k) acc[k] = 0.0f;
  for_scored_pixels(a, b, [&](float dg, float dp_raw) {
    const float dp = fminf(fmaxf(s * dp_raw, a.depth_min), a.depth_max);
    const float e = dg - dp;
    const float le = logf(dg) - logf(dp);
    const float r = fmaxf(div_rn(dg, dp), div_rn(dp, dg));
    acc[D_ABS_REL] += div_rn(fabsf(e), dg);
    acc[D_SQ_REL] += div_rn(e * e, dg);
    acc[D_SE] += e * e;
    acc[D_SE_LOG] += le * le;
    acc[D_A1] += r < 1.25f ? 1.0f : 0.0f;
    acc[D_A2] += r < 1.5625f ? 1.0f : 0.0f;
    acc[D_A3] += r < 1.953125f ? 1.0f : 0.0f;
    acc[D_N] += 1.0f;
  });
  block_store_partials<D_NSUM>(acc, part + (size_t)b * D_NSUM * DEPTH_MAXBPI, DEPTH_MAXBPI);
}

// One block.  A round takes TPB / D_NSUM images: a thread per image and scalar
// sums that scalar's nblk partials in index order, a thread per image turns the
// eight sums into the image's row, and thread 0 adds the rows to the
// accumulator, images in index order.
constexpr int FIN_IMAGES = TPB / D_NSUM;

__global__ __launch_bounds__(TPB) void depth_finish_kernel(
    const double* part, int nblk, int B, const SelState* st, double* acc,
    double* per_image) {
  __shared__ double sums[FIN_IMAGES][D_NSUM];
  __shared__ double rows[FIN_IMAGES][LSI_DEPTH_PER_IMAGE];
  const int li = threadIdx.x / D_NSUM, k = threadIdx.x % D_NSUM;
  for (int b0 = 0; b0 < B; b0 += FIN_IMAGES) {
    const int b = b0 + li;
    if (b < B) {
      const double* p = part + ((size_t)b * D_NSUM + k) * DEPTH_MAXBPI;
      double s = 0.0;
#pragma unroll 8
      for (int i = 0; i < nblk; ++i) s += p[i];
      sums[li][k] = s;
    }
    __syncthreads();
    if (b < B && k == 0) {
      const double* s = sums[li];
      const double n = s[D_N];
      double* row = rows[li];
      for (int c = 0; c < LSI_DEPTH_PER_IMAGE; ++c) row[c] = 0.0;
      if (n > 0.0) {
        row[LSI_DEPTH_ABS_REL] = s[D_ABS_REL] / n;
        row[LSI_DEPTH_SQ_REL] = s[D_SQ_REL] / n;
        row[LSI_DEPTH_RMSE] = sqrt(s[D_SE] / n);
        row[LSI_DEPTH_RMSE_LOG] = sqrt(s[D_SE_LOG] / n);
        row[LSI_DEPTH_A1] = s[D_A1] / n;
        row[LSI_DEPTH_A2] = s[D_A2] / n;
        row[LSI_DEPTH_A3] = s[D_A3] / n;
        row[LSI_DEPTH_SCALE] = st ? (double)st[b].s : 1.0;
        row[LSI_DEPTH_IMAGES] = n;  // (per_image: n_b in this column, then the flag)
        row[LSI_DEPTH_IMAGES + 1] = 1.0;
      }
      if (per_image)
        for (int c = 0; c < LSI_DEPTH_PER_IMAGE; ++c)
          per_image[(size_t)b * LSI_DEPTH_PER_IMAGE + c] = row[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < FIN_IMAGES && b0 + i < B; ++i) {
        if (rows[i][LSI_DEPTH_IMAGES + 1] == 0.0) continue;
        for (int c = 0; c < LSI_DEPTH_IMAGES; ++c) acc[c] += rows[i][c];
        acc[LSI_DEPTH_IMAGES] += 1.0;
      }
    }
    __syncthreads();
  }
}

// workspace: [partial sums][select states][partial histograms]
size_t part_bytes(int B) { return (size_t)B * D_NSUM * DEPTH_MAXBPI * sizeof(double); }
size_t state_bytes(int B) { return ((size_t)B * sizeof(SelState) + 15) / 16 * 16; }
size_t hist_bytes(int B, int bpi) {
  return (size_t)B * bpi * NSEL * NBIN * sizeof(uint32_t);
}

// B is a grid dimension; a pixel index and the strides past the last pixel of
// the unrolled pass stay below 2^31.
bool dims_ok(int32_t B, int32_t H, int32_t W) {
  return B > 0 && H > 0 && W > 0 && B <= 65535 &&
         (int64_t)H * W < (1ll << 31) - 2 * UNROLL * TPB * DEPTH_MAXBPI;
}

}  // namespace

extern "C" {

size_t lsi_eval_depth_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t median) {
  if (!dims_ok(B, H, W)) return 0;
  size_t n = part_bytes(B);
  if (median) n += state_bytes(B) + hist_bytes(B, blocks_per_image((long)H * W));
  return n;
}

int lsi_eval_depth_metrics(int32_t B, int32_t H, int32_t W, const float* pred,
                           const float* gt, const void* mask, const float* gt_scale,
                           int32_t y0, int32_t y1, int32_t x0, int32_t x1,
                           float valid_above, float depth_min, float depth_max,
                           uint32_t flags, double* acc, double* per_image,
                           void* ws, size_t ws_bytes, lsi_stream_t stream) {
  if (!dims_ok(B, H, W) || (flags & ~(LSI_DEPTH_MASK_U8 | LSI_DEPTH_MEDIAN)))
    return LSI_EINVAL;
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1) return LSI_EINVAL;
  if (!(depth_min > 0.0f) || !(depth_max >= depth_min) || !(valid_above >= 0.0f))
    return LSI_EINVAL;
  if (!pred || !gt || !gt_scale || !acc || !ws) return LSI_ENULL;
  const int median = (flags & LSI_DEPTH_MEDIAN) ? 1 : 0;
  if (ws_bytes < lsi_eval_depth_workspace_bytes(B, H, W, median)) return LSI_EWORKSPACE;
  DepthArgs a;
  a.H = H; a.W = W; a.y0 = y0; a.x0 = x0; a.ch = y1 - y0; a.cw = x1 - x0;
  a.pred = pred; a.gt = gt; a.mask = mask; a.gt_scale = gt_scale;
  a.mask_u8 = (flags & LSI_DEPTH_MASK_U8) ? 1 : 0;
  a.valid_above = valid_above; a.depth_min = depth_min; a.depth_max = depth_max;
  const int bpi = blocks_per_image((long)a.ch * a.cw);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  SelState* st = NULL;
  if (median) {
    st = (SelState*)((char*)ws + part_bytes(B));
    uint32_t* hist = (uint32_t*)((char*)st + state_bytes(B));
    for (int pass = 0; pass < NPASS; ++pass) {
      hipLaunchKernelGGL(depth_select_hist_kernel, dim3(bpi, B), dim3(TPB), 0, s, a, pass,
                         (const SelState*)st, hist);
      hipLaunchKernelGGL(depth_select_scan_kernel, dim3(B), dim3(NSEL * NBIN), 0, s, pass, bpi,
                         (const uint32_t*)hist, st);
    }
  }
  hipLaunchKernelGGL(depth_metrics_kernel, dim3(bpi, B), dim3(TPB), 0, s, a,
                     (const SelState*)st, part);
  hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(TPB), 0, s, (const double*)part,
                     bpi, (int)B, (const SelState*)st, acc, per_image);
  return rc_of_launch();
}

}  // extern "C"
