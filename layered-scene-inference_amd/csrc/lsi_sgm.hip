// Semi-global matching on a census cost for a rectified stereo pair on the
// device (gfx950): both views' disparities, 16-bit, disparity * 256 with 0 for
// "no match" -- the format of the KITTI ground-truth maps data.py loads.  No
// reference counterpart (the reference shells out to an external matcher); the
// definition is DESIGN.md section 4.17 and the header's comment.  Everything is
// integer arithmetic: the result is a function of the input bytes alone.
//
// Both views run through the same kernels.  View 0 is the left image matched
// against the right one; view 1 is the right image matched against the left
// one, stored mirrored in x (census_kernel writes a mirrored copy of either
// census), so that in its own coordinates it is a left view as well:
//   cost(y, x, d) = popcount(A[y][x] ^ M[y][x - d]),   62 where x - d < 0.
// The set of path directions is closed under the mirroring.
//
// Kernels and what bounds them (one call, in launch order):
//   grey_kernel      bytes in, bytes out; launch latency.
//   census_kernel    62 cached byte loads per pixel, one 8-byte store (twice:
//                    plain and mirrored); L1/L2 rate, small.
//   path_row_kernel  x2 (left-to-right, right-to-left): a wave per (view, image,
//                    row); lane l holds the K = ceil(D / 64) disparities
//                    l K .. l K + K - 1.  The census words M[x - d] live in a
//                    register window that moves by one disparity per step
//                    through the lanes (DPP wave shift), the step's one new
//                    word comes out of a 64-word chunk register by v_readlane.
//                    Bound by the latency of the step's dependent chain (wave
//                    minimum -> neighbour exchange -> byte arithmetic) times W;
//                    the sums a step adds to are loaded a group of steps ahead,
//                    so that no memory round trip is part of the chain.
//   path_col_kernel  x2 (paths = 4) or x6: a wave per (view, image, column of
//                    the first row); it walks down (or up) the rows, its column
//                    moving by dx = 0, +1 or -1 per row and wrapping at the
//                    image's edge, where the path starts anew -- every line has
//                    H steps and the W waves together cover every diagonal.
//                    A step's census words and sums are loaded a group of
//                    steps ahead.  Same chain, times H.
//   Every path launch adds its L_r into one 16-bit volume S[view][b][y][x][d]
//   in place (the first stores): within a launch every (pixel, d) belongs to
//   one lane, launches are ordered by the stream, integer sums have no order.
//   winner_kernel    a wave per pixel: first argmin, second minimum outside
//                    d0 +- 1, uniqueness, sub-pixel offset; streams S once.
//   lr_kernel        a thread per pixel: the left-right check, both outputs.
// No LDS, no atomics, no floating point, no state; plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int WAVE = 64;
constexpr int TPB = 256;          // 4 waves: 4 lines (or 4 pixels) per block
constexpr int WPB = TPB / WAVE;
constexpr int CENSUS_RX = 4, CENSUS_RY = 3;  // 9 x 7 window
constexpr int COST_OUT = 62;      // the cost of a disparity that leaves the image
constexpr int BIG = 1 << 14;      // above every path cost (<= 255) and sum (<= 2040)
constexpr int MAX_P2 = 193;       // 62 + P2 <= 255
constexpr uint32_t RAW_OK = 1u << 31;   // winner record: q | d0 << 16 | acceptable << 31

// ---------------------------------------------------------------------------
// cross-lane primitives (wave64, DPP; no LDS)
// ---------------------------------------------------------------------------
// Lane l's value of lane l - 1; lane 0 gets `edge`.
__device__ __forceinline__ int from_lane_below(int v, int edge) {
  return __builtin_amdgcn_update_dpp(edge, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
// Lane l's value of lane l + 1; lane 63 gets `edge`.
__device__ __forceinline__ int from_lane_above(int v, int edge) {
  return __builtin_amdgcn_update_dpp(edge, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

// The minimum over the wave's 64 lanes, in every lane (wave-uniform): a scan
// inside each row of 16 lanes, two row broadcasts, and lane 63 read back.
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112 /* row_shr:2 */, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114 /* row_shr:4 */, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118 /* row_shr:8 */, 0xf, 0xf, false));
  // lane 15 of every row now holds its row's minimum
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

struct SgmArgs {
  int B, H, W, D, P1, P2;
  const uint64_t* cen;   // [4][B][H][W]: left, right, left mirrored, right mirrored
  uint16_t* S;           // [2][B][H][W][D]
};

// the census planes of a view: A the view's own image, M the one it is matched to
__device__ __forceinline__ const uint64_t* plane_a(const SgmArgs& a, int view) {
  return a.cen + (size_t)(view ? 3 : 0) * a.B * a.H * a.W;
}
__device__ __forceinline__ const uint64_t* plane_m(const SgmArgs& a, int view) {
  return a.cen + (size_t)(view ? 2 : 1) * a.B * a.H * a.W;
}

// ---------------------------------------------------------------------------
// One step of the recurrence for the lane's K disparities d0 .. d0 + K - 1:
//   L(d) = C(d) + min(Lp(d), Lp(d - 1) + P1, Lp(d + 1) + P1, m + P2) - m,
// m the minimum of the previous pixel's costs (wave-uniform); `start`: the
// previous pixel is outside the image, L = C.  Disparities >= D hold BIG and
// never win a minimum.
// ---------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void path_step(int (&L)[K], const int (&c)[K], int d0, int D,
                                          int P1, int P2, bool start) {
  if (start) {
#pragma unroll
    for (int k = 0; k < K; ++k) L[k] = d0 + k < D ? c[k] : BIG;
    return;
  }
  int lmin = L[0];
#pragma unroll
  for (int k = 1; k < K; ++k) lmin = min(lmin, L[k]);
  const int m = wave_min(lmin);
  const int below = from_lane_below(L[K - 1], BIG);
  const int above = from_lane_above(L[0], BIG);
  int n[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int dm = k > 0 ? L[k - 1] : below;
    const int dp = k < K - 1 ? L[k + 1] : above;
    const int t = min(min(L[k], min(dm, dp) + P1), m + P2);
    n[k] = d0 + k < D ? c[k] + t - m : BIG;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) L[k] = n[k];
}

// The lane's K sums S[d0 .. d0 + K - 1] of one pixel (`pix` its D values, 32-byte
// aligned): contiguous, one access of 2 K bytes where that is a power of two.
// A load stays packed until it is used and is issued by every lane -- a lane
// whose disparities do not exist reads the pixel's last ones instead -- so that
// nothing waits for it where it is issued.  With K = 1, 2, 4 a lane holds K
// disparities or none (D is a multiple of 16); with K = 3 the last one may hold
// fewer, and the accesses go one by one.
template <int K>
struct Packed {
  static constexpr int R = K == 2 ? 1 : K == 4 ? 2 : K;
  uint32_t r[R];
};

template <int K>
__device__ __forceinline__ void load_sums(const uint16_t* pix, int d0, int D, Packed<K>& v) {
  if constexpr (K == 2) {
    v.r[0] = *(const uint32_t*)(pix + min(d0, D - 2));
  } else if constexpr (K == 4) {
    const uint2 w = *(const uint2*)(pix + min(d0, D - 4));
    v.r[0] = w.x;
    v.r[1] = w.y;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) v.r[k] = pix[min(d0 + k, D - 1)];
  }
}

template <int K>
__device__ __forceinline__ int sum_of(const Packed<K>& v, int k) {
  if constexpr (K == 2 || K == 4) return (int)((v.r[k >> 1] >> (16 * (k & 1))) & 0xffffu);
  return (int)v.r[k];
}

// FULL: D = 64 K, every lane holds K disparities and the store is unconditional.
template <int K, bool FULL>
__device__ __forceinline__ void store_sums(uint16_t* pix, int d0, int D, const int (&s)[K]) {
  uint16_t* p = pix + d0;
  if (FULL || d0 + K <= D) {
    if constexpr (K == 2) {
      *(uint32_t*)p = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
    } else if constexpr (K == 4) {
      uint2 v;
      v.x = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
      v.y = (uint32_t)s[2] | ((uint32_t)s[3] << 16);
      *(uint2*)p = v;
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) p[k] = (uint16_t)s[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (d0 + k < D) p[k] = (uint16_t)s[k];
  }
}

// Steps of a line that are loaded together, one group ahead of the recurrence:
// the loads of a step must be several steps old when the step needs them, or
// their latency is the step's.
template <int K>
struct Group {
  static constexpr int N = K <= 2 ? 8 : 4;
};

// Whole groups run as straight-line code (Tail = false: no bounds checks, and
// with FULL no lane predicate): the compiler can then count the stores between a
// load and its use, and waits for the load alone, not for the stores' replies.
struct NoTail { static constexpr bool value = false; };
struct Tail { static constexpr bool value = true; };

// Keeps a loaded value from being waited for later than here.
__device__ __forceinline__ void settle(uint64_t& v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  asm volatile("" : "+v"(lo), "+v"(hi));
  v = ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------------
// grey and census
// ---------------------------------------------------------------------------
// left, right: [B][H][W][C] each; grey: [2][B][H][W], the left images first.
__global__ __launch_bounds__(TPB) void grey_kernel(const uint8_t* left, const uint8_t* right,
                                                   int C, size_t n, uint8_t* grey) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= 2 * n) return;
  const uint8_t* src = i < n ? left : right;
  const size_t p = i < n ? i : i - n;
  int g;
  if (C == 3) {
    g = (77 * src[3 * p] + 150 * src[3 * p + 1] + 29 * src[3 * p + 2] + 128) >> 8;
  } else {
    g = src[p];
  }
  grey[i] = (uint8_t)g;
}

// grey: [2][B][H][W]; cen: [4][B][H][W] (left, right, left mirrored, right
// mirrored).  Bit j of a word is neighbour j of the window in row-major order,
// centre skipped; the mirrored planes hold the same words at x' = W - 1 - x.
__global__ __launch_bounds__(TPB) void census_kernel(const uint8_t* grey, int B, int H, int W,
                                                     uint64_t* cen) {
  const size_t n = (size_t)B * H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= 2 * n) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const uint8_t* img = grey + (i - (size_t)y * W - x);  // the image's first pixel
  const int c = img[(size_t)y * W + x];
  uint64_t bits = 0;
#pragma unroll
  for (int dy = -CENSUS_RY; dy <= CENSUS_RY; ++dy) {
    const int yy = min(max(y + dy, 0), H - 1);
    const uint8_t* row = img + (size_t)yy * W;
#pragma unroll
    for (int dx = -CENSUS_RX; dx <= CENSUS_RX; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const int xx = min(max(x + dx, 0), W - 1);
      bits = (bits << 1) | (uint64_t)(row[xx] < c ? 1 : 0);
    }
  }
  cen[i] = bits;
  cen[2 * n + (i - x) + (W - 1 - x)] = bits;
}

// ---------------------------------------------------------------------------
// horizontal paths: wave = (view, b, y); dir = +1 scans x upwards (r = (0, +1)),
// dir = -1 downwards.
// ---------------------------------------------------------------------------
template <int K, bool FULL>
__global__ __launch_bounds__(TPB) void path_row_kernel(SgmArgs a, int dir, int first) {
  constexpr int G = Group<K>::N;
  const int lane = threadIdx.x & (WAVE - 1);
  const long line = (long)blockIdx.x * WPB + (threadIdx.x >> 6);
  const long lines = 2l * a.B * a.H;
  if (line >= lines) return;  // (whole waves leave)
  const int view = (int)(line / ((long)a.B * a.H));
  const size_t row = (size_t)(line % ((long)a.B * a.H));  // b * H + y
  const int W = a.W, D = a.D;
  const uint64_t* A = plane_a(a, view) + row * W;
  const uint64_t* M = plane_m(a, view) + row * W;
  uint16_t* S = a.S + ((size_t)view * a.B * a.H + row) * W * D;
  const int d0 = lane * K;

  // win[k] = M[x - (d0 + k)] at step x.  Scanning upwards the window starts
  // empty (a word is used only after it entered at d = 0); downwards it starts
  // as of x = W and every step takes the word of d + 1, a new one entering at
  // d = D - 1.
  uint64_t win[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    win[k] = 0;
    if (dir < 0) win[k] = M[min(max(W - (d0 + k), 0), W - 1)];
  }
  int L[K];
#pragma unroll
  for (int k = 0; k < K; ++k) L[k] = BIG;

  // step j visits x = j (upwards) or W - 1 - j; the sums of the G steps of a
  // group are loaded while the group before it runs.  The first launch loads
  // them too (whatever the workspace holds) and drops them: no branch.
  Packed<K> cur[G], nxt[G];
  auto load_group = [&](int jbase, Packed<K> (&grp)[G], auto tail) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int j = jbase + g;
      if (!decltype(tail)::value || j < W)
        load_sums<K>(S + (size_t)(dir > 0 ? j : W - 1 - j) * D, d0, D, grp[g]);
    }
  };
  uint64_t chunk_a = 0, chunk_m = 0;
  auto load_chunk = [&](int j0) {
    // the next 64 steps: lane i holds step j0 + i's own word and new word
    const int xs = dir > 0 ? j0 + lane : W - 1 - (j0 + lane);
    const int xn = dir > 0 ? xs : xs - (D - 1);
    chunk_a = A[min(max(xs, 0), W - 1)];
    chunk_m = M[min(max(xn, 0), W - 1)];
    settle(chunk_a);
    settle(chunk_m);
  };
  auto run_group = [&](int j0, auto tail) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int j = j0 + g;
      if (!decltype(tail)::value || j < W) {
        const int x = dir > 0 ? j : W - 1 - j;
        const uint64_t wa = readlane_u64(chunk_a, j & (WAVE - 1));
        const uint64_t wn = readlane_u64(chunk_m, j & (WAVE - 1));
        // move the window by one disparity
        if (dir > 0) {
          const int lo = from_lane_below((int)(uint32_t)win[K - 1], 0);
          const int hi = from_lane_below((int)(uint32_t)(win[K - 1] >> 32), 0);
#pragma unroll
          for (int k = K - 1; k > 0; --k) win[k] = win[k - 1];
          win[0] = lane == 0 ? wn : (((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
        } else {
          const int lo = from_lane_above((int)(uint32_t)win[0], 0);
          const int hi = from_lane_above((int)(uint32_t)(win[0] >> 32), 0);
#pragma unroll
          for (int k = 0; k < K - 1; ++k) win[k] = win[k + 1];
          win[K - 1] = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
#pragma unroll
          for (int k = 0; k < K; ++k)
            if (d0 + k == D - 1) win[k] = wn;
        }
        int c[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
          c[k] = x - (d0 + k) >= 0 ? __popcll(wa ^ win[k]) : COST_OUT;
        path_step<K>(L, c, d0, D, a.P1, a.P2, j == 0);
        int s[K];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = (first ? 0 : sum_of<K>(cur[g], k)) + L[k];
        store_sums<K, FULL>(S + (size_t)x * D, d0, D, s);
      }
    }
  };
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int r = 0; r < Packed<K>::R; ++r) cur[g].r[r] = nxt[g].r[r] = 0;
  }
  load_group(0, cur, Tail());
  int j0 = 0;
  for (; j0 + 2 * G <= W; j0 += G) {  // this group and the next one are whole
    if ((j0 & (WAVE - 1)) == 0) load_chunk(j0);
    load_group(j0 + G, nxt, NoTail());
    run_group(j0, NoTail());
#pragma unroll
    for (int g = 0; g < G; ++g) cur[g] = nxt[g];
  }
  for (; j0 < W; j0 += G) {
    if ((j0 & (WAVE - 1)) == 0) load_chunk(j0);
    load_group(j0 + G, nxt, Tail());
    run_group(j0, Tail());
#pragma unroll
    for (int g = 0; g < G; ++g) cur[g] = nxt[g];
  }
}

// ---------------------------------------------------------------------------
// vertical and diagonal paths: wave = (view, b, j); step t visits
// y = t (dy > 0) or H - 1 - t, x = (j + dx t) mod W.
// ---------------------------------------------------------------------------
// One step's inputs: the pixel, its own census word, the K words it is matched
// to and its K sums so far.
template <int K>
struct ColStep {
  int y, x;
  uint64_t wa, wm[K];
  Packed<K> s;
};

template <int K, bool FULL>
__global__ __launch_bounds__(TPB) void path_col_kernel(SgmArgs a, int dy, int dx) {
  constexpr int G = Group<K>::N;
  const int lane = threadIdx.x & (WAVE - 1);
  const long line = (long)blockIdx.x * WPB + (threadIdx.x >> 6);
  const long lines = 2l * a.B * a.W;
  if (line >= lines) return;
  const int H = a.H, W = a.W, D = a.D;
  const int view = (int)(line / ((long)a.B * W));
  const int b = (int)((line / W) % a.B);
  const size_t img = (size_t)b * H * W;
  const uint64_t* A = plane_a(a, view) + img;
  const uint64_t* M = plane_m(a, view) + img;
  uint16_t* S = a.S + ((size_t)view * a.B + b) * H * W * D;
  const int d0 = lane * K;

  int L[K];
#pragma unroll
  for (int k = 0; k < K; ++k) L[k] = BIG;

  // (py, px): the pixel of the next step to load, t_load its number
  int py = dy > 0 ? 0 : H - 1, px = (int)(line % W), t_load = 0;
  auto load_group = [&](ColStep<K> (&grp)[G], auto tail) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (!decltype(tail)::value || t_load < H) {
        ColStep<K>& st = grp[g];
        st.y = py;
        st.x = px;
        const size_t p = (size_t)py * W + px;
        st.wa = A[p];
#pragma unroll
        for (int k = 0; k < K; ++k) st.wm[k] = M[(size_t)py * W + max(px - (d0 + k), 0)];
        load_sums<K>(S + p * D, d0, D, st.s);
        py += dy;
        px += dx;
        if (px == W) px = 0;
        if (px < 0) px = W - 1;
        ++t_load;
      }
    }
  };

  ColStep<K> cur[G], nxt[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    cur[g].y = cur[g].x = 0;
    cur[g].wa = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) cur[g].wm[k] = 0;
#pragma unroll
    for (int r = 0; r < Packed<K>::R; ++r) cur[g].s.r[r] = 0;
    nxt[g] = cur[g];
  }
  auto run_group = [&](int t0, auto tail) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int t = t0 + g;
      if (!decltype(tail)::value || t < H) {
        ColStep<K>& st = cur[g];
        int c[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
          c[k] = st.x - (d0 + k) >= 0 ? __popcll(st.wa ^ st.wm[k]) : COST_OUT;
        // the path starts anew where the previous pixel is outside the image
        const bool start = t == 0 || (dx > 0 && st.x == 0) || (dx < 0 && st.x == W - 1);
        path_step<K>(L, c, d0, D, a.P1, a.P2, start);
        int s[K];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = sum_of<K>(st.s, k) + L[k];
        store_sums<K, FULL>(S + ((size_t)st.y * W + st.x) * D, d0, D, s);
      }
    }
  };
  load_group(cur, Tail());
  int t0 = 0;
  for (; t0 + 2 * G <= H; t0 += G) {  // this group and the next one are whole
    load_group(nxt, NoTail());         // the group after this one, while this one runs
    run_group(t0, NoTail());
#pragma unroll
    for (int g = 0; g < G; ++g) cur[g] = nxt[g];
  }
  for (; t0 < H; t0 += G) {
    load_group(nxt, Tail());
    run_group(t0, Tail());
#pragma unroll
    for (int g = 0; g < G; ++g) cur[g] = nxt[g];
  }
}

// ---------------------------------------------------------------------------
// winner: a wave per pixel of either view.
// ---------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(TPB) void winner_kernel(const uint16_t* S, size_t npix, int D,
                                                     int uniq, uint32_t* raw) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int d0l = lane * K;
  const size_t nwaves = (size_t)gridDim.x * WPB;
  for (size_t p = (size_t)blockIdx.x * WPB + (threadIdx.x >> 6); p < npix; p += nwaves) {
    const uint16_t* sp = S + p * D;
    Packed<K> packed;
    load_sums<K>(sp, d0l, D, packed);
    int s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = d0l + k < D ? sum_of<K>(packed, k) : BIG;
    // first argmin: the sum above the disparity in one key
    int key = (BIG << 8) | 255;
#pragma unroll
    for (int k = 0; k < K; ++k) key = min(key, (s[k] << 8) | (d0l + k));
    key = wave_min(key);
    const int best = key >> 8, d0 = key & 255;
    int other = BIG;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int d = d0l + k;
      if (d < d0 - 1 || d > d0 + 1) other = min(other, s[k]);
    }
    const int s2 = wave_min(other);
    if (lane == 0) {
      const bool ok = 100 * best <= uniq * s2 && d0 > 0;
      int off = 0;
      if (d0 > 0 && d0 < D - 1) {
        const int sm = sp[d0 - 1], spl = sp[d0 + 1];
        const int den = sm - 2 * best + spl;
        if (den > 0) off = (sm - spl) * 128 / den;
      }
      const uint32_t q = (uint32_t)(256 * d0 + off);
      raw[p] = q | ((uint32_t)d0 << 16) | (ok ? RAW_OK : 0u);
    }
  }
}

// ---------------------------------------------------------------------------
// left-right check and output: a thread per pixel, both views.  raw[1] is
// mirrored in x.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void lr_kernel(const uint32_t* raw, size_t n, int W, int lr_max,
                                                 uint16_t* out_left, uint16_t* out_right) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % W);
  const uint32_t* row_l = raw + (i - x);
  const uint32_t* row_r = raw + n + (i - x);
  {
    const uint32_t r = row_l[x];
    bool stay = (r & RAW_OK) != 0;
    if (stay && lr_max >= 0) {
      const int d = (r >> 16) & 255, xr = x - d;
      stay = xr >= 0;
      if (stay) {
        const uint32_t o = row_r[W - 1 - xr];
        const int diff = (int)((o >> 16) & 255) - d;
        stay = (o & RAW_OK) != 0 && diff <= lr_max && -diff <= lr_max;
      }
    }
    out_left[i] = stay ? (uint16_t)(r & 0xffffu) : (uint16_t)0;
  }
  {
    const uint32_t r = row_r[W - 1 - x];
    bool stay = (r & RAW_OK) != 0;
    if (stay && lr_max >= 0) {
      const int d = (r >> 16) & 255, xl = x + d;
      stay = xl <= W - 1;
      if (stay) {
        const uint32_t o = row_l[xl];
        const int diff = (int)((o >> 16) & 255) - d;
        stay = (o & RAW_OK) != 0 && diff <= lr_max && -diff <= lr_max;
      }
    }
    out_right[i] = stay ? (uint16_t)(r & 0xffffu) : (uint16_t)0;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// workspace: [census 4 n x 8][S 2 n D x 2][raw 2 n x 4][grey 2 n], each part
// a multiple of 16 bytes
size_t round16(size_t v) { return (v + 15) / 16 * 16; }

// Line and block counts stay below 2^31 and a pixel index below 2^28.
bool dims_ok(int32_t B, int32_t H, int32_t W, int32_t C, int32_t D, int32_t paths) {
  if (B <= 0 || H <= 0 || W <= 0) return false;
  if ((int64_t)B * H * W > (1ll << 27)) return false;
  if (C != 1 && C != 3) return false;
  if (D < 16 || D > 256 || D % 16) return false;
  return paths == 4 || paths == 8;
}

size_t census_bytes(size_t n) { return 4 * n * sizeof(uint64_t); }
size_t sum_bytes(size_t n, int D) { return 2 * n * D * sizeof(uint16_t); }
size_t raw_bytes(size_t n) { return round16(2 * n * sizeof(uint32_t)); }
size_t grey_bytes(size_t n) { return round16(2 * n); }

template <int K, bool FULL>
void launch_paths(const SgmArgs& a, int paths, hipStream_t s) {
  const long rows = 2l * a.B * a.H, cols = 2l * a.B * a.W;
  const dim3 grow((unsigned)((rows + WPB - 1) / WPB)), gcol((unsigned)((cols + WPB - 1) / WPB));
  hipLaunchKernelGGL((path_row_kernel<K, FULL>), grow, dim3(TPB), 0, s, a, 1, 1);
  hipLaunchKernelGGL((path_row_kernel<K, FULL>), grow, dim3(TPB), 0, s, a, -1, 0);
  for (int dy = 1; dy >= -1; dy -= 2)
    hipLaunchKernelGGL((path_col_kernel<K, FULL>), gcol, dim3(TPB), 0, s, a, dy, 0);
  if (paths == 8)
    for (int dy = 1; dy >= -1; dy -= 2)
      for (int dx = 1; dx >= -1; dx -= 2)
        hipLaunchKernelGGL((path_col_kernel<K, FULL>), gcol, dim3(TPB), 0, s, a, dy, dx);
}

template <int K>
void launch_winner(const uint16_t* S, size_t npix, int D, int uniq, uint32_t* raw,
                   hipStream_t s) {
  size_t blocks = (npix + WPB - 1) / WPB;
  if (blocks > 16384) blocks = 16384;  // (the waves stride over the pixels)
  hipLaunchKernelGGL(winner_kernel<K>, dim3((unsigned)blocks), dim3(TPB), 0, s, S, npix, D, uniq,
                     raw);
}

}  // namespace

extern "C" {

size_t lsi_sgm_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t D,
                               int32_t paths) {
  if (!dims_ok(B, H, W, C, D, paths)) return 0;
  const size_t n = (size_t)B * H * W;
  return census_bytes(n) + sum_bytes(n, D) + raw_bytes(n) + grey_bytes(n);
}

int lsi_sgm_disparity_u8(int32_t B, int32_t H, int32_t W, int32_t C, const uint8_t* left,
                         const uint8_t* right, int32_t D, int32_t P1, int32_t P2,
                         int32_t paths, int32_t uniq, int32_t lr_max, uint16_t* disp_left,
                         uint16_t* disp_right, void* ws, size_t ws_bytes,
                         lsi_stream_t stream) {
  if (!dims_ok(B, H, W, C, D, paths)) return LSI_EINVAL;
  if (P1 < 0 || P1 > P2 || P2 > MAX_P2 || uniq < 0 || uniq > 100) return LSI_EINVAL;
  if (!left || !right || !disp_left || !disp_right || !ws) return LSI_ENULL;
  if (ws_bytes < lsi_sgm_workspace_bytes(B, H, W, C, D, paths)) return LSI_EWORKSPACE;
  const size_t n = (size_t)B * H * W;
  char* p = (char*)ws;
  uint64_t* cen = (uint64_t*)p;
  p += census_bytes(n);
  uint16_t* S = (uint16_t*)p;
  p += sum_bytes(n, D);
  uint32_t* raw = (uint32_t*)p;
  p += raw_bytes(n);
  uint8_t* grey = (uint8_t*)p;
  hipStream_t s = (hipStream_t)stream;
  const dim3 per_pixel2((unsigned)((2 * n + TPB - 1) / TPB));
  hipLaunchKernelGGL(grey_kernel, per_pixel2, dim3(TPB), 0, s, left, right, (int)C, n, grey);
  hipLaunchKernelGGL(census_kernel, per_pixel2, dim3(TPB), 0, s, (const uint8_t*)grey, (int)B,
                     (int)H, (int)W, cen);
  SgmArgs a;
  a.B = B; a.H = H; a.W = W; a.D = D; a.P1 = P1; a.P2 = P2;
  a.cen = cen; a.S = S;
  const int K = (D + WAVE - 1) / WAVE;
  switch (D == WAVE * K ? -K : K) {  // (negative: every lane holds K disparities)
    case -1: launch_paths<1, true>(a, paths, s); break;
    case -2: launch_paths<2, true>(a, paths, s); break;
    case -3: launch_paths<3, true>(a, paths, s); break;
    case -4: launch_paths<4, true>(a, paths, s); break;
    case 1: launch_paths<1, false>(a, paths, s); break;
    case 2: launch_paths<2, false>(a, paths, s); break;
    case 3: launch_paths<3, false>(a, paths, s); break;
    default: launch_paths<4, false>(a, paths, s); break;
  }
  switch (K) {
    case 1: launch_winner<1>(S, 2 * n, D, uniq, raw, s); break;
    case 2: launch_winner<2>(S, 2 * n, D, uniq, raw, s); break;
    case 3: launch_winner<3>(S, 2 * n, D, uniq, raw, s); break;
    default: launch_winner<4>(S, 2 * n, D, uniq, raw, s); break;
  }
  hipLaunchKernelGGL(lr_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s,
                     (const uint32_t*)raw, n, (int)W, (int)lr_max, disp_left, disp_right);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
