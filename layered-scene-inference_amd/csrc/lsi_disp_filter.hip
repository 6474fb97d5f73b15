// Post-filters for 16-bit disparity maps on the device (gfx950): a 3 x 3 median
// over the valid values and the removal of small connected components
// ("speckles").  The maps are disparity * 256 with 0 for "no match", what
// lsi_sgm_disparity_u8 writes.  No reference counterpart; the definition is
// DESIGN.md section 4.18 and the header's comment.  Everything is integer
// arithmetic and components are unique (the link relation is symmetric), so the
// result is a function of the input alone, whatever order the unions happen in.
//
// Kernels and what bounds them (one call, in launch order):
//   median3_kernel   a thread per pixel: 9 cached loads, the element of rank
//                    (n - 1) / 2 among the n valid ones by counting; launch
//                    latency.
//   tile_kernel      a workgroup per TILE x TILE tile, labelled entirely in LDS:
//                    a pixel starts with the first pixel of its horizontal run
//                    as label (one wave ballot per row, no loop), vertical links
//                    are united with LDS atomicMin, a run adds its length to its
//                    root's count.  Writes, per pixel, the global index of its
//                    tile-local root (`parent`) and, at every tile-local root,
//                    the component's pixel count inside the tile (`size`; 0 at
//                    every other pixel).
//   border_kernel    a thread per pixel pair across a tile edge: a lock-free
//                    union of the two roots in `parent`.  Every read there is an
//                    agent-scope relaxed atomic load and every write an
//                    agent-scope atomicMin (another workgroup's plain store or a
//                    cached line could be stale: the XCDs' L2s are not coherent);
//                    labels only ever decrease, so every loop ends; nobody waits
//                    for anybody.  A pair that the previous pair of the same edge
//                    already bridges is skipped (one union per stretch of
//                    linked pairs: 75 -> 15 us on a matcher's two KITTI maps).
//                    Bound by the latency of the chains it walks.
//   flatten_kernel   a thread per pixel; only tile-local roots act: they find
//                    their global root, add their tile count to its size with
//                    ONE atomicAdd and point at it directly.  (A component that
//                    covers the image costs an add per tile, not per pixel.)
//   apply_kernel     a thread per pixel: root, size, store the value or 0.
// 4 launches for the speckle stage, 1 for the median, a device copy when both
// are off.  No host synchronisation, no allocation, no state, plain vector
// stores and atomics only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int TILE = 32;                 // a tile row is half a wave
constexpr int TILE_PIX = TILE * TILE;
constexpr int ROWS_PER_PASS = TPB / TILE;        // 8
constexpr int PASSES = TILE / ROWS_PER_PASS;     // 4 pixels per thread
constexpr int64_t MAX_PIXELS = 1ll << 27;

__device__ __forceinline__ bool linked(int a, int b, int range) {
  const int d = a > b ? a - b : b - a;
  return a != 0 && b != 0 && d <= range;
}

// ---------------------------------------------------------------------------
// the median
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void median3_kernel(const uint16_t* __restrict__ in, int n,
                                                      int H, int W, uint16_t* __restrict__ out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int centre = in[i];
  if (centre == 0) {
    out[i] = 0;
    return;
  }
  const int x = i % W, y = (i / W) % H;
  int v[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int dy = k / 3 - 1, dx = k % 3 - 1;
    const bool inside = y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W;
    v[k] = inside ? (int)in[i + dy * W + dx] : 0;
  }
  int count = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) count += v[k] != 0;
  const int want = (count - 1) / 2;     // the lower median's rank
  int res = centre;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    int rank = 0;                       // valid values in front of v[k], ties by position
#pragma unroll
    for (int j = 0; j < 9; ++j)
      rank += v[j] != 0 && (v[j] < v[k] || (v[j] == v[k] && j < k));
    if (v[k] != 0 && rank == want) res = v[k];
  }
  out[i] = (uint16_t)res;
}

// ---------------------------------------------------------------------------
// labelling inside a tile (LDS)
// ---------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lds_find(int* lab, int x) {
  for (;;) {
    const int p = lds_load(lab + x);
    if (p == x) return x;
    x = p;
  }
}

// Labels only decrease: a failed atomicMin hands back a smaller ancestor.
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  for (;;) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(TPB) void tile_kernel(const uint16_t* __restrict__ src, int H, int W,
                                                   int tiles_y, int tiles_x, int range,
                                                   int* __restrict__ parent,
                                                   int* __restrict__ size) {
  __shared__ int val[TILE_PIX];
  __shared__ int lab[TILE_PIX];
  __shared__ int cnt[TILE_PIX];
  const int bid = blockIdx.x;
  const int tile_x = bid % tiles_x, tile_y = (bid / tiles_x) % tiles_y;
  const int b = bid / tiles_x / tiles_y;
  const int x0 = tile_x * TILE, y0 = tile_y * TILE;
  const int base = b * H * W;            // (B H W <= 2^27)
  const int tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
  const bool col_in = x0 + tx < W;

#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ry = ty + k * ROWS_PER_PASS, i = ry * TILE + tx;
    const bool inside = col_in && y0 + ry < H;
    val[i] = inside ? (int)src[base + (y0 + ry) * W + x0 + tx] : 0;
    cnt[i] = 0;
  }
  __syncthreads();

  // Horizontal runs: bit x of a row's mask says that x is linked to x - 1; a
  // pixel's label is the first pixel of its run.  The first pixel also keeps
  // the run's length.
  int run_len[PASSES];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ry = ty + k * ROWS_PER_PASS, i = ry * TILE + tx;
    const bool left = tx > 0 && linked(val[i], val[i - 1], range);
    const uint64_t both = __ballot(left);          // two tile rows per wave
    const uint32_t m = (uint32_t)(both >> (threadIdx.x & 32));
    const uint32_t upto = ~m & (0xffffffffu >> (31 - tx));   // bit 0 is always set
    const int start = 31 - __clz((int)upto);
    // the run ends in front of the next clear bit above tx (bit 32: the tile's edge)
    const uint64_t above = ((uint64_t)(~m) | (1ull << 32)) >> (tx + 1);
    const int end = tx + (__ffsll((unsigned long long)above) - 1);
    lab[i] = ry * TILE + start;
    run_len[k] = start == tx ? end - start + 1 : 0;
  }
  __syncthreads();

  // Vertical links.  A link whose left neighbours already form the same bridge
  // (left, up-left and the link between them) adds nothing.
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ry = ty + k * ROWS_PER_PASS, i = ry * TILE + tx;
    if (ry == 0 || !linked(val[i], val[i - TILE], range)) continue;
    if (tx > 0 && linked(val[i], val[i - 1], range) &&
        linked(val[i - 1], val[i - 1 - TILE], range) &&
        linked(val[i - TILE], val[i - 1 - TILE], range))
      continue;
    lds_union(lab, i, i - TILE);
  }
  __syncthreads();

  int root[PASSES];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ry = ty + k * ROWS_PER_PASS, i = ry * TILE + tx;
    root[k] = lds_find(lab, i);
    if (run_len[k] > 0 && val[i] != 0) atomicAdd(&cnt[root[k]], run_len[k]);
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ry = ty + k * ROWS_PER_PASS, i = ry * TILE + tx;
    if (!col_in || y0 + ry >= H) continue;
    const int g = base + (y0 + ry) * W + x0 + tx;
    const int r = root[k];
    parent[g] = base + (y0 + r / TILE) * W + x0 + r % TILE;
    size[g] = r == i ? cnt[i] : 0;      // (an invalid pixel is its own root with count 0)
  }
}

// ---------------------------------------------------------------------------
// merging across tile edges (global memory, lock-free)
// ---------------------------------------------------------------------------
__device__ __forceinline__ int agent_load(int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int agent_min(int* p, int v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x.  On the way every visited entry is lowered to its
// grandparent (path halving by atomicMin: an entry only ever moves to an
// ancestor, and ancestors have smaller indices).
__device__ __forceinline__ int agent_find(int* parent, int x) {
  int p = agent_load(parent + x);
  while (p != x) {
    const int g = agent_load(parent + p);
    if (g == p) return p;
    agent_min(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void agent_union(int* parent, int a, int b) {
  for (;;) {
    a = agent_find(parent, a);
    b = agent_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = agent_min(parent + a, b);   // a was a root iff old == a
    if (old == a) return;
    a = old;
  }
}

// Pairs [0, n_rows): (y - 1, x), (y, x) for the tile rows y = TILE, 2 TILE, ...;
// pairs [n_rows, n_rows + n_cols): (y, x - 1), (y, x) for the tile columns.
__global__ __launch_bounds__(TPB) void border_kernel(const uint16_t* __restrict__ src, int H,
                                                     int W, int tiles_y, int tiles_x,
                                                     uint32_t n_rows, uint32_t n_cols, int range,
                                                     int* parent) {
  uint32_t idx = blockIdx.x * (uint32_t)TPB + threadIdx.x;
  int a, c, back;     // back: the step to the previous pair along the edge, 0 at a tile's first
  if (idx < n_rows) {
    const int x = idx % W;
    const uint32_t r = idx / W;
    const int k = r % (tiles_y - 1), b = r / (tiles_y - 1);
    a = b * H * W + ((k + 1) * TILE - 1) * W + x;
    c = a + W;
    back = x % TILE ? 1 : 0;
  } else {
    idx -= n_rows;
    if (idx >= n_cols) return;
    const int y = idx % H;
    const uint32_t r = idx / H;
    const int k = r % (tiles_x - 1), b = r / (tiles_x - 1);
    a = b * H * W + y * W + (k + 1) * TILE - 1;
    c = a + 1;
    back = y % TILE ? W : 0;
  }
  const int va = src[a], vc = src[c];
  if (!linked(va, vc, range)) return;
  // The previous pair of the same two tiles already joins these components if
  // it is linked itself and to this pair on both sides: one union per stretch
  // of such pairs, not one per pixel.
  if (back) {
    const int pa = src[a - back], pc = src[c - back];
    if (linked(pa, pc, range) && linked(va, pa, range) && linked(vc, pc, range)) return;
  }
  agent_union(parent, a, c);
}

// Tile-local roots (size > 0) that are not global roots hand their count to the
// global root and point at it.  Nobody adds to a non-root's size, and a global
// root does not read its own, so no add races with a read.
__global__ __launch_bounds__(TPB) void flatten_kernel(int n, int* parent, int* size) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int own = size[i];
  if (own == 0) return;
  int r = agent_load(parent + i);
  if (r == i) return;
  for (;;) {                           // (read only: halving on the way was measured slower)
    const int p = agent_load(parent + r);
    if (p == r) break;
    r = p;
  }
  atomicAdd(size + r, own);
  agent_min(parent + i, r);
}

__global__ __launch_bounds__(TPB) void apply_kernel(const uint16_t* __restrict__ src, int n,
                                                    const int* __restrict__ parent,
                                                    const int* __restrict__ size,
                                                    int speckle_size, uint16_t* __restrict__ out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint16_t v = src[i];
  if (v == 0) {
    out[i] = 0;
    return;
  }
  int r = parent[i];                   // the tile-local root, then (at most) the global one
  for (;;) {
    const int p = parent[r];
    if (p == r) break;
    r = p;
  }
  out[i] = size[r] <= speckle_size ? (uint16_t)0 : v;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
size_t round16(size_t v) { return (v + 15) / 16 * 16; }

bool args_ok(int32_t B, int32_t H, int32_t W, int32_t median, int32_t speckle_size) {
  if (B <= 0 || H <= 0 || W <= 0) return false;
  if ((int64_t)B * H * W > MAX_PIXELS) return false;
  if (median != 0 && median != 3) return false;
  return speckle_size >= 0 && speckle_size <= MAX_PIXELS;
}

}  // namespace

extern "C" {

size_t lsi_disparity_filter_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t median,
                                            int32_t speckle_size) {
  if (!args_ok(B, H, W, median, speckle_size) || speckle_size == 0) return 0;
  const size_t n = (size_t)B * H * W;
  return 8 * n + (median == 3 ? round16(2 * n) : 0);
}

int lsi_disparity_filter_u16(int32_t B, int32_t H, int32_t W, const uint16_t* in, uint16_t* out,
                             int32_t median, int32_t speckle_size, int32_t speckle_range,
                             void* ws, size_t ws_bytes, lsi_stream_t stream) {
  if (!args_ok(B, H, W, median, speckle_size)) return LSI_EINVAL;
  if (speckle_range < 0 || speckle_range > 65535) return LSI_EINVAL;
  if (in && out == in) return LSI_EINVAL;
  const size_t need = lsi_disparity_filter_workspace_bytes(B, H, W, median, speckle_size);
  if (!in || !out || (need > 0 && !ws)) return LSI_ENULL;
  if (ws_bytes < need) return LSI_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int n = B * H * W;
  const dim3 per_pixel((unsigned)((n + TPB - 1) / TPB));
  if (median == 0 && speckle_size == 0) {
    if (hipMemcpyAsync(out, in, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToDevice, s) !=
        hipSuccess)
      return LSI_ELAUNCH;
    return LSI_OK;
  }
  int* parent = (int*)ws;
  int* size = parent + n;
  const uint16_t* src = in;
  if (median == 3) {
    uint16_t* dst = speckle_size > 0 ? (uint16_t*)(size + n) : out;
    hipLaunchKernelGGL(median3_kernel, per_pixel, dim3(TPB), 0, s, in, n, (int)H, (int)W, dst);
    src = dst;
  }
  if (speckle_size > 0) {
    const int tiles_y = (H + TILE - 1) / TILE, tiles_x = (W + TILE - 1) / TILE;
    // (at most 2^27 tiles and 2^28 pairs)
    hipLaunchKernelGGL(tile_kernel, dim3((unsigned)(B * tiles_y * tiles_x)), dim3(TPB), 0, s, src,
                       (int)H, (int)W, tiles_y, tiles_x, (int)speckle_range, parent, size);
    const uint32_t n_rows = (uint32_t)B * (tiles_y - 1) * W;
    const uint32_t n_cols = (uint32_t)B * (tiles_x - 1) * H;
    if (n_rows + n_cols > 0)
      hipLaunchKernelGGL(border_kernel, dim3((n_rows + n_cols + TPB - 1) / TPB), dim3(TPB), 0, s,
                         src, (int)H, (int)W, tiles_y, tiles_x, n_rows, n_cols,
                         (int)speckle_range, parent);
    hipLaunchKernelGGL(flatten_kernel, per_pixel, dim3(TPB), 0, s, n, parent, size);
    hipLaunchKernelGGL(apply_kernel, per_pixel, dim3(TPB), 0, s, src, n, (const int*)parent,
                       (const int*)size, (int)speckle_size, out);
  }
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
