// The triangle mesh of a layered depth image (lsi_ldi_mesh's surface) rasterised
// into V target views per item with a z-buffer (gfx950).  No reference
// counterpart; the definition is DESIGN.md section 4.25 and the header's
// comment.  Vertices are snapped to 8 sub-pixel bits and coverage is decided by
// int64 edge functions with a top-left rule; the depth and the colours are fp32
// in the stated order without contraction (explicit __f*_rn, correctly rounded
// division); the z-test is one unsigned 64-bit atomic maximum per covered
// pixel, which commutes.  So the outputs are a function of the inputs alone, bit
// for bit, whatever the order the triangles arrive in.
//
// Kernels and what bounds them (one call, in launch order):
//   clear_kernel    zeroes the keys, 8 bytes per target pixel: their write.
//   project_kernel  a thread per (view, texel): the export's existence rule
//                   (restated here, held to the same NumPy function), the
//                   projection with its three divisions and the snap; stages
//                   {X, Y, dd, d} as one 16-byte store, dd = 0 where there is no
//                   usable vertex.  Bound by that write.
//   raster_kernel   a thread per (view, texel) -- the corner a of its quad; the
//                   last row and column have none and return --, lanes along a
//                   source row so that a wave's atomics land on neighbouring
//                   target pixels: reads the quad's four staged corners (three
//                   of them re-read
//                   through L1/L2 by the neighbours), sets its two triangles up
//                   and walks their clipped boxes, at most max_extent^2 pixels
//                   each.  A key that a plain load already shows to be larger
//                   skips the atomic (keys only grow).  Bound by the atomics.
//   resolve_kernel  a thread per target pixel: decodes the winner, forms its
//                   vertices, edge functions and weights again and interpolates
//                   the colours from tex.  Bound by the write of the outputs.
// 4 launches whatever the data.  No host synchronisation, no allocation, no
// state, no LDS, plain vector stores and atomics only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int SUB = 1 << LSI_RASTER_SUBPIXEL_BITS;       // 256 sub-pixels per pixel
constexpr int HALF = SUB / 2;
constexpr int64_t MAX_TEXELS = 1ll << 28;                 // lsi_ldi_mesh's limit
constexpr int CLEAR_GRID_MAX = 1 << 16;

static_assert(LSI_RASTER_SUBPIXEL_BITS == 8, "the snap multiplies by 256");

struct RasterArgs {
  const float* tex;
  const float* mask;        // NULL: every texel passes
  const float* disp;
  const float* M;           // B V x 16
  float* img;
  float* cov;
  float* out_disp;          // NULL: not wanted
  unsigned long long* keys; // B V x Ht Wt
  int4* stage;              // B V x N: {X, Y, bits(dd), bits(d)}
  int64_t n_keys;           // B V Ht Wt
  int32_t L, H, W, V;
  int32_t N;                // L H W
  int32_t Ht, Wt;
  int32_t max_extent;
  int64_t tex_sl, tex_sb, tex_sy, tex_sx, tex_sc;
  int64_t disp_sl, disp_sb, disp_sy, disp_sx;
  int64_t mask_sl, mask_sb, mask_sy, mask_sx;
  float disp_min, mask_min, edge_ratio, merge_ratio;
  float bg_value;
  int32_t cull;
};

struct Texel {
  int l, y, x;
};

__device__ __forceinline__ Texel texel_of(const RasterArgs& a, int n) {
  Texel t;
  const int row = n / a.W;
  t.x = n - row * a.W;
  t.l = row / a.H;
  t.y = row - t.l * a.H;
  return t;
}

__device__ __forceinline__ float disp_at(const RasterArgs& a, int b, int l, int y, int x) {
  return a.disp[l * a.disp_sl + b * a.disp_sb + y * a.disp_sy + x * a.disp_sx];
}

// finite and at least disp_min (a NaN fails both compares)
__device__ __forceinline__ bool in_range(const RasterArgs& a, float d) {
  return d >= a.disp_min && d <= 3.402823466e+38f;
}

// lsi_ldi_mesh's existence rule; *d is the texel's disparity.
__device__ __forceinline__ bool vertex_exists(const RasterArgs& a, int b, int l, int y, int x,
                                              float* d) {
  const float v = disp_at(a, b, l, y, x);
  *d = v;
  if (!in_range(a, v)) return false;
  if (a.mask) {
    const float m = a.mask[l * a.mask_sl + b * a.mask_sb + y * a.mask_sy + x * a.mask_sx];
    if (!(m > a.mask_min)) return false;
  }
  if (a.merge_ratio > 0.0f && l > 0) {
    const float f = disp_at(a, b, l - 1, y, x);
    if (in_range(a, f) && v >= __fmul_rn(a.merge_ratio, f)) return false;   // merged
  }
  return true;
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

__global__ __launch_bounds__(TPB) void clear_kernel(RasterArgs a) {
  const int64_t step = (int64_t)gridDim.x * TPB;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < a.n_keys; i += step)
    a.keys[i] = 0ull;
}

__global__ __launch_bounds__(TPB) void project_kernel(RasterArgs a) {
  const int bv = blockIdx.y, n = blockIdx.x * TPB + threadIdx.x;
  if (n >= a.N) return;
  const Texel t = texel_of(a, n);
  float d;
  int4 rec = make_int4(0, 0, 0, 0);
  if (vertex_exists(a, bv / a.V, t.l, t.y, t.x, &d)) {
    const float* m = a.M + 16 * (int64_t)bv;
    const float px = (float)t.x + 0.5f, py = (float)t.y + 0.5f;
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      q[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(px, m[4 * j]), __fmul_rn(py, m[4 * j + 1])),
                                 m[4 * j + 2]),
                       __fmul_rn(d, m[4 * j + 3]));
    const float nn = q[2];
    const float u = __fdiv_rn(q[0], nn), v = __fdiv_rn(q[1], nn), dd = __fdiv_rn(q[3], nn);
    const float guard = (float)LSI_RASTER_GUARD;
    if (finite(u) && finite(v) && finite(dd) && nn > 0.0f && dd > 0.0f && fabsf(u) <= guard &&
        fabsf(v) <= guard)
      rec = make_int4((int)rintf(__fmul_rn(u, (float)SUB)), (int)rintf(__fmul_rn(v, (float)SUB)),
                      __float_as_int(dd), __float_as_int(d));
  }
  a.stage[(int64_t)bv * a.N + n] = rec;
}

// A triangle set up for a view: vertices in the order coverage uses (A > 0).
struct Tri {
  int64_t X[3], Y[3];
  float dd[3];
  int64_t A;
  int i0, i1, j0, j1;       // the clipped box of pixels, inclusive
  bool swapped;             // vertices 1 and 2 exchanged
};

// false: no triangle under this view (a missing vertex, the cut, A == 0, culled,
// an empty or too large box).  p0, p1, p2 in the export's order.
__device__ __forceinline__ bool setup(const RasterArgs& a, const int4& p0, const int4& p1,
                                      const int4& p2, Tri* t) {
  if (p0.z == 0 || p1.z == 0 || p2.z == 0) return false;     // (dd > 0 has non-zero bits)
  const float d0 = __int_as_float(p0.w), d1 = __int_as_float(p1.w), d2 = __int_as_float(p2.w);
  const float lo = fminf(fminf(d0, d1), d2), hi = fmaxf(fmaxf(d0, d1), d2);
  if (!(lo >= __fmul_rn(a.edge_ratio, hi))) return false;
  const int64_t A = (int64_t)(p1.x - p0.x) * (p2.y - p0.y) - (int64_t)(p1.y - p0.y) * (p2.x - p0.x);
  if (A == 0) return false;
  if (A > 0 && a.cull) return false;                          // seen from behind
  t->swapped = A < 0;
  const int4& v1 = t->swapped ? p2 : p1;
  const int4& v2 = t->swapped ? p1 : p2;
  t->A = A < 0 ? -A : A;
  t->X[0] = p0.x, t->X[1] = v1.x, t->X[2] = v2.x;
  t->Y[0] = p0.y, t->Y[1] = v1.y, t->Y[2] = v2.y;
  t->dd[0] = __int_as_float(p0.z), t->dd[1] = __int_as_float(v1.z);
  t->dd[2] = __int_as_float(v2.z);
  const int xlo = min(min(p0.x, p1.x), p2.x), xhi = max(max(p0.x, p1.x), p2.x);
  const int ylo = min(min(p0.y, p1.y), p2.y), yhi = max(max(p0.y, p1.y), p2.y);
  t->i0 = max((xlo + HALF - 1) >> LSI_RASTER_SUBPIXEL_BITS, 0);
  t->i1 = min((xhi - HALF) >> LSI_RASTER_SUBPIXEL_BITS, a.Wt - 1);
  t->j0 = max((ylo + HALF - 1) >> LSI_RASTER_SUBPIXEL_BITS, 0);
  t->j1 = min((yhi - HALF) >> LSI_RASTER_SUBPIXEL_BITS, a.Ht - 1);
  if (t->i0 > t->i1 || t->j0 > t->j1) return false;
  return t->i1 - t->i0 < a.max_extent && t->j1 - t->j0 < a.max_extent;
}

// Edge functions of pixel (i, j); false when it is outside.
__device__ __forceinline__ bool edges(const Tri& t, int i, int j, int64_t E[3]) {
  const int64_t px = (int64_t)i * SUB + HALF, py = (int64_t)j * SUB + HALF;
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ka = (k + 1) % 3, kb = (k + 2) % 3;
    const int64_t dx = t.X[kb] - t.X[ka], dy = t.Y[kb] - t.Y[ka];
    E[k] = dx * (py - t.Y[ka]) - dy * (px - t.X[ka]);
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    inside = inside && (E[k] > 0 || (E[k] == 0 && top_left));
  }
  return inside;
}

__device__ __forceinline__ void weights(const Tri& t, const int64_t E[3], float b[3]) {
  const float fa = (float)t.A;
  b[1] = __fdiv_rn((float)E[1], fa);
  b[2] = __fdiv_rn((float)E[2], fa);
  b[0] = __fsub_rn(__fsub_rn(1.0f, b[1]), b[2]);
}

__device__ __forceinline__ float blend(const float b[3], float c0, float c1, float c2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(b[0], c0), __fmul_rn(b[1], c1)), __fmul_rn(b[2], c2));
}

__device__ __forceinline__ void raster_triangle(const RasterArgs& a, unsigned long long* keys,
                                                const int4& p0, const int4& p1, const int4& p2,
                                                uint32_t id) {
  Tri t;
  if (!setup(a, p0, p1, p2, &t)) return;
  const unsigned long long low = 0xFFFFFFFFull - id;
  for (int j = t.j0; j <= t.j1; ++j) {
    for (int i = t.i0; i <= t.i1; ++i) {
      int64_t E[3];
      if (!edges(t, i, j, E)) continue;
      float b[3];
      weights(t, E, b);
      const float z = blend(b, t.dd[0], t.dd[1], t.dd[2]);
      if (!(z > 0.0f && finite(z))) continue;
      const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | low;
      unsigned long long* p = keys + (int64_t)j * a.Wt + i;
      if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) continue;
      (void)__hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(TPB) void raster_kernel(RasterArgs a) {
  const int bv = blockIdx.y, n = blockIdx.x * TPB + threadIdx.x;
  if (n >= a.N) return;
  const Texel t = texel_of(a, n);
  if (t.y >= a.H - 1 || t.x >= a.W - 1) return;
  const int4* s = a.stage + (int64_t)bv * a.N + n;
  const int4 vb = s[1], vc = s[a.W];
  if (vb.z == 0 || vc.z == 0) return;                         // both triangles hold b and c
  const int4 va = s[0], vd = s[a.W + 1];
  unsigned long long* keys = a.keys + (int64_t)bv * a.Ht * a.Wt;
  raster_triangle(a, keys, va, vc, vb, 2u * (uint32_t)n);
  raster_triangle(a, keys, vb, vc, vd, 2u * (uint32_t)n + 1u);
}

__global__ __launch_bounds__(TPB) void resolve_kernel(RasterArgs a) {
  const int bv = blockIdx.y, p = blockIdx.x * TPB + threadIdx.x;
  if (p >= a.Ht * a.Wt) return;
  const int64_t o = (int64_t)bv * a.Ht * a.Wt + p;
  const unsigned long long key = a.keys[o];
  float c[3] = {a.bg_value, a.bg_value, a.bg_value}, cov = 0.0f, z = 0.0f;
  if (key != 0ull) {
    const uint32_t id = 0xFFFFFFFFu - (uint32_t)key;
    const int n = (int)(id >> 1), b = bv / a.V;
    const bool second = (id & 1u) != 0u;
    const Texel q = texel_of(a, n);
    const int4* s = a.stage + (int64_t)bv * a.N + n;
    // the export's order: (a, c, b) or (b, c, d), and where their texels are
    const int4 p0 = second ? s[1] : s[0], p1 = s[a.W], p2 = second ? s[a.W + 1] : s[1];
    const int x0 = q.x + (second ? 1 : 0), y0 = q.y;
    const int x1 = q.x, y1 = q.y + 1;
    const int x2 = q.x + 1, y2 = q.y + (second ? 1 : 0);
    Tri t;
    int64_t E[3];
    float w[3];
    const int j = p / a.Wt, i = p - j * a.Wt;
    // (the winner passed both once: only their values are wanted here)
    (void)setup(a, p0, p1, p2, &t);
    (void)edges(t, i, j, E);
    weights(t, E, w);
    const float* base = a.tex + (q.l * a.tex_sl + b * a.tex_sb);
    const float* c0 = base + (y0 * a.tex_sy + x0 * a.tex_sx);
    const float* c1 = base + (t.swapped ? y2 * a.tex_sy + x2 * a.tex_sx
                                        : y1 * a.tex_sy + x1 * a.tex_sx);
    const float* c2 = base + (t.swapped ? y1 * a.tex_sy + x1 * a.tex_sx
                                        : y2 * a.tex_sy + x2 * a.tex_sx);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = blend(w, c0[k * a.tex_sc], c1[k * a.tex_sc], c2[k * a.tex_sc]);
    cov = 1.0f;
    z = __uint_as_float((uint32_t)(key >> 32));
  }
  a.img[3 * o] = c[0], a.img[3 * o + 1] = c[1], a.img[3 * o + 2] = c[2];
  a.cov[o] = cov;
  if (a.out_disp) a.out_disp[o] = z;
}

bool ratio_ok(float r) { return r >= 0.0f && r <= 1.0f; }   // (a NaN fails)

// The plan of a descriptor; false for one the call refuses.
bool plan(const LsiRasterDesc* d, RasterArgs* a) {
  if (!d) return false;
  if (d->L < 1 || d->B < 1 || d->B > 65535 || d->H < 1 || d->W < 1) return false;
  const int64_t n = (int64_t)d->L * d->H * d->W;
  if ((int64_t)d->L * d->H > MAX_TEXELS || n > MAX_TEXELS) return false;
  const int64_t strides[] = {d->tex_sl, d->tex_sb, d->tex_sy, d->tex_sx, d->tex_sc,
                             d->disp_sl, d->disp_sb, d->disp_sy, d->disp_sx,
                             d->mask_sl, d->mask_sb, d->mask_sy, d->mask_sx};
  for (int64_t s : strides)
    if (s < 0) return false;
  if (!(isfinite(d->disp_min) && d->disp_min > 0.0f) || !isfinite(d->mask_min)) return false;
  if (!ratio_ok(d->edge_ratio) || !ratio_ok(d->merge_ratio)) return false;
  if (d->V < 1 || d->V > LSI_RASTER_MAX_VIEWS || (int64_t)d->B * d->V > 65535) return false;
  if (d->Ht < 1 || d->Ht > LSI_RASTER_MAX_SIZE || d->Wt < 1 || d->Wt > LSI_RASTER_MAX_SIZE)
    return false;
  if (d->max_extent < 1 || d->max_extent > LSI_RASTER_MAX_EXTENT) return false;
  if (!isfinite(d->bg_value)) return false;
  if ((d->flags & ~LSI_RASTER_CULL_BACK) != 0 || d->reserved != 0) return false;
  a->L = d->L, a->H = d->H, a->W = d->W, a->V = d->V, a->N = (int32_t)n;
  a->Ht = d->Ht, a->Wt = d->Wt, a->max_extent = d->max_extent;
  a->n_keys = (int64_t)d->B * d->V * d->Ht * d->Wt;
  a->tex_sl = d->tex_sl, a->tex_sb = d->tex_sb, a->tex_sy = d->tex_sy, a->tex_sx = d->tex_sx;
  a->tex_sc = d->tex_sc;
  a->disp_sl = d->disp_sl, a->disp_sb = d->disp_sb, a->disp_sy = d->disp_sy;
  a->disp_sx = d->disp_sx;
  a->mask_sl = d->mask_sl, a->mask_sb = d->mask_sb, a->mask_sy = d->mask_sy;
  a->mask_sx = d->mask_sx;
  a->disp_min = d->disp_min, a->mask_min = d->mask_min;
  a->edge_ratio = d->edge_ratio, a->merge_ratio = d->merge_ratio;
  a->bg_value = d->bg_value;
  a->cull = (d->flags & LSI_RASTER_CULL_BACK) != 0;
  return true;
}

// bytes of the keys of all views, a multiple of 16: the staged vertices follow
size_t key_bytes(const RasterArgs& a) {
  return ((size_t)a.n_keys * sizeof(unsigned long long) + 15) / 16 * 16;
}

}  // namespace

extern "C" {

size_t lsi_ldi_raster_workspace_bytes(const LsiRasterDesc* desc) {
  RasterArgs a;
  if (!plan(desc, &a)) return 0;
  return key_bytes(a) + (size_t)desc->B * (size_t)desc->V * (size_t)a.N * sizeof(int4);
}

int lsi_ldi_raster(const LsiRasterDesc* desc, const float* tex, const float* mask,
                   const float* disp, const float* M, float* img, float* cov,
                   float* out_disp, void* workspace, size_t workspace_bytes,
                   lsi_stream_t stream) {
  RasterArgs a;
  if (!plan(desc, &a)) return LSI_EINVAL;
  if (((uintptr_t)tex & 3) || ((uintptr_t)mask & 3) || ((uintptr_t)disp & 3) ||
      ((uintptr_t)M & 3) || ((uintptr_t)img & 3) || ((uintptr_t)cov & 3) ||
      ((uintptr_t)out_disp & 3) || ((uintptr_t)workspace & 15))
    return LSI_EINVAL;
  if (!tex || !disp || !M || !img || !cov || !workspace) return LSI_ENULL;
  if (workspace_bytes < lsi_ldi_raster_workspace_bytes(desc)) return LSI_EWORKSPACE;
  a.tex = tex, a.mask = mask, a.disp = disp, a.M = M;
  a.img = img, a.cov = cov, a.out_disp = out_disp;
  a.keys = static_cast<unsigned long long*>(workspace);
  a.stage = reinterpret_cast<int4*>(static_cast<uint8_t*>(workspace) + key_bytes(a));
  hipStream_t s = (hipStream_t)stream;
  const int views = desc->B * desc->V;
  const int64_t clear_groups = (a.n_keys + TPB - 1) / TPB;
  const dim3 texels((a.N + TPB - 1) / TPB, views);
  const dim3 pixels((a.Ht * a.Wt + TPB - 1) / TPB, views);
  hipLaunchKernelGGL(clear_kernel, dim3((unsigned)(clear_groups < CLEAR_GRID_MAX ? clear_groups
                                                                                 : CLEAR_GRID_MAX)),
                     dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(project_kernel, texels, dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(raster_kernel, texels, dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(resolve_kernel, pixels, dim3(TPB), 0, s, a);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
