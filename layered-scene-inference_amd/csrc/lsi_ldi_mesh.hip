// A layered depth image as a textured triangle mesh, packed on the device as
// the vertex and face records of a binary little-endian PLY file (gfx950).  No
// reference counterpart; the definition is DESIGN.md section 4.24 and the
// header's comment.  All arithmetic is fp32 in the stated order without
// contraction (explicit __f*_rn, correctly rounded division), there are no
// atomics and every byte has one writer, so the output is a function of the
// input alone, bit for bit.
//
// A workgroup owns CHUNK = 256 consecutive texels of one item in the order
// (l, y, x), a thread one texel and the two triangles of the quad whose corner
// `a` it is.  Vertices and faces are numbered in that order, so a record's
// number is (records of the item's earlier workgroups) + (records of earlier
// threads of its workgroup): an exclusive scan of the workgroup totals, and a
// ballot with a population count of the lower lanes plus wave offsets in LDS.
//
// Kernels and what bounds them (one call, in launch order):
//   count_kernel   classifies its texel and the three other corners of its quad
//                  (disparity, mask and the layer in front, re-read through
//                  L1/L2 by the neighbours), writes {vertices, faces} of the
//                  workgroup.  Bound by the one read of disp and mask.
//   scan_kernel    a workgroup per item: exclusive scan of the item's workgroup
//                  totals in trips of SCAN_TRIP = 256 with a carry, in place;
//                  writes counts[b].  8 bytes per 256 texels: launch latency.
//   vertex_kernel  classifies its texel again, ranks it, writes its compact
//                  number (-1: none) to the index map and, below the capacity,
//                  its 16-byte record as one store.  Bound by the read of tex
//                  and disp and the write of records and map.
//   face_kernel    reads the quad's four map entries and the disparities of
//                  those that exist, ranks its triangles, stages the
//                  workgroup's 13-byte records in LDS at the byte phase of
//                  their place in the buffer and stores that contiguous byte
//                  range as aligned dwords; at most three bytes at either end
//                  go out as single bytes.  Bound by the write of the records.
// 4 launches whatever the data; 3 with a face capacity of 0 (face_kernel has
// nothing it may write).  No host synchronisation, no allocation, no state,
// plain vector stores only.
//
// LDS: 2 x 4 wave totals, and in face_kernel 2 CHUNK 13 + 3 bytes (6.5 KB).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int TPB = LSI_MESH_CHUNK;               // 256: a thread per texel
constexpr int WAVES = TPB / 64;
constexpr int TRIP = LSI_MESH_SCAN_TRIP;          // totals per trip of scan_kernel
constexpr int VB = LSI_MESH_VERTEX_BYTES;         // 16
constexpr int FB = LSI_MESH_FACE_BYTES;           // 13
// texels per item: vertex numbers, face numbers (< 2 N) and a workgroup's dword
// index into an item's face bytes (< 2 N 13 / 4) all stay below 2^31
constexpr int64_t MAX_TEXELS = 1ll << 28;
constexpr int64_t MAX_CAPACITY = 1ll << 29;

static_assert(TPB == 256 && TRIP == TPB && VB == 16 && FB == 13, "record and chunk sizes");

struct MeshArgs {
  const float* tex;
  const float* mask;        // NULL: every texel passes
  const float* disp;
  const float* kinv;        // B x 9
  uint8_t* vbuf;
  uint8_t* fbuf;
  int32_t* counts;          // B x 2
  int2* totals;             // B x G: {vertices, faces} per workgroup, then their scan
  int32_t* map;             // B x N: compact vertex number or -1
  int32_t L, H, W;
  int32_t N;                // L H W
  int32_t G;                // workgroups per item
  int32_t vcap, fcap;
  int64_t tex_sl, tex_sb, tex_sy, tex_sx, tex_sc;
  int64_t disp_sl, disp_sb, disp_sy, disp_sx;
  int64_t mask_sl, mask_sb, mask_sy, mask_sx;
  float disp_min, mask_min, edge_ratio, merge_ratio;
  int32_t flip;
};

struct Texel {
  int l, y, x;
};

__device__ __forceinline__ Texel texel_of(const MeshArgs& a, int n) {
  Texel t;
  const int row = n / a.W;
  t.x = n - row * a.W;
  t.l = row / a.H;
  t.y = row - t.l * a.H;
  return t;
}

__device__ __forceinline__ float disp_at(const MeshArgs& a, int b, int l, int y, int x) {
  return a.disp[l * a.disp_sl + b * a.disp_sb + y * a.disp_sy + x * a.disp_sx];
}

// finite and at least disp_min (a NaN fails both compares)
__device__ __forceinline__ bool in_range(const MeshArgs& a, float d) {
  return d >= a.disp_min && d <= 3.402823466e+38f;
}

// Does the vertex (l, y, x) exist; *d is its disparity.
__device__ __forceinline__ bool vertex_exists(const MeshArgs& a, int b, int l, int y, int x,
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

// The discontinuity cut of a triangle whose three vertices exist.
__device__ __forceinline__ bool edge_ok(const MeshArgs& a, float d0, float d1, float d2) {
  const float lo = fminf(fminf(d0, d1), d2), hi = fmaxf(fmaxf(d0, d1), d2);
  return lo >= __fmul_rn(a.edge_ratio, hi);
}

__device__ __forceinline__ int lower_lanes(uint64_t ballot) {
  const int lane = threadIdx.x & 63;
  return __popcll(ballot & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(TPB) void count_kernel(MeshArgs a) {
  __shared__ int s_v[WAVES], s_f[WAVES];
  const int b = blockIdx.y, n = blockIdx.x * TPB + threadIdx.x;
  bool ea = false, t0 = false, t1 = false;
  if (n < a.N) {
    const Texel t = texel_of(a, n);
    float da, db, dc, dd;
    ea = vertex_exists(a, b, t.l, t.y, t.x, &da);
    if (t.y < a.H - 1 && t.x < a.W - 1) {
      const bool eb = vertex_exists(a, b, t.l, t.y, t.x + 1, &db);
      const bool ec = vertex_exists(a, b, t.l, t.y + 1, t.x, &dc);
      if (eb && ec) {
        t0 = ea && edge_ok(a, da, dc, db);
        t1 = vertex_exists(a, b, t.l, t.y + 1, t.x + 1, &dd) && edge_ok(a, db, dc, dd);
      }
    }
  }
  const uint64_t bv = __ballot(ea), b0 = __ballot(t0), b1 = __ballot(t1);
  if ((threadIdx.x & 63) == 0) {
    s_v[threadIdx.x >> 6] = __popcll(bv);
    s_f[threadIdx.x >> 6] = __popcll(b0) + __popcll(b1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int nv = 0, nf = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) nv += s_v[w], nf += s_f[w];
    a.totals[(int64_t)b * a.G + blockIdx.x] = make_int2(nv, nf);
  }
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int wave_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

__global__ __launch_bounds__(TPB) void scan_kernel(MeshArgs a) {
  __shared__ int s_v[WAVES], s_f[WAVES];
  const int b = blockIdx.x, wave = threadIdx.x >> 6;
  int2* totals = a.totals + (int64_t)b * a.G;
  int cv = 0, cf = 0;                                   // the carry: all earlier trips
  for (int base = 0; base < a.G; base += TRIP) {        // (uniform: a kernel argument)
    const int i = base + threadIdx.x;
    const int2 t = i < a.G ? totals[i] : make_int2(0, 0);
    const int iv = wave_scan(t.x), jf = wave_scan(t.y);
    __syncthreads();                                    // the previous trip's reads of s_*
    if ((threadIdx.x & 63) == 63) s_v[wave] = iv, s_f[wave] = jf;
    __syncthreads();
    int ov = cv, of = cf, sv = 0, sf = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) ov += s_v[w], of += s_f[w];
      sv += s_v[w], sf += s_f[w];
    }
    if (i < a.G) totals[i] = make_int2(ov + iv - t.x, of + jf - t.y);
    cv += sv, cf += sf;
  }
  if (threadIdx.x == 0) a.counts[2 * b] = cv, a.counts[2 * b + 1] = cf;
}

// the byte of a colour channel: lsi_visual_pack_u8's rule with lo = 0, inv = 1
__device__ __forceinline__ uint32_t colour_byte(float v) {
  if (v != v) return 0u;
  const float t = fminf(fmaxf(v, 0.0f), 1.0f);
  return (uint32_t)(int)floorf(__fadd_rn(__fmul_rn(t, 255.0f), 0.5f));
}

__global__ __launch_bounds__(TPB) void vertex_kernel(MeshArgs a) {
  __shared__ int s_v[WAVES];
  const int b = blockIdx.y, n = blockIdx.x * TPB + threadIdx.x;
  bool ea = false;
  float d = 0.0f;
  Texel t = {0, 0, 0};
  if (n < a.N) {
    t = texel_of(a, n);
    ea = vertex_exists(a, b, t.l, t.y, t.x, &d);
  }
  const uint64_t bv = __ballot(ea);
  if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = __popcll(bv);
  __syncthreads();
  if (n >= a.N) return;
  int rank = a.totals[(int64_t)b * a.G + blockIdx.x].x + lower_lanes(bv);
#pragma unroll
  for (int w = 0; w < WAVES; ++w)
    if (w < (int)(threadIdx.x >> 6)) rank += s_v[w];
  a.map[(int64_t)b * a.N + n] = ea ? rank : -1;
  if (!ea || rank >= a.vcap) return;
  const float* k = a.kinv + 9 * b;
  const float u = (float)t.x + 0.5f, v = (float)t.y + 0.5f, z = __fdiv_rn(1.0f, d);
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(k[3 * r], u), __fmul_rn(k[3 * r + 1], v)),
                               k[3 * r + 2]), z);
  if (a.flip) p[1] = -p[1], p[2] = -p[2];
  const float* c = a.tex + (t.l * a.tex_sl + b * a.tex_sb + t.y * a.tex_sy + t.x * a.tex_sx);
  const uint32_t rgba = colour_byte(c[0]) | colour_byte(c[a.tex_sc]) << 8 |
                        colour_byte(c[2 * a.tex_sc]) << 16 | 0xff000000u;
  float4 rec = make_float4(p[0], p[1], p[2], __uint_as_float(rgba));
  *reinterpret_cast<float4*>(a.vbuf + ((int64_t)b * a.vcap + rank) * VB) = rec;
}

__device__ __forceinline__ void stage_face(uint8_t* s, int i0, int i1, int i2) {
  s[0] = 3;
  const uint32_t v[3] = {(uint32_t)i0, (uint32_t)i1, (uint32_t)i2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s[1 + 4 * k] = (uint8_t)v[k], s[2 + 4 * k] = (uint8_t)(v[k] >> 8);
    s[3 + 4 * k] = (uint8_t)(v[k] >> 16), s[4 + 4 * k] = (uint8_t)(v[k] >> 24);
  }
}

__global__ __launch_bounds__(TPB) void face_kernel(MeshArgs a) {
  __shared__ int s_f[WAVES];
  // the workgroup's records at the byte phase (0 .. 3) of their place in fbuf
  __shared__ uint32_t s_rec[(2 * TPB * FB + 3 + 3) / 4];
  const int b = blockIdx.y, n = blockIdx.x * TPB + threadIdx.x;
  bool t0 = false, t1 = false;
  int ia = -1, ib = -1, ic = -1, id = -1;
  if (n < a.N) {
    const Texel t = texel_of(a, n);
    if (t.y < a.H - 1 && t.x < a.W - 1) {
      const int32_t* m = a.map + (int64_t)b * a.N + n;
      ib = m[1], ic = m[a.W];
      if (ib >= 0 && ic >= 0) {
        ia = m[0], id = m[a.W + 1];
        const float db = disp_at(a, b, t.l, t.y, t.x + 1), dc = disp_at(a, b, t.l, t.y + 1, t.x);
        if (ia >= 0) t0 = edge_ok(a, disp_at(a, b, t.l, t.y, t.x), dc, db);
        if (id >= 0) t1 = edge_ok(a, db, dc, disp_at(a, b, t.l, t.y + 1, t.x + 1));
      }
    }
  }
  const uint64_t b0 = __ballot(t0), b1 = __ballot(t1);
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = __popcll(b0) + __popcll(b1);
  __syncthreads();
  int local = lower_lanes(b0) + lower_lanes(b1), total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < (int)(threadIdx.x >> 6)) local += s_f[w];
    total += s_f[w];
  }
  const int first = a.totals[(int64_t)b * a.G + blockIdx.x].y;     // the item's earlier faces
  // what the capacity leaves of [first, first + total)
  const int keep = min(total, max(a.fcap - first, 0));
  if (keep == 0) return;                                           // (uniform)
  const int64_t A0 = ((int64_t)b * a.fcap + first) * FB, A1 = A0 + (int64_t)keep * FB;
  const int phase = (int)(A0 & 3);
  uint8_t* s = reinterpret_cast<uint8_t*>(s_rec) + phase;
  if (t0 && local < keep) stage_face(s + local * FB, ia, ic, ib);
  if (t1 && local + (t0 ? 1 : 0) < keep) stage_face(s + (local + (t0 ? 1 : 0)) * FB, ib, ic, id);
  __syncthreads();
  // s_rec[i] is the dword at byte (A0 - phase) + 4 i of fbuf.  The whole dwords
  // of [A0, A1) are [w0, w1): at least two, a record being 13 bytes.
  const int64_t w0 = (A0 + 3) >> 2, w1 = A1 >> 2;
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(s_rec);
  const int64_t origin = A0 - phase;
  uint32_t* out = reinterpret_cast<uint32_t*>(a.fbuf) + w0;
  const int skip = (int)(w0 - (origin >> 2)), words = (int)(w1 - w0);
  for (int i = threadIdx.x; i < words; i += TPB) out[i] = s_rec[skip + i];
  const int head = (int)(4 * w0 - A0), tail = (int)(A1 - 4 * w1);  // 0 .. 3 bytes each
  if (threadIdx.x < head) a.fbuf[A0 + threadIdx.x] = sb[phase + threadIdx.x];
  if (threadIdx.x < tail)
    a.fbuf[4 * w1 + threadIdx.x] = sb[(int)(4 * w1 - origin) + threadIdx.x];
}

bool ratio_ok(float r) { return r >= 0.0f && r <= 1.0f; }   // (a NaN fails)

// The plan of a descriptor; false for one the call refuses.
bool plan(const LsiMeshDesc* d, MeshArgs* a) {
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
  if ((d->flags & ~LSI_MESH_FLIP_YZ) != 0 || d->reserved != 0) return false;
  a->L = d->L, a->H = d->H, a->W = d->W, a->N = (int32_t)n;
  a->G = (int32_t)((n + TPB - 1) / TPB);
  a->tex_sl = d->tex_sl, a->tex_sb = d->tex_sb, a->tex_sy = d->tex_sy, a->tex_sx = d->tex_sx;
  a->tex_sc = d->tex_sc;
  a->disp_sl = d->disp_sl, a->disp_sb = d->disp_sb, a->disp_sy = d->disp_sy;
  a->disp_sx = d->disp_sx;
  a->mask_sl = d->mask_sl, a->mask_sb = d->mask_sb, a->mask_sy = d->mask_sy;
  a->mask_sx = d->mask_sx;
  a->disp_min = d->disp_min, a->mask_min = d->mask_min;
  a->edge_ratio = d->edge_ratio, a->merge_ratio = d->merge_ratio;
  a->flip = (d->flags & LSI_MESH_FLIP_YZ) != 0;
  return true;
}

// bytes of the index map of all items, a multiple of 16: the totals follow it
size_t map_bytes(const LsiMeshDesc* d, const MeshArgs& a) {
  return ((size_t)d->B * (size_t)a.N * sizeof(int32_t) + 15) / 16 * 16;
}

}  // namespace

extern "C" {

size_t lsi_ldi_mesh_workspace_bytes(const LsiMeshDesc* desc) {
  MeshArgs a;
  if (!plan(desc, &a)) return 0;
  return map_bytes(desc, a) + (size_t)desc->B * (size_t)a.G * sizeof(int2);
}

int lsi_ldi_mesh(const LsiMeshDesc* desc, const float* tex, const float* mask,
                 const float* disp, const float* kinv_dev, void* vertices,
                 int64_t vertex_capacity, void* faces, int64_t face_capacity,
                 int32_t* counts, void* workspace, size_t workspace_bytes,
                 lsi_stream_t stream) {
  MeshArgs a;
  if (!plan(desc, &a)) return LSI_EINVAL;
  if (vertex_capacity < 0 || vertex_capacity > MAX_CAPACITY || face_capacity < 0 ||
      face_capacity > MAX_CAPACITY)
    return LSI_EINVAL;
  if (((uintptr_t)tex & 3) || ((uintptr_t)mask & 3) || ((uintptr_t)disp & 3) ||
      ((uintptr_t)kinv_dev & 3) || ((uintptr_t)vertices & 15) || ((uintptr_t)faces & 3) ||
      ((uintptr_t)counts & 3) || ((uintptr_t)workspace & 15))
    return LSI_EINVAL;
  if (!tex || !disp || !kinv_dev || !counts || !workspace) return LSI_ENULL;
  if ((!vertices && vertex_capacity > 0) || (!faces && face_capacity > 0)) return LSI_ENULL;
  if (workspace_bytes < lsi_ldi_mesh_workspace_bytes(desc)) return LSI_EWORKSPACE;
  a.tex = tex, a.mask = mask, a.disp = disp, a.kinv = kinv_dev;
  a.vbuf = static_cast<uint8_t*>(vertices), a.fbuf = static_cast<uint8_t*>(faces);
  a.counts = counts;
  a.map = static_cast<int32_t*>(workspace);
  a.totals = reinterpret_cast<int2*>(static_cast<uint8_t*>(workspace) + map_bytes(desc, a));
  a.vcap = (int32_t)vertex_capacity, a.fcap = (int32_t)face_capacity;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.G, desc->B);
  hipLaunchKernelGGL(count_kernel, grid, dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(scan_kernel, dim3(desc->B), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(vertex_kernel, grid, dim3(TPB), 0, s, a);
  if (face_capacity > 0) hipLaunchKernelGGL(face_kernel, grid, dim3(TPB), 0, s, a);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
