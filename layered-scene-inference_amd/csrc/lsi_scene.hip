// Fused renderer of planar scenes on MI355X (gfx950): lsi_render_planes.
//
// One launch renders B worlds x V views.  Per view pixel and plane, in
// registers: homography (helpers.transform_pts), divide_safe, the four
// bilinear taps of the RGBA texel (sampling.py:41-168), the analytic plane
// disparity (homography.trg_disp_maps); then over the P + 1 layers the soft
// z-buffer, layers.compose (hard or soft) and layers.compose_depth
// (bg_layer=False) -- optionally a second time with the masks of the object
// planes [n_box, P) taken as 0 (the room alone).  The warped P x H x W x 5
// layers of the op route never exist in memory.
//
// The arithmetic is the op route's, operation for operation: taps_of and
// layer_logp_of are the code lsi_sampling.hip / lsi_loss.hip compile
// (lsi_layers.h); the max / sum / div_rn(expf, sum) / first-maximum sequence is
// compose_kernel's.
//
// Mapping: one thread per view pixel, pixels numbered along rows, so a wave
// covers a run of 64 pixels of one row (W % 64 == 0) and its taps fall on
// neighbouring 16-byte texels.  The 12 floats of a plane are addressed by
// blockIdx and the (unrolled) plane index only: wave-uniform loads through the
// constant cache, no per-lane traffic.  Workgroups are renumbered so that the
// blocks of one world (all its views) run on one XCD -- workgroup i runs on XCD
// i % 8, every XCD takes a contiguous run of (world, view, block) ids -- and a
// texel is brought into one L2 instead of eight.  No atomics, no LDS, no
// workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"
#include "lsi_layers.h"

#pragma clang fp contract(off)

using namespace lsi;

namespace {

constexpr int TPB = 256;

struct SArgs {
  int P, Hs, Ws, H, W, n_box, soft;
  int nblk;            // workgroups per view
  unsigned outputs;
  float min_disp, temp;
  const float4* tex;   // [B, P, Hs, Ws] RGBA
  const float* hom;    // [B, V, P, 9]
  const float* dmat;   // [B, V, P, 3]
  float* img; float* disp; float* img_room; float* disp_room;
  int V;
};

// One composition of the pixel's P + 1 layers (compose_kernel's sequence,
// csrc/lsi_loss.hip): lp[] the planes' log-probabilities, lp_bg the background
// layer's.  Every index is a compile-time constant after unrolling, the winner
// is carried by selects: nothing is addressed by a lane's own index.
template <int PB>
__device__ __forceinline__ void compose_px(int P, const float (&lp)[PB], float lp_bg,
                                           const float (&d)[PB],
                                           const float (&col)[PB][3], int soft,
                                           float min_disp, float (&o_img)[3],
                                           float& o_disp) {
  float mx = lp[0];
#pragma unroll
  for (int l = 1; l < PB; ++l)
    if (l < P) mx = fmaxf(mx, lp[l]);
  mx = fmaxf(mx, lp_bg);
  float sum = 0.0f;
#pragma unroll
  for (int l = 0; l < PB; ++l)
    if (l < P) sum += expf(lp[l] - mx);
  sum += expf(lp_bg - mx);
  float pbest = div_rn(expf(lp[0] - mx), sum);
  float bd = d[0], b0 = col[0][0], b1 = col[0][1], b2 = col[0][2];
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  if (soft) { s0 += pbest * col[0][0]; s1 += pbest * col[0][1]; s2 += pbest * col[0][2]; }
#pragma unroll
  for (int l = 1; l < PB; ++l) {
    if (l < P) {
      const float pl = div_rn(expf(lp[l] - mx), sum);
      if (pl > pbest) {
        pbest = pl; bd = d[l]; b0 = col[l][0]; b1 = col[l][1]; b2 = col[l][2];
      }
      if (soft) { s0 += pl * col[l][0]; s1 += pl * col[l][1]; s2 += pl * col[l][2]; }
    }
  }
  {
    const float pl = div_rn(expf(lp_bg - mx), sum);
    if (pl > pbest) { pbest = pl; bd = min_disp; b0 = b1 = b2 = 1.0f; }
    if (soft) { s0 += pl * 1.0f; s1 += pl * 1.0f; s2 += pl * 1.0f; }
  }
  o_img[0] = soft ? s0 : b0; o_img[1] = soft ? s1 : b1; o_img[2] = soft ? s2 : b2;
  o_disp = bd;
}

template <int PB, bool ROOM>
__global__ __launch_bounds__(TPB) void render_planes_kernel(SArgs a) {
  // XCD-aware numbering (as lsi_splat_stream2.hip): workgroup `lin` runs on XCD
  // lin % 8 and takes the (lin / 8)-th id of that XCD's contiguous run
  const unsigned nwg = gridDim.x, lin = blockIdx.x;
  const unsigned xcd = lin & 7u, q = nwg >> 3, r8 = nwg & 7u;
  const unsigned base = xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q;
  const unsigned id = base + (lin >> 3);
  const int bv = (int)(id / (unsigned)a.nblk);        // b * V + v
  const int blk = (int)(id - (unsigned)bv * (unsigned)a.nblk);
  const int b = bv / a.V;
  const int pix = blk * TPB + (int)threadIdx.x;
  if (pix >= a.H * a.W) return;
  const int iy = pix / a.W, ix = pix - iy * a.W;
  const float x = (float)ix + 0.5f, y = (float)iy + 0.5f;   // helpers.pixel_coords

  const int P = a.P;
  const float* __restrict__ hom = a.hom + (size_t)bv * P * 9;
  const float* __restrict__ dmat = a.dmat + (size_t)bv * P * 3;
  const size_t plane_px = (size_t)a.Hs * a.Ws;
  const float4* __restrict__ tex = a.tex + (size_t)b * P * plane_px;

  float lp[PB], lpr[PB], d[PB], col[PB][3];  // (lpr: dead without ROOM)
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    lp[p] = 0.0f; d[p] = 0.0f; col[p][0] = col[p][1] = col[p][2] = 0.0f;
    lpr[p] = 0.0f;
    if (p < P) {
      const float* __restrict__ h = hom + p * 9;
      // helpers.transform_pts (seq_matmul): ((x h0) + (y h1)) + 1 h2
      const float q0 = (x * h[0] + y * h[1]) + h[2];
      const float q1 = (x * h[3] + y * h[4]) + h[5];
      const float q2 = (x * h[6] + y * h[7]) + h[8];
      const float den = safe_den(q2);                 // homography.normalize_homogeneous
      const float u = div_rn(q0, den), v = div_rn(q1, den);
      Taps t;
      taps_of(u, v, a.Hs, a.Ws, t);
      const float c00 = t.vx0 * t.vy0 * t.wx0 * t.wy0;
      const float c01 = t.vx0 * t.vy1 * t.wx0 * t.wy1;
      const float c10 = t.vx1 * t.vy0 * t.wx1 * t.wy0;
      const float c11 = t.vx1 * t.vy1 * t.wx1 * t.wy1;
      const float4* __restrict__ tp = tex + (size_t)p * plane_px;
      // (indices are clamped into the texture by taps_of, 0 when !t.ok)
      const float4 t00 = tp[t.i00], t01 = tp[t.i01], t10 = tp[t.i10], t11 = tp[t.i11];
      float m = 0.0f;
      if (t.ok) {   // a non-finite coordinate samples 0 (bilinear_fwd_kernel)
        col[p][0] = ((c00 * t00.x + c01 * t01.x) + c10 * t10.x) + c11 * t11.x;
        col[p][1] = ((c00 * t00.y + c01 * t01.y) + c10 * t10.y) + c11 * t11.y;
        col[p][2] = ((c00 * t00.z + c01 * t01.z) + c10 * t10.z) + c11 * t11.z;
        m = ((c00 * t00.w + c01 * t01.w) + c10 * t10.w) + c11 * t11.w;
      }
      // homography.trg_disp_maps: ((D0 x) + (D1 y)) + D2 1
      const float* __restrict__ dm = dmat + p * 3;
      const float dd = (dm[0] * x + dm[1] * y) + dm[2];
      d[p] = fmaxf(dd, 0.0f);                         // relu (compose_kernel)
      lp[p] = layer_logp_of(m, d[p], a.temp);
      if (ROOM)  // the room alone: an object plane's mask is 0 everywhere
        lpr[p] = p < a.n_box ? lp[p] : layer_logp_of(0.0f, d[p], a.temp);
    }
  }
  const float lp_bg = layer_logp_of(1.0f, a.min_disp, a.temp);
  const size_t o = (size_t)bv * a.H * a.W + pix;
  float oi[3], od;
  compose_px<PB>(P, lp, lp_bg, d, col, a.soft, a.min_disp, oi, od);
  if (a.outputs & LSI_SCENE_IMG) {
    a.img[3 * o] = oi[0]; a.img[3 * o + 1] = oi[1]; a.img[3 * o + 2] = oi[2];
  }
  if (a.outputs & LSI_SCENE_DISP) a.disp[o] = od;
  if constexpr (ROOM) {
    compose_px<PB>(P, lpr, lp_bg, d, col, a.soft, a.min_disp, oi, od);
    if (a.outputs & LSI_SCENE_IMG_ROOM) {
      a.img_room[3 * o] = oi[0]; a.img_room[3 * o + 1] = oi[1];
      a.img_room[3 * o + 2] = oi[2];
    }
    if (a.outputs & LSI_SCENE_DISP_ROOM) a.disp_room[o] = od;
  }
}

template <int PB>
void launch_pb(const SArgs& a, bool room, unsigned grid, hipStream_t st) {
  if (room)
    hipLaunchKernelGGL((render_planes_kernel<PB, true>), dim3(grid), dim3(TPB), 0, st, a);
  else
    hipLaunchKernelGGL((render_planes_kernel<PB, false>), dim3(grid), dim3(TPB), 0, st, a);
}

}  // namespace

extern "C" {

int lsi_render_planes(const LsiSceneDesc* d, const float* tex_rgba, const float* hom,
                      const float* dmat, float* img, float* disp, float* img_room,
                      float* disp_room, lsi_stream_t stream) {
  if (!d) return LSI_ENULL;
  if (d->B <= 0 || d->V <= 0 || d->P <= 0 || d->P > LSI_SCENE_MAX_PLANES ||
      d->Hs <= 0 || d->Ws <= 0 || d->H <= 0 || d->W <= 0 || d->n_box < 0 ||
      d->n_box > d->P)
    return LSI_EINVAL;
  const unsigned all = LSI_SCENE_IMG | LSI_SCENE_DISP | LSI_SCENE_IMG_ROOM |
                       LSI_SCENE_DISP_ROOM;
  if (d->outputs == 0 || (d->outputs & ~all)) return LSI_EINVAL;
  // tap indices are formed in fp32 (taps_of): exact up to 2^24 texels per plane
  if ((int64_t)d->Hs * d->Ws > (1 << 24) || (int64_t)d->H * d->W > (1 << 30))
    return LSI_EINVAL;
  if (!tex_rgba || !hom || !dmat) return LSI_ENULL;
  if (((d->outputs & LSI_SCENE_IMG) && !img) || ((d->outputs & LSI_SCENE_DISP) && !disp) ||
      ((d->outputs & LSI_SCENE_IMG_ROOM) && !img_room) ||
      ((d->outputs & LSI_SCENE_DISP_ROOM) && !disp_room))
    return LSI_ENULL;
  if ((uintptr_t)tex_rgba & 15u) return LSI_EINVAL;   // one 16-byte load per tap
  const int64_t nblk = ((int64_t)d->H * d->W + TPB - 1) / TPB;
  const int64_t grid = nblk * d->B * d->V;
  if (grid > 0x7fffffffLL) return LSI_EINVAL;
  SArgs a;
  a.P = d->P; a.Hs = d->Hs; a.Ws = d->Ws; a.H = d->H; a.W = d->W; a.V = d->V;
  a.n_box = d->n_box; a.soft = d->soft != 0; a.nblk = (int)nblk;
  a.outputs = d->outputs; a.min_disp = d->min_disp; a.temp = d->temp;
  a.tex = reinterpret_cast<const float4*>(tex_rgba); a.hom = hom; a.dmat = dmat;
  a.img = img; a.disp = disp; a.img_room = img_room; a.disp_room = disp_room;
  const bool room = (d->outputs & (LSI_SCENE_IMG_ROOM | LSI_SCENE_DISP_ROOM)) != 0;
  hipStream_t st = (hipStream_t)stream;
  // the plane loop is unrolled to a compile-time bound: the smallest that holds P
  if (d->P <= 2) launch_pb<2>(a, room, (unsigned)grid, st);
  else if (d->P <= 5) launch_pb<5>(a, room, (unsigned)grid, st);
  else if (d->P <= 9) launch_pb<9>(a, room, (unsigned)grid, st);
  else launch_pb<16>(a, room, (unsigned)grid, st);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
