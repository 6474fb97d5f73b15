// Evaluation metrics accumulated on the device (gfx950): the arithmetic of the
// reference's define_metrics (ldi_pred_eval.py:297-548) after the render, and
// its dis-occlusion mask (lsi/geometry/projection.py:109-150).  The reference
// builds each from 20-40 stock elementwise / reduce ops and reads every
// (sum, normaliser) pair back to the host; here one pass per rendered view or
// per pair of LDIs leaves its sums in a caller-owned device array of
// LSI_EVAL_SLOTS doubles, which the caller reads once at the end.
// Bound: HBM streaming, a few MB per call -- launch latency in practice.
// Reductions: per-thread fp32, per-block and final sums in fp64 in a fixed
// order (lsi_reduce.h); the accumulator is updated by thread 0 of a one-block
// finishing kernel, so a sequence of calls is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"
#include "lsi_layers.h"
#include "lsi_reduce.h"

// the mask's coordinates feed floor() and a threshold
#pragma clang fp contract(off)

using namespace lsi;

namespace {

// ---------------------------------------------------------------------------
// view-synthesis metrics (ldi_pred_eval.py:385-460)
// ---------------------------------------------------------------------------
enum { V_PW, V_CENTRE, V_PW_DM, V_CENTRE_DM, V_PD, V_PD_DM, V_SE, V_NSUM };

struct EvalViewArgs {
  int nl, B, Ht, Wt, H, W, x_min, y_min;
  const float* recons;       // [nl, B, Ht, Wt, 3]
  const float* recons_disp;  // [nl, B, Ht, Wt] or NULL
  const float* target;       // [B, H, W, 3], element strides below
  long t_sb, t_sy, t_sx, t_sc;
  const float* valid;        // [B, H, W] or NULL
  const void* disocc;        // [B, H, W] float or uint8, or NULL
  const float* gt_disp;      // [B, H, W] or NULL
  int disocc_u8, valid_gt;
  float valid_thresh;
};

__global__ __launch_bounds__(TPB) void eval_view_kernel(EvalViewArgs a, double* part) {
  const int fy = a.H / a.Ht, fx = a.W / a.Wt;
  const long N = (long)a.B * a.Ht * a.Wt;
  float acc[V_NSUM];
#pragma unroll
  for (int k = 0; k < V_NSUM; ++k) acc[k] = 0.0f;
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < N;
       i += (long)gridDim.x * TPB) {
    const int xt = (int)(i % a.Wt);
    const long q = i / a.Wt;
    const int yt = (int)(q % a.Ht), b = (int)(q / a.Ht);
    // centre = crop * valid is 0 or 1, and every sum carries it as a factor:
    // a cell outside contributes nothing and is not read
    if (xt < a.x_min || xt >= a.Wt - a.x_min || yt < a.y_min || yt >= a.Ht - a.y_min)
      continue;
    // first element of the cell's fy x fx block in a contiguous [B, H, W] map
    const long f0 = ((long)b * a.H + (long)yt * fy) * a.W + (long)xt * fx;
    if (a.valid) {
      // "ignore pixels that might have aliasing": > 0.95 after the AREA resize
      float v[1];
      if (a.valid_gt) {  // the mask is the caller's (map > valid_thresh).float()
        v[0] = 0.0f;
        for (int dy = 0; dy < fy; ++dy)
          for (int dx = 0; dx < fx; ++dx)
            v[0] += a.valid[f0 + (long)dy * a.W + dx] > a.valid_thresh ? 1.0f : 0.0f;
        v[0] *= 1.0f / (float)(fy * fx);
      } else {
        area_mean<1>(a.valid + f0, a.W, 1, 0, fy, fx, v);
      }
      if (!(v[0] > 0.95f)) continue;
    }
    float t[3];
    area_mean<3>(a.target + (long)b * a.t_sb + (long)yt * fy * a.t_sy +
                     (long)xt * fx * a.t_sx,
                 a.t_sy, a.t_sx, a.t_sc, fy, fx, t);
    const long cell = ((long)b * a.Ht + yt) * a.Wt + xt;  // within one layer
    const long P = (long)a.B * a.Ht * a.Wt;
    float pw = 0.0f, se = 0.0f;
    for (int l = 0; l < a.nl; ++l) {
      const float* r = a.recons + ((long)l * P + cell) * 3;
      const float e0 = t[0] - r[0], e1 = t[1] - r[1], e2 = t[2] - r[2];
      // mean over the three channels: sum, then / 3
      const float l1 = ((fabsf(e0) + fabsf(e1)) + fabsf(e2)) / 3.0f;
      if (l == 0) {
        pw = l1;
        se = ((e0 * e0 + e1 * e1) + e2 * e2) / 3.0f;
      } else {
        pw = fminf(pw, l1);
      }
    }
    float dm = 0.0f;
    if (a.disocc) {
      float m[1];
      if (a.disocc_u8)
        area_mean<1>((const uint8_t*)a.disocc + f0, a.W, 1, 0, fy, fx, m);
      else
        area_mean<1>((const float*)a.disocc + f0, a.W, 1, 0, fy, fx, m);
      dm = m[0];
    }
    float pd = 0.0f;
    if (a.recons_disp && a.gt_disp) {
      float g[1];
      area_mean<1>(a.gt_disp + f0, a.W, 1, 0, fy, fx, g);
      pd = fabsf(g[0] - a.recons_disp[cell]);
      for (int l = 1; l < a.nl; ++l)
        pd = fminf(pd, fabsf(g[0] - a.recons_disp[(long)l * P + cell]));
    }
    acc[V_PW] += pw;
    acc[V_CENTRE] += 1.0f;
    acc[V_PW_DM] += pw * dm;
    acc[V_CENTRE_DM] += dm;
    acc[V_PD] += pd;
    acc[V_PD_DM] += pd * dm;
    acc[V_SE] += se;
  }
  block_store_partials<V_NSUM>(acc, part);
}

__global__ __launch_bounds__(TPB) void eval_view_finish_kernel(
    const double* part, int nblk, int has_disocc, int has_depth, double* acc) {
  __shared__ double sm[TPB];
  double s[V_NSUM];
  for (int k = 0; k < V_NSUM; ++k) s[k] = block_total(part + (size_t)k * MAXBLK, nblk, sm);
  if (threadIdx.x != 0) return;
  acc[LSI_EVAL_COMPOSE_SUM] += s[V_PW];
  acc[LSI_EVAL_COMPOSE_NORM] += s[V_CENTRE];
  if (has_disocc) {
    acc[LSI_EVAL_COMPOSE_DISOCC_SUM] += s[V_PW_DM];
    acc[LSI_EVAL_COMPOSE_DISOCC_NORM] += s[V_CENTRE_DM];
  }
  if (has_depth) {
    acc[LSI_EVAL_DEPTH_SUM] += s[V_PD];
    acc[LSI_EVAL_DEPTH_NORM] += s[V_CENTRE];
    if (has_disocc) {
      acc[LSI_EVAL_DEPTH_DISOCC_SUM] += s[V_PD_DM];
      acc[LSI_EVAL_DEPTH_DISOCC_NORM] += s[V_CENTRE_DM];
    }
  }
  if (s[V_CENTRE] > 0.0) {
    const double mse = fmax(s[V_SE] / s[V_CENTRE], 1e-20);
    acc[LSI_EVAL_PSNR_SUM] += 10.0 * log10(1.0 / mse);
    acc[LSI_EVAL_PSNR_COUNT] += 1.0;
  }
}

// ---------------------------------------------------------------------------
// per-layer metrics (ldi_pred_eval.py:476-531)
// ---------------------------------------------------------------------------
enum { L_FG_TEX, L_FG_DISP, L_FG_N, L_BG_TEX, L_BG_DISP, L_BG_N, L_NSUM };

struct EvalLayerView {
  const float *tex, *disp, *img, *gt_disp, *gt_disp_bg, *gt_tex_bg;
  long tex_sl, tex_sb, tex_sy, tex_sx, tex_sc;
  long disp_sl, disp_sb, disp_sy, disp_sx;
};

struct EvalLayerArgs {
  int L, B, H, W;
  float bg_layer_disp;
  EvalLayerView v[2];
};

// sum_c |tex_c - ref_c|; the / 3 is applied once to the total, in fp64
__device__ __forceinline__ float tex_l1(const float* tp, long sc, const float* ref) {
  return (fabsf(tp[0] - ref[0]) + fabsf(tp[sc] - ref[1])) + fabsf(tp[2 * sc] - ref[2]);
}

__global__ __launch_bounds__(TPB) void eval_layer_kernel(EvalLayerArgs a, double* part) {
  const long P = (long)a.B * a.H * a.W;
  float acc[L_NSUM];
#pragma unroll
  for (int k = 0; k < L_NSUM; ++k) acc[k] = 0.0f;
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < 2 * P;
       i += (long)gridDim.x * TPB) {
    const EvalLayerView& w = a.v[i >= P ? 1 : 0];
    const long p = i >= P ? i - P : i;
    const int x = (int)(p % a.W);
    const long q = p / a.W;
    const int y = (int)(q % a.H), b = (int)(q / a.H);
    const long to = (long)b * w.tex_sb + (long)y * w.tex_sy + (long)x * w.tex_sx;
    const long d_o = (long)b * w.disp_sb + (long)y * w.disp_sy + (long)x * w.disp_sx;
    const float gd = w.gt_disp[p];
    if (gd > a.bg_layer_disp) {
      acc[L_FG_TEX] += tex_l1(w.tex + to, w.tex_sc, w.img + p * 3);
      acc[L_FG_DISP] += fabsf(w.disp[d_o] - gd);
      acc[L_FG_N] += 1.0f;
    }
    if (w.gt_disp_bg) {
      const float gb = w.gt_disp_bg[p];
      if (gd > gb) {
        const long ll = a.L - 1;
        acc[L_BG_TEX] += tex_l1(w.tex + to + ll * w.tex_sl, w.tex_sc, w.gt_tex_bg + p * 3);
        acc[L_BG_DISP] += fabsf(w.disp[d_o + ll * w.disp_sl] - gb);
        acc[L_BG_N] += 1.0f;
      }
    }
  }
  block_store_partials<L_NSUM>(acc, part);
}

__global__ __launch_bounds__(TPB) void eval_layer_finish_kernel(
    const double* part, int nblk, int has_bg, double* acc) {
  __shared__ double sm[TPB];
  double s[L_NSUM];
  for (int k = 0; k < L_NSUM; ++k) s[k] = block_total(part + (size_t)k * MAXBLK, nblk, sm);
  if (threadIdx.x != 0) return;
  acc[LSI_EVAL_FG_TEX_SUM] += s[L_FG_TEX] / 3.0;
  acc[LSI_EVAL_FG_DISP_SUM] += s[L_FG_DISP];
  acc[LSI_EVAL_FG_NORM] += s[L_FG_N];
  if (has_bg) {
    acc[LSI_EVAL_BG_TEX_SUM] += s[L_BG_TEX] / 3.0;
    acc[LSI_EVAL_BG_DISP_SUM] += s[L_BG_DISP];
    acc[LSI_EVAL_BG_NORM] += s[L_BG_N];
  }
}

// ---------------------------------------------------------------------------
// dis-occlusion mask (projection.py:109-150), source points on the pixel grid
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void disocclusion_kernel(
    int Hs, int Ws, int Ht, int Wt, const float* __restrict__ disps_src,
    const float* __restrict__ disps_trg, const float* __restrict__ M, float thresh,
    float* __restrict__ mask) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Hs * Ws) return;
  const int x = i % Ws, y = i / Ws;
  const size_t si = (size_t)b * Hs * Ws + i;
  // q = M (x + .5, y + .5, 1, d) and divide_safe under the renderer's contract;
  // the splat footprint project_px also forms is unused here (scale 1, mask 1)
  Proj o;
  project_px(M + 16 * b, (float)x + 0.5f, (float)y + 0.5f, disps_src[si], 1.0f, 1.0f,
             1.0f, 0.0f, Ht, Wt, o);
  const float u = div_rn(o.q0, o.nden), v = div_rn(o.q1, o.nden);
  const bool trunc = u > (float)Wt || v > (float)Ht || u < 0.0f || v < 0.0f;
  Taps t;
  taps_of(u, v, Ht, Wt, t);
  float c[4];
  tap_weights(t, c);
  const float sampled = bilinear_gather(t, c, disps_trg + (size_t)b * Ht * Wt, 1, 0);
  const float dis = fabsf(o.dd - sampled) > thresh ? 1.0f : 0.0f;
  mask[si] = (1.0f - (trunc ? 1.0f : 0.0f)) * dis;
}

constexpr int EVAL_NSUM = V_NSUM > L_NSUM ? V_NSUM : L_NSUM;

void layer_view_of(const LsiLossDesc* d, const float* tex, const float* disp,
                   const float* img, const float* gt_disp, const float* gt_disp_bg,
                   const float* gt_tex_bg, EvalLayerView* w) {
  w->tex = tex; w->disp = disp; w->img = img; w->gt_disp = gt_disp;
  w->gt_disp_bg = gt_disp_bg; w->gt_tex_bg = gt_tex_bg;
  w->tex_sl = d->img_sl; w->tex_sb = d->img_sb; w->tex_sy = d->img_sy;
  w->tex_sx = d->img_sx; w->tex_sc = d->img_sc;
  w->disp_sl = d->disp_sl; w->disp_sb = d->disp_sb; w->disp_sy = d->disp_sy;
  w->disp_sx = d->disp_sx;
}

}  // namespace

extern "C" {

size_t lsi_eval_workspace_bytes(void) {
  return (size_t)EVAL_NSUM * MAXBLK * sizeof(double);
}

int lsi_eval_view_metrics(int32_t nl, int32_t B, int32_t Ht, int32_t Wt,
                          int32_t H, int32_t W, int32_t x_min, int32_t y_min,
                          const float* recons, const float* recons_disp,
                          const float* target, int64_t t_sb, int64_t t_sy,
                          int64_t t_sx, int64_t t_sc, const float* valid,
                          const void* disocc, const float* gt_disp,
                          uint32_t flags, float valid_thresh, double* acc,
                          void* ws, size_t ws_bytes, lsi_stream_t stream) {
  if (nl <= 0 || B <= 0 || Ht <= 0 || Wt <= 0 || H <= 0 || W <= 0 || H % Ht ||
      W % Wt || x_min < 0 || y_min < 0 ||
      (flags & ~(LSI_EVAL_DISOCC_U8 | LSI_EVAL_VALID_GT)))
    return LSI_EINVAL;
  if (!recons || !target || !acc || !ws || ws_bytes < lsi_eval_workspace_bytes())
    return LSI_EINVAL;
  EvalViewArgs a;
  a.nl = nl; a.B = B; a.Ht = Ht; a.Wt = Wt; a.H = H; a.W = W;
  a.x_min = x_min; a.y_min = y_min;
  a.recons = recons; a.recons_disp = recons_disp; a.target = target;
  a.t_sb = t_sb; a.t_sy = t_sy; a.t_sx = t_sx; a.t_sc = t_sc;
  a.valid = valid; a.disocc = disocc; a.gt_disp = gt_disp;
  a.disocc_u8 = (flags & LSI_EVAL_DISOCC_U8) ? 1 : 0;
  a.valid_gt = (flags & LSI_EVAL_VALID_GT) ? 1 : 0;
  a.valid_thresh = valid_thresh;
  const int g = grid_for((long)B * Ht * Wt);
  hipLaunchKernelGGL(eval_view_kernel, dim3(g), dim3(TPB), 0, (hipStream_t)stream,
                     a, (double*)ws);
  hipLaunchKernelGGL(eval_view_finish_kernel, dim3(1), dim3(TPB), 0,
                     (hipStream_t)stream, (const double*)ws, g, disocc ? 1 : 0,
                     (recons_disp && gt_disp) ? 1 : 0, acc);
  return rc_of_launch();
}

int lsi_eval_layer_metrics(const LsiLossDesc* sd, const float* src_tex,
                           const float* src_disp, const float* src_img,
                           const float* src_gt_disp, const float* src_gt_disp_bg,
                           const float* src_gt_tex_bg, const LsiLossDesc* td,
                           const float* trg_tex, const float* trg_disp,
                           const float* trg_img, const float* trg_gt_disp,
                           const float* trg_gt_disp_bg, const float* trg_gt_tex_bg,
                           double* acc, void* ws, size_t ws_bytes,
                           lsi_stream_t stream) {
  if (!sd || !td || sd->L <= 0 || sd->B <= 0 || sd->H <= 0 || sd->W <= 0 ||
      sd->L != td->L || sd->B != td->B || sd->H != td->H || sd->W != td->W ||
      sd->bg_layer_disp != td->bg_layer_disp)
    return LSI_EINVAL;
  if (!src_tex || !src_disp || !src_img || !src_gt_disp || !trg_tex || !trg_disp ||
      !trg_img || !trg_gt_disp || !acc || !ws ||
      ws_bytes < lsi_eval_workspace_bytes())
    return LSI_EINVAL;
  // the background inputs: all four or none
  const int n_bg = (src_gt_disp_bg ? 1 : 0) + (src_gt_tex_bg ? 1 : 0) +
                   (trg_gt_disp_bg ? 1 : 0) + (trg_gt_tex_bg ? 1 : 0);
  if (n_bg != 0 && n_bg != 4) return LSI_EINVAL;
  EvalLayerArgs a;
  a.L = sd->L; a.B = sd->B; a.H = sd->H; a.W = sd->W;
  a.bg_layer_disp = sd->bg_layer_disp;
  layer_view_of(sd, src_tex, src_disp, src_img, src_gt_disp, src_gt_disp_bg,
                src_gt_tex_bg, &a.v[0]);
  layer_view_of(td, trg_tex, trg_disp, trg_img, trg_gt_disp, trg_gt_disp_bg,
                trg_gt_tex_bg, &a.v[1]);
  const int g = grid_for(2L * a.B * a.H * a.W);
  hipLaunchKernelGGL(eval_layer_kernel, dim3(g), dim3(TPB), 0, (hipStream_t)stream,
                     a, (double*)ws);
  hipLaunchKernelGGL(eval_layer_finish_kernel, dim3(1), dim3(TPB), 0,
                     (hipStream_t)stream, (const double*)ws, g, n_bg ? 1 : 0, acc);
  return rc_of_launch();
}

int lsi_disocclusion_mask(int32_t B, int32_t Hs, int32_t Ws, int32_t Ht,
                          int32_t Wt, const float* disps_src,
                          const float* disps_trg, const float* M, float thresh,
                          float* mask, lsi_stream_t stream) {
  // tap indices are formed in fp32 (taps_of): exact below 2^24 target pixels
  if (B <= 0 || Hs <= 0 || Ws <= 0 || Ht <= 0 || Wt <= 0 || B > 65535 ||
      (int64_t)Ht * Wt >= (1 << 24) || (int64_t)Hs * Ws >= (1 << 24))
    return LSI_EINVAL;
  if (!disps_src || !disps_trg || !M || !mask) return LSI_EINVAL;
  const int Ns = Hs * Ws;
  hipLaunchKernelGGL(disocclusion_kernel, dim3((Ns + 255) / 256, B), dim3(256), 0,
                     (hipStream_t)stream, Hs, Ws, Ht, Wt, disps_src, disps_trg, M,
                     thresh, mask);
  return rc_of_launch();
}

}  // extern "C"
