// Host code that the bf16 (lsi_conv_igemm.hip, lsi_conv_wgrad_igemm.hip) and the
// fp32 (lsi_conv_f32.hip) implicit-GEMM convolutions share: the descriptor
// check, the tap lists, the launch plan and its split over the input channels,
// the pack job, the weight gradient's tap table and pixel blocks, and the
// declarations of the family's internal cross-file functions.  Host only;
// templates over the kernels' argument structs (IgArgs / FArgs, GwArgs /
// FwArgs), whose layouts belong to the kernels and stay where they are.  Where
// the two precisions answer differently (a return code, a byte count), the
// caller passes its answer as a plain argument.
#ifndef LSI_CONV_HOST_H_
#define LSI_CONV_HOST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lsi_hip.h"

// What every kernel of the family takes: the kernel's input channels multiples
// of 32, its output channels of `cout_multiple`.
static inline bool conv_desc_common(const LsiConvDesc* d, int cout_multiple) {
  if (!d) return false;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->OH <= 0 || d->OW <= 0) return false;
  if (d->Cin <= 0 || d->Cout <= 0 || d->Cin % 32 || d->Cout % cout_multiple) return false;
  if (d->KH < 1 || d->KW < 1 || d->KH > 7 || d->KW > 7) return false;
  if (d->stride != 1 && d->stride != 2) return false;
  if (d->pad_t < 0 || d->pad_l < 0 || d->pad_t >= d->KH || d->pad_l >= d->KW) return false;
  // int32 element offsets inside the kernels
  if ((int64_t)d->N * d->H * d->W * d->Cin >= (1ll << 31)) return false;
  if ((int64_t)d->N * d->OH * d->OW * d->Cout >= (1ll << 31)) return false;
  return true;
}

// The tap lists of a call.  mode 0: forward (one class); mode 1: data gradient
// (stride^2 parity classes of input pixels).  `tap` receives ky * KW + kx of
// every tap in class order (the order of the packed weights).
template <class Args>
void conv_classes(const LsiConvDesc* d, int mode, Args& k, int8_t* tap) {
  memset(&k, 0, sizeof(k));
  int nt = 0;
  if (mode == 0) {
    auto& q = k.cls[0];
    for (int y = 0; y < d->KH; ++y)
      for (int xk = 0; xk < d->KW; ++xk) {
        tap[nt] = (signed char)(y * d->KW + xk);
        q.tdy[q.ntaps] = (signed char)(y - d->pad_t);
        q.tdx[q.ntaps] = (signed char)(xk - d->pad_l);
        ++q.ntaps; ++nt;
      }
    q.OHt = d->OH; q.OWt = d->OW; q.wofs = 0;
    k.ncls = 1;
    k.N = d->N; k.H = d->H; k.W = d->W; k.Cin = d->Cin; k.Cout = d->Cout;
    k.s = d->stride; k.os = 1; k.OHF = d->OH; k.OWF = d->OW;
    return;
  }
  const int s = d->stride;
  // input pixels (iy, ix) = (s i + p, s j + q): the taps with ky = p + pad_t (mod s)
  //   gx[s i + p] += gy[oy] W[ky],   s oy + ky - pad_t = s i + p
  for (int p = 0; p < s; ++p)
    for (int q_ = 0; q_ < s; ++q_) {
      auto& q = k.cls[k.ncls++];
      q.wofs = nt;
      for (int y = 0; y < d->KH; ++y) {
        if ((p + d->pad_t - y) % s != 0) continue;
        for (int xk = 0; xk < d->KW; ++xk) {
          if ((q_ + d->pad_l - xk) % s != 0) continue;
          tap[nt] = (signed char)(y * d->KW + xk);
          q.tdy[q.ntaps] = (signed char)((p + d->pad_t - y) / s);
          q.tdx[q.ntaps] = (signed char)((q_ + d->pad_l - xk) / s);
          ++q.ntaps; ++nt;
        }
      }
      q.ooy = p; q.oox = q_;
      q.OHt = (d->H - p + s - 1) / s; q.OWt = (d->W - q_ + s - 1) / s;
    }
  k.N = d->N; k.H = d->OH; k.W = d->OW; k.Cin = d->Cout; k.Cout = d->Cin;
  k.s = 1; k.os = s; k.OHF = d->H; k.OWF = d->W;
}

// Every class's smallest (dy, dx) into its dy0 / dx0; the largest tap span of a
// class in rows and columns and the tallest class.
struct ConvSpans {
  int spany, spanx, maxoh;
};
template <class Args>
ConvSpans conv_tap_spans(Args& k) {
  ConvSpans sp = {1, 1, 1};
  for (int c = 0; c < k.ncls; ++c) {
    auto& q = k.cls[c];
    int dy1 = -128, dx1 = -128, dy0 = 127, dx0 = 127;
    for (int t = 0; t < q.ntaps; ++t) {
      dy0 = q.tdy[t] < dy0 ? q.tdy[t] : dy0; dy1 = q.tdy[t] > dy1 ? q.tdy[t] : dy1;
      dx0 = q.tdx[t] < dx0 ? q.tdx[t] : dx0; dx1 = q.tdx[t] > dx1 ? q.tdx[t] : dx1;
    }
    if (q.ntaps == 0) { dy0 = dy1 = dx0 = dx1 = 0; }
    q.dy0 = dy0; q.dx0 = dx0;
    sp.spany = dy1 - dy0 + 1 > sp.spany ? dy1 - dy0 + 1 : sp.spany;
    sp.spanx = dx1 - dx0 + 1 > sp.spanx ? dx1 - dx0 + 1 : sp.spanx;
    sp.maxoh = q.OHt > sp.maxoh ? q.OHt : sp.maxoh;
  }
  return sp;
}

// toff[0 .. n) of every class: the tap's byte offset inside the staged patch
// (k.PW pixels per row, `pix_bytes` apart), 0 past the class's last tap.
template <class Args>
void conv_tap_offsets(Args& k, int pix_bytes, int n) {
  for (int c = 0; c < k.ncls; ++c) {
    auto& q = k.cls[c];
    for (int t = 0; t < n; ++t)
      q.toff[t] = t < q.ntaps ? ((q.tdy[t] - q.dy0) * k.PW + (q.tdx[t] - q.dx0)) * pix_bytes : 0;
  }
}

// The split over the input channels (Args::ks) of a launch of `nwg` tiles: as
// many splits as bring the launch to `target` workgroups (512: ~2 per CU; <= 0:
// never), at least two chunks of 32 channels each.
static inline int conv_splits(int cin, long nwg, long target) {
  const int nch = cin / 32;
  if (target <= 0 || nch < 4 || nwg <= 0 || nwg * 2 > target) return 1;
  long ks = target / nwg;
  if (ks > nch / 2) ks = nch / 2;
  if (ks > 16) ks = 16;
  return ks < 2 ? 1 : (int)ks;
}

struct ConvPlan {
  int rw, nct, ks;
  size_t lds;
  dim3 grid;   // (grid.z without the splits)
};

// shape(k, &rw, &nct, &lds): the precision's tile shape; grid_limit_rc: its code
// for a grid over 65535 in y or z.
template <class Args, class Shape>
int conv_plan(Args& k, Shape shape, int grid_limit_rc, long split_target, ConvPlan* p) {
  if (!shape(k, &p->rw, &p->nct, &p->lds)) return LSI_EUNSUPPORTED;
  const int th = 4 * p->rw, bn = 16 * p->nct;
  int oh = 0, ow = 0;
  for (int c = 0; c < k.ncls; ++c) {
    oh = k.cls[c].OHt > oh ? k.cls[c].OHt : oh;
    ow = k.cls[c].OWt > ow ? k.cls[c].OWt : ow;
  }
  p->ks = 1;
  p->grid = dim3(0, 0, 0);
  if (oh <= 0 || ow <= 0) return LSI_OK;
  p->grid = dim3((ow + 15) / 16, (oh + th - 1) / th, k.ncls * k.N * (k.Cout / bn));
  if (p->grid.z > 65535 || p->grid.y > 65535) return grid_limit_rc;
  p->ks = conv_splits(k.Cin, (long)p->grid.x * p->grid.y * p->grid.z, split_target);
  if ((long)p->grid.z * p->ks > 65535) p->ks = 1;
  return LSI_OK;
}

template <class Args>
size_t conv_part_bytes(const Args& k, int ks) {
  return ks > 1 ? (size_t)ks * k.N * k.OHF * k.OWF * k.Cout * sizeof(float) : 0;
}

// The planned split is taken when the caller's workspace holds its slabs
// (k.ks, k.part, grid->z); else the launch runs unsplit.
template <class Args>
void conv_adopt_split(Args& k, const ConvPlan& pl, void* workspace, size_t workspace_bytes,
                      dim3* grid) {
  k.ks = 1;
  k.part = nullptr;
  if (pl.ks > 1 && workspace && !((uintptr_t)workspace & 15) &&
      workspace_bytes >= conv_part_bytes(k, pl.ks)) {
    k.ks = pl.ks;
    k.part = (float*)workspace;
    grid->z *= pl.ks;
  }
}

// lsi_conv2d[_f32]_pack_job.  desc_ok, need: the precision's word on the
// descriptor and its packed size in bytes.
template <class Args>
int conv_pack_job(const LsiConvDesc* d, int32_t mode, const float* weight, void* packed,
                  size_t packed_bytes, LsiPackJob* job, int32_t* nblocks, bool desc_ok,
                  size_t need) {
  if (!d || !weight || !packed || !job || !nblocks) return LSI_ENULL;
  if (!desc_ok) return LSI_EUNSUPPORTED;
  if (mode < 0 || mode > 3) return LSI_EINVAL;
  if ((uintptr_t)packed & 15) return LSI_EINVAL;
  if (packed_bytes < need) return LSI_EWORKSPACE;
  Args k;
  memset(job, 0, sizeof(*job));
  conv_classes(d, mode & 1, k, job->tap);
  job->w = weight; job->dst = packed;
  job->D0 = d->Cout; job->D1 = d->Cin; job->khw = d->KH * d->KW; job->tr = mode;
  job->ntaps = d->KH * d->KW;
  job->block0 = 0;
  *nblocks = ((d->Cin + 31) / 32) * ((d->Cout + 31) / 32);
  return LSI_OK;
}

// ---- weight gradient ----------------------------------------------------------
// The tap table of a weight gradient (every tap of the kernel, ky * KW + kx
// order) and its groups of `group` taps.
template <class Args>
void conv_wgrad_taps(const LsiConvDesc* d, Args& k, int group) {
  k.ntaps = d->KH * d->KW;
  k.khw = k.ntaps;
  k.ntg = (k.ntaps + group - 1) / group;
  int nt = 0;
  for (int y = 0; y < d->KH; ++y)
    for (int x = 0; x < d->KW; ++x) {
      k.tdy[nt] = (signed char)(y - d->pad_t);
      k.tdx[nt] = (signed char)(x - d->pad_l);
      ++nt;
    }
  k.dy0 = -d->pad_t; k.dx0 = -d->pad_l;
}

// Stages of `th` output rows (k.TH, k.nrs) in strips of 32 columns (k.nstrip),
// and the workgroups per strip: as many as keep the whole launch resident (512
// = two per CU; chan_wgs: the workgroups of one pixel block), at most one per
// stage, the partial sums within part_cap bytes.
template <class Args>
long conv_wgrad_ps(const LsiConvDesc* d, Args& k, int th, long chan_wgs, size_t part_cap) {
  k.TH = th;
  k.nstrip = (d->OW + 31) / 32;
  k.nrs = (d->OH + th - 1) / th;
  const size_t wbytes = (size_t)d->Cout * d->Cin * k.khw * sizeof(float);
  const long nstage = (long)d->N * k.nrs;
  long ps = 512 / (chan_wgs * k.nstrip);
  if (ps < 1) ps = 1;
  if (ps > nstage) ps = nstage;
  while (ps > 1 && (size_t)(ps * k.nstrip) * wbytes > part_cap) --ps;
  return ps;
}

// g_weight (cl: with torch's channels-last strides) = the sum of the nblk
// partials [blk][tap][Cout][Cin] in `part`, in block order: the two fold
// kernels of lsi_conv_wgrad_igemm.hip, which read and write fp32 whatever the
// precision of the convolution.
int lsi_conv_wgrad_fold(const float* part, int nblk, const LsiConvDesc* d, float* g_weight,
                        int cl, hipStream_t stream);

// The prediction head's weight + bias gradient (lsi_conv_wgrad.hip; called by
// lsi_conv3x3_pred_bwd, lsi_conv.hip): g_wb = [cout * 288 + cout], written.
size_t lsi_pred_wgrad_workspace_bytes(int N, int H, int W, int cout);
int lsi_pred_wgrad_launch(int N, int H, int W, int cout, const float* g, const float* y,
                          const void* x, float* g_wb, void* workspace, size_t workspace_bytes,
                          hipStream_t stream);

#endif  // LSI_CONV_HOST_H_
