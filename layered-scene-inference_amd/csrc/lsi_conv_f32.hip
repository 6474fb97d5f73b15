// The convolutions of the encoder-decoder and the LDI heads in EXACT fp32 on
// the matrix cores (gfx950, v_mfma_f32_16x16x4_f32: a k-ordered chain of f32
// fmas, no reduced-precision inputs): reference nets.py:29-70, 73-114, 244-348
// -- slim.conv2d (k x k, stride 1 | 2, TF `SAME` padding) and
// slim.conv2d_transpose (4 x 4, stride 2) on fp32 channels-last activations,
// as the reference computes them.  The fp32 counterparts of
// lsi_conv_igemm.hip (forward and data gradient) and lsi_conv_wgrad_igemm.hip
// (weight gradient), with the same tap lists, parity classes, two-tensor skip
// inputs, split over the input channels and deterministic folds; only the
// operand staging and the MFMA change.
//
// Forward / data gradient (`conv_f32_kernel`).  The weights are the A operand
// (16 output channels x K), the pixels the B operand (16 pixels x K); lane l
// holds A[co l & 15][k = l >> 4] and B[k = l >> 4][pixel l & 15], and its
// accumulator is output channels 4 (l >> 4) .. + 3 of pixel l & 15 -- the C/D
// layout of the bf16 MFMA, so the channels-last epilogue is unchanged.  A chunk
// of 32 input channels is 8 MFMAs per tap: one ds_read_b128 per lane and
// operand hands lane l channels 16 h + 4 (l >> 4) + e, e = 0..3, and MFMA (h, e)
// takes element e -- the same channel-to-k-slot permutation for A and B, so
// the 8 MFMAs together cover the 32 channels once.  A staged pixel (or weight
// row) is 128 bytes + 16 of padding.
//
// Weight gradient (`conv_wgrad_f32_kernel`): per tap a GEMM with M = Cout,
// N = Cin, K = output pixels.  With one fp32 value per lane, a fragment row is
// 16 consecutive channels of ONE pixel (lane l: channel l & 15 of pixel
// l >> 4 of the K step) -- a plain ds_read_b32 out of the pixel-major LDS rows,
// no transposing read.  Partial sums per workgroup, folded in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lsi_hip.h"
#include "lsi_common.h"
#include "lsi_conv_device.h"
#include "lsi_conv_host.h"

using namespace lsi;

namespace {

constexpr int F_MAXTAPS = 49;
constexpr int F_PIX = 144;   // bytes per staged pixel / weight row (128 + 16 of padding)
constexpr int F_MAXP = 16;   // 16-byte pieces per thread of a staged patch (<= 512 pixels)
constexpr size_t F_LDS_CAP = 80 * 1024;   // two workgroups per CU

// One tap list = one class of output pixels (lsi_conv_igemm.hip: IgClass).
struct FClass {
  int ntaps, dy0, dx0;
  int ooy, oox;
  int OHt, OWt;
  int wofs;
  int toff[F_MAXTAPS + 1];   // patch byte offset of every tap
  signed char tdy[F_MAXTAPS + 3], tdx[F_MAXTAPS + 3];
};
struct FArgs {
  const float* x;     // N x H x W x Cin (C1 channels of it when x2 != nullptr)
  const float* x2;    // channels [C1, Cin) (a skip connection's second tensor)
  int C1;
  float* out2;        // output channels [O1, Cout) (a data gradient into two tensors)
  int O1;
  const float* wp;    // [taps of all classes][Cout][Cin]
  float* out;         // N x OHF x OWF x Cout
  int N, H, W, Cin, Cout;
  int s, os;
  int OHF, OWF;
  int G;              // taps per weight stage (the last stage may hold fewer)
  int PH, PW;
  int ncls;
  float* part;        // split over the input channels: part[ksi][n][y][x][co]
  int ks;
  FClass cls[4];
};

// RW: pixel rows per wave; NCT: tiles of 16 output channels (BN = 16 NCT); G:
// taps per weight stage.  Workgroup = 4 waves = (4 RW) x 16 output pixels x BN
// output channels; per unit (chunk of 32 input channels, group of G taps) the
// patch and the weights are staged in LDS, the next unit's loads in flight.
template <int RW, int NCT, int G>
__global__ __launch_bounds__(256) void conv_f32_kernel(FArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char f_smem[];
  constexpr int TH = 4 * RW, BN = 16 * NCT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pxl = lane & 15, kg = lane >> 4;
  const int ncb = a.Cout / BN;
  const int zz = blockIdx.z / ncb;
  const int co0 = (blockIdx.z - zz * ncb) * BN;
  const int ksi = zz / (a.ncls * a.N);
  const int zc = zz - ksi * (a.ncls * a.N);
  const int ci_ = zc / a.N, n = zc - ci_ * a.N;
  const FClass& k = a.cls[ci_];
  const int i0 = blockIdx.y * TH, j0 = blockIdx.x * 16;
  if (i0 >= k.OHt || j0 >= k.OWt) return;   // (the grid covers the largest class)
  const int PW = a.PW, npix = a.PH * PW;
  unsigned char* const patch = f_smem;
  unsigned char* const wts = f_smem + (size_t)npix * F_PIX;

  // the patch pieces this thread stages (16 bytes: pixel, eighth of its 32
  // channels): pixel index into the input, -1 outside it
  int goff[F_MAXP];
  const int npiece = npix * 8;
  {
    const int iy0 = i0 * a.s + k.dy0, ix0 = j0 * a.s + k.dx0;
#pragma unroll
    for (int q = 0; q < F_MAXP; ++q) {
      const int idx = tid + 256 * q;
      const int pix = idx >> 3;
      const int py = pix / PW, px = pix - py * PW;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool ok = idx < npiece && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      goff[q] = ok ? ((n * a.H + iy) * a.W + ix) : -1;
    }
  }
  f32x4 acc[RW][NCT];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const unsigned b_lane =
      (unsigned)((wave * RW * a.s) * PW + pxl * a.s) * F_PIX + (unsigned)kg * 16u;
  const unsigned b_row = (unsigned)(a.s * PW) * F_PIX;
  const int ntaps = k.ntaps;
  const float* const wp = a.wp + (size_t)k.wofs * a.Cout * a.Cin;
  const unsigned a_lane = (unsigned)pxl * F_PIX + (unsigned)kg * 16u;

  constexpr int NWP = G * BN * 8, WB = (NWP + 255) / 256;
  const int ngrp = (ntaps + G - 1) / G;
  const int nch = a.Cin / 32;
  const int ch_lo = ksi * nch / a.ks, ch_hi = (ksi + 1) * nch / a.ks;
  const int nunit = (ch_hi - ch_lo) * ngrp;
  u32x4 pv[F_MAXP], wv[WB];
  auto fetch = [&](int u) {
    const int chl = u / ngrp, gi = u - chl * ngrp;
    const int c0 = (ch_lo + chl) * 32, t0 = gi * G;
    if (gi == 0) {
      const bool second = c0 >= a.C1;
      const float* const xb = second ? a.x2 + (c0 - a.C1) : a.x + c0;
      const int pitch = second ? a.Cin - a.C1 : a.C1;
#pragma unroll
      for (int q = 0; q < F_MAXP; ++q) {
        pv[q] = zero4;
        if (tid + 256 * q < npiece && goff[q] >= 0)
          pv[q] = *reinterpret_cast<const u32x4*>(xb + (size_t)goff[q] * pitch +
                                                  4 * ((tid + 256 * q) & 7));
      }
    }
    const float* const wsrc = wp + ((size_t)t0 * a.Cout + co0) * a.Cin + c0;
    const int nreal = (ntaps - t0) * BN * 8;
#pragma unroll
    for (int q = 0; q < WB; ++q) {
      const int idx = tid + 256 * q;
      wv[q] = zero4;
      if (idx < NWP && idx < nreal) {
        const int e = idx & 7, co = (idx >> 3) & (BN - 1), t = idx / (8 * BN);
        wv[q] = *reinterpret_cast<const u32x4*>(wsrc + ((size_t)t * a.Cout + co) * a.Cin + 4 * e);
      }
    }
  };
  auto stash = [&](int u) {
    if (u % ngrp == 0) {
#pragma unroll
      for (int q = 0; q < F_MAXP; ++q) {
        const int idx = tid + 256 * q;
        if (idx < npiece)
          *reinterpret_cast<u32x4*>(patch + (size_t)(idx >> 3) * F_PIX + (idx & 7) * 16) = pv[q];
      }
    }
#pragma unroll
    for (int q = 0; q < WB; ++q) {
      const int idx = tid + 256 * q;
      if (idx < NWP) {
        const int e = idx & 7, co = (idx >> 3) & (BN - 1), t = idx / (8 * BN);
        *reinterpret_cast<u32x4*>(wts + (size_t)(t * BN + co) * F_PIX + e * 16) = wv[q];
      }
    }
  };
  if (nunit > 0) fetch(0);
  for (int u = 0; u < nunit; ++u) {
    __syncthreads();  // (the previous unit's fragments have been read)
    stash(u);
    __syncthreads();
    if (u + 1 < nunit) fetch(u + 1);   // in flight while this unit is multiplied
    const int t0 = (u % ngrp) * G;
#pragma unroll
    for (int t = 0; t < G; ++t) {
      if (t0 + t >= ntaps) break;   // (wave-uniform: the class's last stage)
      const unsigned char* const bp = patch + b_lane + (unsigned)k.toff[t0 + t];
      // (the tap's 32 channels into a fresh accumulator, added to the running sum
      // after: chains of 32 products instead of one chain over all taps and
      // channels -- 3x less rounding error on the 1600-term sums of a 5 x 5 layer
      // over 64 channels, where one chain was 3x the library's)
      f32x4 tacc[RW][NCT];
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < NCT; ++c) tacc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 af[NCT];
#pragma unroll
        for (int c = 0; c < NCT; ++c)
          af[c] = *reinterpret_cast<const f32x4*>(wts + (size_t)(t * BN + 16 * c) * F_PIX +
                                                  a_lane + 64 * h);
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const f32x4 bf = *reinterpret_cast<const f32x4*>(bp + r * b_row + 64 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < NCT; ++c)
              tacc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[c][e], bf[e], tacc[r][c], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[r][c] += tacc[r][c];
    }
  }
  // ---- channels-last stores: lane = 4 output channels of one pixel -----------
  const int j = j0 + pxl;
  if (j >= k.OWt) return;
  if (a.ks > 1) {
    float* const pb = a.part + (size_t)ksi * a.N * a.OHF * a.OWF * a.Cout;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int i = i0 + wave * RW + r;
      if (i < k.OHt) {
        float* const o = pb + (((size_t)n * a.OHF + (size_t)(i * a.os + k.ooy)) * a.OWF +
                               (j * a.os + k.oox)) * a.Cout + co0 + 4 * kg;
#pragma unroll
        for (int c = 0; c < NCT; ++c) *reinterpret_cast<f32x4*>(o + 16 * c) = acc[r][c];
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int i = i0 + wave * RW + r;
    if (i < k.OHt) {
      const bool o_second = co0 >= a.O1;
      float* const o = (o_second ? a.out2 + (co0 - a.O1) : a.out + co0) +
          (((size_t)n * a.OHF + (size_t)(i * a.os + k.ooy)) * a.OWF + (j * a.os + k.oox)) *
              (o_second ? a.Cout - a.O1 : a.O1) + 4 * kg;
#pragma unroll
      for (int c = 0; c < NCT; ++c) *reinterpret_cast<f32x4*>(o + 16 * c) = acc[r][c];
    }
  }
}

// out = slab 0 + slab 1 + ... in that order (fp32, into one or two tensors).
// Block = 64 quads of channels x 4 pixels; grid.x = pixel blocks, grid.y =
// blocks of 256 channels.
struct FFoldArgs {
  const float* part;
  float* out;
  float* out2;
  int O1, Cout, ks;
  long npix;   // pixels of the whole output (N x OHF x OWF)
  long per;    // pixels per block
};
__global__ __launch_bounds__(256) void conv_f32_fold_kernel(FFoldArgs a) {
  const int co = 4 * ((int)blockIdx.y * 64 + (int)threadIdx.x);
  if (co >= a.Cout) return;
  const long p0 = (long)blockIdx.x * a.per;
  const long p1 = p0 + a.per < a.npix ? p0 + a.per : a.npix;
  const size_t slab = (size_t)a.npix * a.Cout;
  const bool second = co >= a.O1;
  float* const ob = second ? a.out2 + (co - a.O1) : a.out + co;
  const int pitch = second ? a.Cout - a.O1 : a.O1;
  for (long p = p0 + threadIdx.y; p < p1; p += 4) {
    const float* const src = a.part + (size_t)p * a.Cout + co;
    f32x4 v = *reinterpret_cast<const f32x4*>(src);
    for (int k = 1; k < a.ks; ++k) v += *reinterpret_cast<const f32x4*>(src + k * slab);
    *reinterpret_cast<f32x4*>(ob + (size_t)p * pitch) = v;
  }
}

// The weights in the kernel's operand order, fp32 (lsi_conv_device.h's pack; D0,
// D1 multiples of 16: the edge tiles are guarded).
__global__ __launch_bounds__(256) void conv_f32_pack_kernel(LsiPackJob a) {
  __shared__ float tile[PACK_TC][32][33];
  pack_tile<float, true>(a, blockIdx.x, blockIdx.y, tile);   // block (x, y) = tile (d1, d0) / 32
}
__global__ __launch_bounds__(256) void conv_f32_pack_many_kernel(const LsiPackJob* jobs, int njobs) {
  __shared__ float tile[PACK_TC][32][33];
  __shared__ int which;
  pack_job_tile<float, true>(jobs, njobs, tile, &which);
}

// Tile shape: the tallest row block (<= 4 rows per wave) whose patch and one
// weight stage fit the LDS share; G: the most taps per stage that fit.
bool f_shape(FArgs& k, int* rw_out, int* nct_out, size_t* lds_out) {
  const int nct = (k.Cout % 64 == 0) ? 4 : (k.Cout % 32 == 0) ? 2 : 1;
  const int bn = 16 * nct;
  const ConvSpans sp = conv_tap_spans(k);
  const int spany = sp.spany, spanx = sp.spanx, maxoh = sp.maxoh;
  k.PW = 15 * k.s + spanx;
  for (int rw = 4; rw >= 1; rw >>= 1) {
    if (rw > 1 && 4 * (rw / 2) >= maxoh) continue;   // (a shorter block covers the rows)
    // (shorter tiles while the launch would leave CUs without a workgroup)
    if (rw > 1 && (long)((maxoh + 4 * rw - 1) / (4 * rw)) * ((k.cls[0].OWt + 15) / 16) * k.N *
                          k.ncls * (k.Cout / bn) < 512)
      continue;
    k.PH = (4 * rw - 1) * k.s + spany;
    if (k.PH * k.PW * 8 > 256 * F_MAXP) continue;
    const size_t patch = (size_t)k.PH * k.PW * F_PIX;
    int g = 0;
    for (int gc = 8; gc >= 2; gc >>= 1)
      if (patch + (size_t)gc * bn * F_PIX <= F_LDS_CAP) { g = gc; break; }
    if (!g) continue;
    k.G = g;
    conv_tap_offsets(k, F_PIX, F_MAXTAPS + 1);
    *rw_out = rw; *nct_out = nct;
    *lds_out = patch + (size_t)g * bn * F_PIX;
    return true;
  }
  return false;
}

// The plan of a launch: split over the input channels towards 512 workgroups.
int f_plan(FArgs& k, ConvPlan* p) { return conv_plan(k, f_shape, LSI_EUNSUPPORTED, 512, p); }

int f_launch(FArgs& k, hipStream_t stream, void* workspace, size_t workspace_bytes) {
  ConvPlan pl;
  const int prc = f_plan(k, &pl);
  if (prc != LSI_OK) return prc;
  if (pl.grid.x == 0) return LSI_OK;
  const int rw = pl.rw, nct = pl.nct;
  dim3 grid = pl.grid;
  conv_adopt_split(k, pl, workspace, workspace_bytes, &grid);
  const void* fn = nullptr;
#define F_CASE(R, C, GG) \
  if (rw == R && nct == C && k.G == GG) fn = (const void*)conv_f32_kernel<R, C, GG>
#define F_CASES(GG) \
  F_CASE(4, 4, GG); F_CASE(2, 4, GG); F_CASE(1, 4, GG); \
  F_CASE(4, 2, GG); F_CASE(2, 2, GG); F_CASE(1, 2, GG); \
  F_CASE(4, 1, GG); F_CASE(2, 1, GG); F_CASE(1, 1, GG)
  F_CASES(8); F_CASES(4); F_CASES(2);
#undef F_CASES
#undef F_CASE
  if (!fn) return LSI_EINVAL;
  {
    static const char* dbg = getenv("LSI_IG_DEBUG");   // (experiments: the plan of every call)
    if (dbg)
      fprintf(stderr, "f32 N%d %dx%d cin %d cout %d s%d os%d ncls %d taps %d: RW %d NCT %d G %d grid %u x %u x %u (ks %d), lds %zu\n",
              k.N, k.H, k.W, k.Cin, k.Cout, k.s, k.os, k.ncls, k.cls[0].ntaps, rw, nct, k.G,
              grid.x, grid.y, grid.z, k.ks, pl.lds);
  }
  if (lsi_ensure_dynamic_lds(fn, pl.lds) != LSI_OK) return LSI_ELAUNCH;
  void* kargs[1] = {&k};
  if (hipLaunchKernel(fn, grid, dim3(256), kargs, pl.lds, stream) != hipSuccess) return LSI_ELAUNCH;
  if (hipGetLastError() != hipSuccess) return LSI_ELAUNCH;
  if (k.ks > 1) {
    FFoldArgs f;
    f.part = k.part; f.out = k.out; f.out2 = k.out2; f.O1 = k.O1; f.Cout = k.Cout; f.ks = k.ks;
    f.npix = (long)k.N * k.OHF * k.OWF;
    const int cb = (k.Cout + 255) / 256;
    long nb = 512 / cb;
    if (nb > (f.npix + 3) / 4) nb = (f.npix + 3) / 4;
    if (nb < 1) nb = 1;
    f.per = (f.npix + nb - 1) / nb;
    nb = (f.npix + f.per - 1) / f.per;
    hipLaunchKernelGGL(conv_f32_fold_kernel, dim3((unsigned)nb, cb), dim3(64, 4), 0, stream, f);
    if (hipGetLastError() != hipSuccess) return LSI_ELAUNCH;
  }
  return LSI_OK;
}

// What the fp32 kernels take: the kernel's input channels (Cin forward, Cout
// data gradient) multiples of 32, its output channels of 16.
bool f_desc_ok(const LsiConvDesc* d) {
  if (!conv_desc_common(d, 16)) return false;
  // (the output grid must be the one the padding implies: every output pixel reads
  // at least one input pixel)
  if ((int64_t)(d->OH - 1) * d->stride - d->pad_t >= d->H) return false;
  if ((int64_t)(d->OW - 1) * d->stride - d->pad_l >= d->W) return false;
  return true;
}

bool f_mode_ok(const LsiConvDesc* d, int mode) {
  return f_desc_ok(d) && (mode == 0 || d->Cout % 32 == 0);
}

// ---- weight gradient ------------------------------------------------------------
constexpr int FW_GT = 9;      // taps per workgroup
constexpr int FW_PB = 5;      // (tap, 16-channel tile) pairs per wave: 4 waves x 5 >= 2 x 9
constexpr size_t FW_PART_CAP = 96u << 20;   // partial sums: at most this many bytes

// LDS floats per staged input pixel / gy pixel: the four k slots of a fragment
// (pixels 0..3 of the K step, S input pixels apart) fall into the two halves of
// the 32 banks of a ds_read_b32 lane group -- pitch x S = 16 (mod 32)
constexpr int fw_xs(int s) { return s == 1 ? 48 : 40; }
constexpr int fw_gs(int bn) { return bn == 16 ? 48 : bn + 16; }

struct FwArgs {
  const float* x;
  const float* x2;    // channels [C1, Cin) (a skip connection's second tensor)
  int C1;
  const float* gy;    // N x OH x OW x Cout
  float* part;        // [pixel blocks][khw][Cout][Cin]
  int N, H, W, Cin, OH, OW, Cout;
  int khw, ntaps, ntg;
  int dy0, dx0, PH, PW, TH;
  int nstrip, nrs, PS;
  signed char tdy[F_MAXTAPS + 3], tdx[F_MAXTAPS + 3];
};

// Workgroup = (strip of 32 output columns x its share PS of the (image, TH-row)
// stages) x (32 input channels, group of <= 9 taps) x (BN output channels);
// the accumulators (wave: <= 5 (tap, 16-channel) pairs x BN) stay in registers
// for all its stages and leave as one partial sum.
template <int NCT, int S>
__global__ __launch_bounds__(256) void conv_wgrad_f32_kernel(FwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fw_smem[];
  constexpr int BN = 16 * NCT, XS = fw_xs(S), GS = fw_gs(BN), NW = 4, PB = FW_PB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = lane & 15, g = lane >> 4;
  const int PW = a.PW, npix = a.PH * PW, TH = a.TH;
  float* const xs = reinterpret_cast<float*>(fw_smem);
  float* const gs = xs + (size_t)npix * XS;

  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int st = bx % a.nstrip, slot = bx / a.nstrip;
  const int tg = by % a.ntg, c0 = (by / a.ntg) * 32;
  const int o0 = bz * BN;
  const int t0 = tg * FW_GT, nt = min(FW_GT, a.ntaps - t0);
  const int j0 = st * 32;
  const int nstage = a.N * a.nrs;

  // patch pieces of this thread (pixel, eighth of the 32 channels): row of the
  // patch and element offset in image 0 for the block's first stage; -1 outside
  int prow[F_MAXP], goff[F_MAXP];
  const int npiece = npix * 8;
  const bool second = c0 >= a.C1;
  const float* const xsrc = second ? a.x2 + (c0 - a.C1) : a.x + c0;
  const int xpitch = second ? a.Cin - a.C1 : a.C1;
  {
    const int ix0 = j0 * S + a.dx0;
#pragma unroll
    for (int q = 0; q < F_MAXP; ++q) {
      const int idx = tid + 256 * q;
      const int pix = idx >> 3, e = idx & 7;
      const int py = pix / PW, px = pix - py * PW;
      const int ix = ix0 + px;
      const bool ok = idx < npiece && ix >= 0 && ix < a.W;
      prow[q] = ok ? py : -1;
      goff[q] = (py * a.W + ix) * xpitch + 4 * e;
    }
  }
  f32x4 acc[PB][NCT];
#pragma unroll
  for (int j = 0; j < PB; ++j)
#pragma unroll
    for (int m = 0; m < NCT; ++m) acc[j][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // the wave's pairs: LDS float offset of (tap, channel tile) in the patch, plus
  // this lane's k slot (pixel g of a K step) and channel
  int poff[PB];
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int p = wave + j * NW;
    const int tl = p >> 1, c = p & 1;
    poff[j] = -1;
    if (tl < nt)
      poff[j] = ((a.tdy[t0 + tl] - a.dy0) * PW + (a.tdx[t0 + tl] - a.dx0)) * XS + 16 * c +
                g * S * XS + t;
  }

  for (int sg = slot; sg < nstage; sg += a.PS) {
    const int ni = sg / a.nrs, i0 = (sg - ni * a.nrs) * TH;
    __syncthreads();  // (the previous stage's fragments have been read)
    {
      const int iy0 = i0 * S + a.dy0;
      const long shift = ((long)iy0 + (long)ni * a.H) * a.W * xpitch;
      u32x4 pv[F_MAXP];
#pragma unroll
      for (int q = 0; q < F_MAXP; ++q) {
        pv[q] = zero4;
        const int iy = iy0 + prow[q];
        if (prow[q] >= 0 && iy >= 0 && iy < a.H)
          pv[q] = *reinterpret_cast<const u32x4*>(xsrc + (long)goff[q] + shift);
      }
#pragma unroll
      for (int q = 0; q < F_MAXP; ++q) {
        const int idx = tid + 256 * q;
        if (idx < npiece)
          *reinterpret_cast<u32x4*>(xs + (size_t)(idx >> 3) * XS + (idx & 7) * 4) = pv[q];
      }
    }
    {
      constexpr int PPX = BN / 4;        // 16-byte pieces per gy pixel
      const int ngp = TH * 32 * PPX;
      for (int base = 0; base < ngp; base += 256 * 8) {
        u32x4 gv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int piece = base + tid + 256 * q;
          const int pp = piece / PPX, part = piece - pp * PPX;
          const int r = pp >> 5, c = pp & 31;
          const int oy = i0 + r, ox = j0 + c;
          gv[q] = zero4;
          if (piece < ngp && oy < a.OH && ox < a.OW)
            gv[q] = *reinterpret_cast<const u32x4*>(
                a.gy + (((size_t)ni * a.OH + oy) * a.OW + ox) * a.Cout + o0 + 4 * part);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int piece = base + tid + 256 * q;
          const int pp = piece / PPX, part = piece - pp * PPX;
          if (piece < ngp) *reinterpret_cast<u32x4*>(gs + (size_t)pp * GS + 4 * part) = gv[q];
        }
      }
    }
    __syncthreads();
    const int nrow = min(TH, a.OH - i0);
    for (int r = 0; r < nrow; ++r) {
      // (a row's 32 pixels into a fresh accumulator, added to the running sum
      // after: chains of 32 products, not one over all the block's pixels)
      f32x4 racc[PB][NCT];
#pragma unroll
      for (int j = 0; j < PB; ++j)
#pragma unroll
        for (int m = 0; m < NCT; ++m) racc[j][m] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* const grow = gs + (size_t)(r * 32 + g) * GS + t;
      const float* const xrow = xs + (size_t)(r * S) * PW * XS;
#pragma unroll 2
      for (int kstep = 0; kstep < 8; ++kstep) {
        float af[NCT];
#pragma unroll
        for (int m = 0; m < NCT; ++m) af[m] = grow[(size_t)(4 * kstep) * GS + 16 * m];
        const float* const xk = xrow + 4 * kstep * S * XS;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
          if (poff[j] >= 0) {   // (wave-uniform)
            const float bf = xk[poff[j]];
#pragma unroll
            for (int m = 0; m < NCT; ++m)
              racc[j][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m], bf, racc[j][m], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PB; ++j)
#pragma unroll
        for (int m = 0; m < NCT; ++m) acc[j][m] += racc[j][m];
    }
  }
  // accumulator of lane (t, g), register r: co = o0 + 16 m + 4 g + r, ci = c0 + 16 c + t
  const size_t nout = (size_t)a.Cout * a.Cin * a.khw;
  float* const out = a.part + (size_t)bx * nout;
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int p = wave + j * NW;
    const int tl = p >> 1, c = p & 1;
    if (tl < nt) {
      const int tap = t0 + tl;
#pragma unroll
      for (int m = 0; m < NCT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          out[((size_t)tap * a.Cout + o0 + 16 * m + 4 * g + r) * a.Cin + c0 + 16 * c + t] =
              acc[j][m][r];
    }
  }
}

// Rows per stage, pixel blocks, LDS bytes; false: not taken (partial sums over
// the cap: small maps with many channels stay on the library).
bool fw_plan(const LsiConvDesc* d, FwArgs& k, int* nct_out, size_t* lds_out, int* nblk_out) {
  const int nct = (d->Cout % 64 == 0) ? 4 : (d->Cout % 32 == 0) ? 2 : 1;
  const int bn = 16 * nct, gsz = fw_gs(bn), s = d->stride, xs = fw_xs(s);
  conv_wgrad_taps(d, k, FW_GT);
  k.PW = 31 * s + d->KW;
  int th = 0;
  for (int cand = 8; cand >= 1; cand >>= 1) {
    const int ph = (cand - 1) * s + d->KH;
    if (ph * k.PW * 8 > 256 * F_MAXP) continue;
    const size_t lds = ((size_t)ph * k.PW * xs + (size_t)cand * 32 * gsz) * sizeof(float);
    if (lds > F_LDS_CAP) continue;
    th = cand; k.PH = ph; *lds_out = lds;
    break;
  }
  if (!th) return false;
  const long chan_wgs = (long)(d->Cin / 32) * k.ntg * (d->Cout / bn);
  const size_t wbytes = (size_t)d->Cout * d->Cin * k.khw * sizeof(float);
  const long ps = conv_wgrad_ps(d, k, th, chan_wgs, FW_PART_CAP);
  k.PS = (int)ps;
  const long nblk = ps * k.nstrip;
  if ((size_t)nblk * wbytes > FW_PART_CAP || nblk > 65535 * 32L) return false;
  *nblk_out = (int)nblk;
  *nct_out = nct;
  return true;
}

}  // namespace

extern "C" int lsi_conv2d_f32_supported(const LsiConvDesc* d) { return f_desc_ok(d) ? 1 : 0; }

extern "C" size_t lsi_conv2d_f32_packed_bytes(const LsiConvDesc* d) {
  if (!f_desc_ok(d)) return 0;
  return (size_t)d->KH * d->KW * d->Cin * d->Cout * sizeof(float);
}

extern "C" int lsi_conv2d_f32_pack_job(const LsiConvDesc* d, int32_t mode, const float* weight,
                                       void* packed, size_t packed_bytes, LsiPackJob* job,
                                       int32_t* nblocks) {
  return conv_pack_job<FArgs>(d, mode, weight, packed, packed_bytes, job, nblocks, f_desc_ok(d),
                              lsi_conv2d_f32_packed_bytes(d));
}

extern "C" int lsi_conv2d_f32_pack(const LsiConvDesc* d, int32_t mode, const float* weight,
                                   void* packed, size_t packed_bytes, lsi_stream_t stream_) {
  LsiPackJob p;
  int32_t nb;
  const int rc = lsi_conv2d_f32_pack_job(d, mode, weight, packed, packed_bytes, &p, &nb);
  if (rc != LSI_OK) return rc;
  hipLaunchKernelGGL(conv_f32_pack_kernel, dim3((d->Cin + 31) / 32, (d->Cout + 31) / 32),
                     dim3(256), 0, (hipStream_t)stream_, p);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

extern "C" int lsi_conv2d_f32_pack_many(const LsiPackJob* jobs_device, int32_t njobs,
                                        int32_t total_blocks, lsi_stream_t stream_) {
  if (!jobs_device) return LSI_ENULL;
  if (njobs <= 0 || total_blocks <= 0) return LSI_EINVAL;
  hipLaunchKernelGGL(conv_f32_pack_many_kernel, dim3(total_blocks), dim3(256), 0,
                     (hipStream_t)stream_, jobs_device, njobs);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

extern "C" size_t lsi_conv2d_f32_workspace_bytes(const LsiConvDesc* d, int32_t mode) {
  if (mode < 0 || mode > 1 || !f_mode_ok(d, mode)) return 0;
  FArgs k;
  int8_t tap[56];
  conv_classes(d, mode, k, tap);
  k.C1 = k.Cin; k.O1 = k.Cout; k.ks = 1;
  ConvPlan pl;
  if (f_plan(k, &pl) != LSI_OK || pl.grid.x == 0) return 0;
  return conv_part_bytes(k, pl.ks);
}

extern "C" int lsi_conv2d_f32_run(const LsiConvDesc* d, int32_t mode, const LsiConvIO* io,
                                  lsi_stream_t stream) {
  if (!d || !io) return LSI_ENULL;
  if (mode < 0 || mode > 1) return LSI_EINVAL;
  if (!f_mode_ok(d, mode)) return LSI_EUNSUPPORTED;
  if (!io->x || !io->packed || !io->out) return LSI_ENULL;
  if (io->workspace_bytes && !io->workspace) return LSI_ENULL;
  // (batch-norm statistics in the epilogue: not in the fp32 kernels)
  if (io->bn_workspace) return LSI_EUNSUPPORTED;
  if (mode == 0 && io->out2) return LSI_EINVAL;
  if (mode == 1 && io->x2) return LSI_EINVAL;
  if (((uintptr_t)io->x & 15) || ((uintptr_t)io->out & 15) || ((uintptr_t)io->packed & 15))
    return LSI_EUNSUPPORTED;
  FArgs k;
  int8_t tap[56];
  conv_classes(d, mode, k, tap);
  k.x = (const float*)io->x; k.wp = (const float*)io->packed; k.out = (float*)io->out;
  k.C1 = k.Cin;
  k.O1 = k.Cout;
  k.ks = 1;
  if (io->out2) {   // the data gradient as two tensors
    const int bn = (k.Cout % 64 == 0) ? 64 : (k.Cout % 32 == 0) ? 32 : 16;
    if ((uintptr_t)io->out2 & 15) return LSI_EUNSUPPORTED;
    if (io->c1 <= 0 || io->c1 >= k.Cout || io->c1 % bn) return LSI_EINVAL;
    k.out2 = (float*)io->out2;
    k.O1 = io->c1;
  }
  if (io->x2) {     // the input as two tensors
    if ((uintptr_t)io->x2 & 15) return LSI_EUNSUPPORTED;
    if (io->c1 <= 0 || io->c1 >= k.Cin || io->c1 % 32) return LSI_EINVAL;
    k.x2 = (const float*)io->x2;
    k.C1 = io->c1;
  }
  return f_launch(k, (hipStream_t)stream, io->workspace, io->workspace_bytes);
}

extern "C" size_t lsi_conv2d_wgrad_f32_workspace_bytes(const LsiConvDesc* d) {
  if (!f_desc_ok(d)) return 0;
  FwArgs k;
  memset(&k, 0, sizeof(k));
  int nct, nblk;
  size_t lds;
  if (!fw_plan(d, k, &nct, &lds, &nblk)) return 0;
  return (size_t)nblk * d->Cout * d->Cin * d->KH * d->KW * sizeof(float);
}

extern "C" int lsi_conv2d_wgrad_f32(const LsiConvDesc* d, const void* x1, const void* x2,
                                    int32_t c1, const void* gy, float* g_weight,
                                    int32_t weight_layout, void* workspace,
                                    size_t workspace_bytes, lsi_stream_t stream_) {
  if (!d || !x1 || !gy || !g_weight || !workspace) return LSI_ENULL;
  if (!f_desc_ok(d)) return LSI_EUNSUPPORTED;
  if (weight_layout != 0 && weight_layout != 2) return LSI_EINVAL;
  if (((uintptr_t)x1 & 15) || ((uintptr_t)gy & 15) || (x2 && ((uintptr_t)x2 & 15)))
    return LSI_EUNSUPPORTED;
  if ((uintptr_t)workspace & 15) return LSI_EINVAL;
  if (x2 && (c1 <= 0 || c1 >= d->Cin || c1 % 32)) return LSI_EINVAL;
  FwArgs k;
  memset(&k, 0, sizeof(k));
  int nct, nblk;
  size_t lds;
  if (!fw_plan(d, k, &nct, &lds, &nblk)) return LSI_EUNSUPPORTED;
  const size_t nout = (size_t)d->Cout * d->Cin * d->KH * d->KW;
  if (nout >= (1u << 31)) return LSI_EUNSUPPORTED;
  if (workspace_bytes < (size_t)nblk * nout * sizeof(float)) return LSI_EWORKSPACE;
  k.x = (const float*)x1; k.x2 = (const float*)x2; k.C1 = x2 ? c1 : d->Cin;
  k.gy = (const float*)gy; k.part = (float*)workspace;
  k.N = d->N; k.H = d->H; k.W = d->W; k.Cin = d->Cin; k.OH = d->OH; k.OW = d->OW; k.Cout = d->Cout;
  hipStream_t stream = (hipStream_t)stream_;
  const void* fn = nullptr;
  if (nct == 4 && d->stride == 1) fn = (const void*)conv_wgrad_f32_kernel<4, 1>;
  if (nct == 2 && d->stride == 1) fn = (const void*)conv_wgrad_f32_kernel<2, 1>;
  if (nct == 1 && d->stride == 1) fn = (const void*)conv_wgrad_f32_kernel<1, 1>;
  if (nct == 4 && d->stride == 2) fn = (const void*)conv_wgrad_f32_kernel<4, 2>;
  if (nct == 2 && d->stride == 2) fn = (const void*)conv_wgrad_f32_kernel<2, 2>;
  if (nct == 1 && d->stride == 2) fn = (const void*)conv_wgrad_f32_kernel<1, 2>;
  if (!fn) return LSI_EINVAL;
  const dim3 grid(nblk, (d->Cin / 32) * k.ntg, d->Cout / (16 * nct));
  if (grid.y > 65535 || grid.z > 65535) return LSI_EUNSUPPORTED;
  if (lsi_ensure_dynamic_lds(fn, lds) != LSI_OK) return LSI_ELAUNCH;
  void* kargs[1] = {&k};
  if (hipLaunchKernel(fn, grid, dim3(256), kargs, lds, stream) != hipSuccess) return LSI_ELAUNCH;
  if (hipGetLastError() != hipSuccess) return LSI_ELAUNCH;
  return lsi_conv_wgrad_fold(k.part, nblk, d, g_weight, weight_layout, stream);
}
