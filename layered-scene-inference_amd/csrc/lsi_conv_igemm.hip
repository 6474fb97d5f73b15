// Convolutions of the encoder-decoder and the LDI heads as implicit GEMMs on
// the matrix cores (gfx950, v_mfma_f32_16x16x32_bf16, fp32 accumulation):
// reference nets.py:29-70, 73-114, 244-348 -- slim.conv2d (k x k, stride 1 | 2,
// TF `SAME` padding) and slim.conv2d_transpose (4 x 4, stride 2) on bf16
// channels-last activations, forward and data gradient.
//
// One kernel, `conv_igemm_kernel`, computes
//     out[n][i * os + ooy][j * os + oox][co] =
//         sum over taps t, channels ci of  x[n][i * s + dy_t][j * s + dx_t][ci] * Wp[t][co][ci]
// for a list of taps (dy_t, dx_t) with zero outside the input.  Everything the
// network needs is that with a tap list:
//   * forward, stride s:       dy = ky - pad_t, dx = kx - pad_l, os = 1;
//   * data gradient, stride 1: the same sum over the incoming gradient with
//     dy = pad_t - ky and the channel roles swapped (Wp[t][ci][co]);
//   * data gradient, stride 2 (= the forward of a transposed convolution): the
//     input pixels of one parity class (iy, ix) = (2 i + p, 2 j + q) receive
//     only the taps with ky = p + pad_t (mod 2), from gradient pixel
//     i + (p + pad_t - ky) / 2: four launches, each a stride-1 sum over a
//     sub-kernel (2 x 2 taps for the 4 x 4 transposed convolutions) writing
//     every second pixel (os = 2) -- no zero-stuffed input, no wasted products;
//   * the data gradient of a transposed convolution is the forward with s = 2.
//
// Layout.  One pixel's 32 consecutive channels are 64 contiguous bytes = the
// K of ONE MFMA.  The weights are the A operand (16 output channels x 32 input
// channels), the pixels the B operand (lane l: pixel l & 15, channels
// 8 (l >> 4) .. + 7), so that the accumulator of lane l is four consecutive
// output channels of one pixel: channels-last stores without a transpose.
//
// Workgroup = 4 waves = a tile of (4 RW) rows x 16 columns of output pixels x BN
// output channels (BN = 64 | 32); wave w owns rows w RW .. + RW - 1.  Per chunk
// of 32 input channels the workgroup stages the input patch the tile's taps
// reach ((TH - 1) s + span rows, pixels 80 bytes apart: the 16 lanes of a
// fragment read then fall into 16 different 16-byte bank groups) and, per group
// of <= G taps, the weights [tap][co][32 ci] (rows 80 bytes apart) in LDS;
// every tap is then RW + BN / 16 fragment reads for RW * BN / 16 MFMAs.  Two or
// three workgroups share a CU (<= 80 KB of LDS each): one stages while another
// multiplies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lsi_hip.h"
#include "lsi_bn_ws.h"
#include "lsi_common.h"
#include "lsi_conv_device.h"
#include "lsi_conv_host.h"

using namespace lsi;

namespace {

constexpr int IG_MAXTAPS = 49;
constexpr int IG_PIX = 80;  // bytes per staged pixel / weight row (64 + 16 of padding)

// One tap list = one class of output pixels: all of them (forward, stride-1
// data gradient) or one parity class of a stride-2 data gradient.
struct IgClass {
  int ntaps, dy0, dx0;   // taps; smallest dy, dx
  int ooy, oox;          // output pixel of (i, j): (i * os + ooy, j * os + oox)
  int OHt, OWt;          // output grid (i, j) of the class
  int wofs;              // first tap of the class in wp
  // patch byte offset of every tap, (dy - dy0) * PW + (dx - dx0) pixels; padded
  // with zeros to whole stages of G taps (their weights are staged as zeros)
  int toff[IG_MAXTAPS + 7];
  signed char tdy[IG_MAXTAPS + 3], tdx[IG_MAXTAPS + 3];
};
struct IgArgs {
  const __bf16* x;    // N x H x W x Cin (C1 channels of it when x2 != nullptr)
  // The input as TWO tensors (the skip connections, nets.py:104-106, 300-345:
  // tf.concat([upcnv, skip], axis=3) in front of a convolution): channels
  // [0, C1) come from x (N x H x W x C1), channels [C1, Cin) from x2
  // (N x H x W x (Cin - C1)) -- the concatenated tensor is never written.
  // C1 a multiple of 32 (a chunk of 32 input channels is one tensor's).
  const __bf16* x2;
  int C1;
  // ... and its data gradient as two tensors: output channels [0, O1) go to out
  // (pitch O1), [O1, Cout) to out2 (pitch Cout - O1); O1 a multiple of the
  // workgroup's block of output channels.
  __bf16* out2;
  int O1;
  const __bf16* wp;   // [taps of all classes][Cout][Cin]
  __bf16* out;        // N x OHF x OWF x Cout
  int N, H, W, Cin, Cout;
  int s;              // input pixels per output step
  int os;             // output pixels per (i, j) step
  int OHF, OWF;
  int G;              // taps per weight stage
  int PH, PW;         // staged patch: rows, pixels per row
  int ncls;
  // Batch-norm statistics of the output, accumulated in the epilogue (st_ws !=
  // nullptr; csrc/lsi_bn.hip's workspace): sums of y and y * y per channel and
  // sub-batch group of the bf16-ROUNDED outputs -- what lsi_bn_relu_fwd's first
  // pass would read the tensor back for --, fp32 device atomics into slot
  // (workgroup index mod st_ns) of the group's accumulators, fire and forget:
  // lsi_bn_relu_norm, the next kernel on the stream, folds and clears them.  (A
  // last-arriver protocol inside this kernel was built first: every workgroup
  // then waits for its adds and a counter's return before it leaves, ~4 us each
  // -- 91 -> 117 us for the 3072 workgroups of `upcnv1`, all that the
  // statistics pass had cost.)
  float* st_ws;
  int st_groups;   // sub-batch groups along N
  int st_ns;       // accumulator slots (lsi_bn_stat_slots)
  // Split over the input channels (ks > 1): workgroup (.., ksi) multiplies the
  // chunks [ksi nch / ks, (ksi + 1) nch / ks) of 32 input channels and leaves its
  // fp32 sums in part[ksi][n][y][x][co]; conv_splitk_fold_kernel adds the ks
  // slabs in a fixed order, rounds, stores (and takes the batch-norm sums).  For
  // the bottleneck maps (2 x 6 ... 16 x 48 pixels, 256 - 1024 channels), where
  // the tiles alone are 64 - 256 workgroups, each a chain of 16 - 32 staged
  // units that wait a load latency per 36 - 72 MFMAs.
  float* part;
  int ks;
  int swz;   // XCD-aware workgroup order (see the kernel's index decode)
  IgClass cls[4];
};

// RW: pixel rows per wave; NCT: tiles of 16 output channels (BN = 16 NCT); G:
// taps per weight stage -- a compile-time count, so that a stage is straight-
// line code: the tap offsets come in one batch of scalar loads and the
// scheduler overlaps a tap's fragment reads with the previous tap's MFMAs
template <int RW, int NCT, int G>
__global__ __launch_bounds__(256) void conv_igemm_kernel(IgArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ig_smem[];
  constexpr int TH = 4 * RW, BN = 16 * NCT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pxl = lane & 15, kg = lane >> 4;
  const int ncb = a.Cout / BN;
  // Workgroup -> (tile, image, class, channel block, split).  The workgroups that
  // read the same input patch -- the parity classes of a stride-2 data gradient /
  // transposed convolution, the blocks of output channels, the splits -- used to
  // sit gridDim.x * gridDim.y * N apart in dispatch order: never in flight
  // together, on whatever XCD, and the patch came from HBM once per class
  // (`upcnv1`: 4 x 50 MB read for 100 MB written).  a.swz: with block b on XCD
  // b % 8 (observed placement; a speed matter only), the (class, channel block,
  // split) siblings of a tile are consecutive blocks OF ONE XCD -- eight apart in
  // dispatch order: in flight together, sharing that XCD's L2.
  int bx = blockIdx.x, by = blockIdx.y, co0, ksi, ci_, n;
  if (a.swz) {
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const unsigned xcd = lin & 7u, r = lin >> 3;
    const unsigned nsib = (unsigned)(a.ks * a.ncls * ncb);
    const unsigned g = r % nsib, tile = (r / nsib) * 8u + xcd;   // tile over gx * gy * N
    bx = (int)(tile % gridDim.x);
    by = (int)((tile / gridDim.x) % gridDim.y);
    n = (int)(tile / (gridDim.x * gridDim.y));
    co0 = (int)(g % ncb) * BN;
    ci_ = (int)((g / ncb) % a.ncls);
    ksi = (int)(g / (ncb * a.ncls));
  } else {
    const int zz = blockIdx.z / ncb;
    co0 = (blockIdx.z - zz * ncb) * BN;
    ksi = zz / (a.ncls * a.N);
    const int zc = zz - ksi * (a.ncls * a.N);
    ci_ = zc / a.N; n = zc - ci_ * a.N;
  }
  const IgClass& k = a.cls[ci_];
  const int i0 = by * TH, j0 = bx * 16;
  if (i0 >= k.OHt || j0 >= k.OWt) return;  // (the grid covers the largest class)
  const int PW = a.PW, npix = a.PH * PW;
  unsigned char* const patch = ig_smem;
  unsigned char* const wts = ig_smem + (size_t)npix * IG_PIX;

  // The patch pieces this thread stages (16 bytes each: pixel, quarter of its
  // 32 channels): pixel index into the input, -1 outside it.  The same for
  // every chunk.
  constexpr int MAXP = 12;  // (<= 768 staged pixels)
  int goff[MAXP];
  const int npiece = npix * 4;
  {
    const int iy0 = i0 * a.s + k.dy0, ix0 = j0 * a.s + k.dx0;
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
      const int idx = tid + 256 * k;
      const int pix = idx >> 2;
      const int py = pix / PW, px = pix - py * PW;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool ok = idx < npiece && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      goff[k] = ok ? ((n * a.H + iy) * a.W + ix) : -1;   // (pixel index)
    }
  }
  f32x4 acc[RW][NCT];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // this lane's B fragments: pixel (row wave * RW + r, column pxl) of the tile
  const unsigned b_lane =
      (unsigned)((wave * RW * a.s) * PW + pxl * a.s) * IG_PIX + (unsigned)kg * 16u;
  const unsigned b_row = (unsigned)(a.s * PW) * IG_PIX;
  const int ntaps = k.ntaps;
  const __bf16* const wp = a.wp + (size_t)k.wofs * a.Cout * a.Cin;
  const unsigned a_lane = (unsigned)pxl * IG_PIX + (unsigned)kg * 16u;  // weight row pxl of a tile

  // Software pipeline over the units (chunk of 32 channels, group of G taps):
  // the loads of unit u + 1 -- its weights, and the chunk's patch when the unit
  // opens a chunk -- are issued into registers before unit u is multiplied and
  // written to LDS after it, so a stage's memory latency hides behind the
  // previous stage's MFMAs (one wave per SIMD and workgroup: nobody else would).
  constexpr int NWP = G * BN * 4, WB = (NWP + 255) / 256;
  const int ngrp = (ntaps + G - 1) / G;
  const int nch = a.Cin / 32;
  const int ch_lo = ksi * nch / a.ks, ch_hi = (ksi + 1) * nch / a.ks;   // (this split's chunks)
  const int nunit = (ch_hi - ch_lo) * ngrp;
  u32x4 pv[MAXP], wv[WB];
  auto fetch = [&](int u) {
    const int chl = u / ngrp, gi = u - chl * ngrp;
    const int c0 = (ch_lo + chl) * 32, t0 = gi * G;
    if (gi == 0) {
      // (the chunk's tensor: its channel count is the pixel pitch)
      const bool second = c0 >= a.C1;
      const __bf16* const xb = second ? a.x2 + (c0 - a.C1) : a.x + c0;
      const int pitch = second ? a.Cin - a.C1 : a.C1;
#pragma unroll
      for (int kk = 0; kk < MAXP; ++kk) {
        pv[kk] = zero4;
        if (tid + 256 * kk < npiece && goff[kk] >= 0)
          pv[kk] = *reinterpret_cast<const u32x4*>(xb + (size_t)goff[kk] * pitch +
                                                   8 * ((tid + 256 * kk) & 3));
      }
    }
    const __bf16* const wsrc = wp + ((size_t)t0 * a.Cout + co0) * a.Cin + c0;
    const int nreal = (ntaps - t0) * BN * 4;   // (taps past the class's last one: zeros)
#pragma unroll
    for (int kk = 0; kk < WB; ++kk) {
      const int idx = tid + 256 * kk;
      wv[kk] = zero4;
      if (idx < NWP && idx < nreal) {
        const int q = idx & 3, co = (idx >> 2) & (BN - 1), t = idx / (4 * BN);
        wv[kk] = *reinterpret_cast<const u32x4*>(wsrc + ((size_t)t * a.Cout + co) * a.Cin + 8 * q);
      }
    }
  };
  auto stash = [&](int u) {   // registers -> LDS
    const int gi = u % ngrp;
    if (gi == 0) {
#pragma unroll
      for (int kk = 0; kk < MAXP; ++kk) {
        const int idx = tid + 256 * kk;
        if (idx < npiece)
          *reinterpret_cast<u32x4*>(patch + (size_t)(idx >> 2) * IG_PIX + (idx & 3) * 16) = pv[kk];
      }
    }
#pragma unroll
    for (int kk = 0; kk < WB; ++kk) {
      const int idx = tid + 256 * kk;
      if (idx < NWP) {
        const int q = idx & 3, co = (idx >> 2) & (BN - 1), t = idx / (4 * BN);
        *reinterpret_cast<u32x4*>(wts + (size_t)(t * BN + co) * IG_PIX + q * 16) = wv[kk];
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
      const unsigned toff = (unsigned)k.toff[t0 + t];
      bf16x8 af[NCT];
#pragma unroll
      for (int c = 0; c < NCT; ++c)
        af[c] = *reinterpret_cast<const bf16x8*>(wts + (size_t)(t * BN + 16 * c) * IG_PIX + a_lane);
      const unsigned char* const bp = patch + b_lane + toff;
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(bp + r * b_row);
#pragma unroll
        for (int c = 0; c < NCT; ++c)
          acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], bf, acc[r][c], 0, 0, 0);
      }
    }
  }
  // ---- channels-last stores: lane = 4 output channels of one pixel -----------
  const int j = j0 + pxl;
  if (a.ks > 1) {
    // ---- a split's fp32 sums: part[ksi][n][y][x][co] ----------------------------
    if (j < k.OWt) {
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
    }
    return;
  }
  if (a.st_ws) {
    // ---- batch-norm statistics of this tile (see IgArgs) -----------------------
    __syncthreads();  // (the last unit's fragments have been read: red is the staging memory)
    const int per_grp = a.N / a.st_groups, grp = n / per_grp;
    // (the hand-over tag of the group, lsi_bn_ws.h, by the workgroup of its first tile)
    bn_stats_epilogue<RW, NCT>(
        acc, [&](int r) { return j < k.OWt && i0 + wave * RW + r < k.OHt; },
        reinterpret_cast<float*>(ig_smem), a.st_ws, grp, a.st_groups, a.st_ns, a.Cout, co0,
        bx == 0 && by == 0 && co0 == 0 && ci_ == 0 && n == grp * per_grp);
  }
  if (j < k.OWt) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int i = i0 + wave * RW + r;
      if (i < k.OHt) {
        const bool o_second = co0 >= a.O1;
        __bf16* const o = (o_second ? a.out2 + (co0 - a.O1) : a.out + co0) +
            (((size_t)n * a.OHF + (size_t)(i * a.os + k.ooy)) * a.OWF + (j * a.os + k.oox)) *
                (o_second ? a.Cout - a.O1 : a.O1) + 4 * kg;
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
          bf16x4 v;
          v[0] = (__bf16)acc[r][c][0]; v[1] = (__bf16)acc[r][c][1];
          v[2] = (__bf16)acc[r][c][2]; v[3] = (__bf16)acc[r][c][3];
          *reinterpret_cast<bf16x4*>(o + 16 * c) = v;
        }
      }
    }
  }
}

// The sums of a split convolution (IgArgs::part): out = bf16(slab 0 + slab 1 +
// ...), the order fixed; the batch-norm sums of the rounded values as the
// unsplit kernel's epilogue takes them.  Block = 64 quads of channels x 4
// pixels; grid.x = image x pixel block (a block's pixels belong to one image =
// one sub-batch group), grid.y = blocks of 256 channels.
struct FoldArgs {
  const float* part;
  __bf16* out;
  __bf16* out2;
  int O1, Cout, N, ks, pb;
  long npix;       // pixels per image
  float* st_ws;
  int st_groups, st_ns;
};
__global__ __launch_bounds__(256) void conv_splitk_fold_kernel(FoldArgs a) {
  __shared__ float red[4][2][256];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int co = 4 * ((int)blockIdx.y * 64 + tx);
  const int n = blockIdx.x / a.pb, pbk = blockIdx.x - n * a.pb;
  const long per = (a.npix + a.pb - 1) / a.pb;
  const long p0 = pbk * per, p1 = p0 + per < a.npix ? p0 + per : a.npix;
  const bool live = co < a.Cout;
  float ss[4] = {0.f, 0.f, 0.f, 0.f}, qq[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const size_t slab = (size_t)a.N * a.npix * a.Cout;
    const bool second = co >= a.O1;
    __bf16* const ob = second ? a.out2 + (co - a.O1) : a.out + co;
    const int pitch = second ? a.Cout - a.O1 : a.O1;
    for (long p = p0 + ty; p < p1; p += 4) {
      const size_t pix = (size_t)n * a.npix + p;
      const float* const src = a.part + pix * a.Cout + co;
      f32x4 v = *reinterpret_cast<const f32x4*>(src);
      for (int k = 1; k < a.ks; ++k) v += *reinterpret_cast<const f32x4*>(src + k * slab);
      bf16x4 o;
      o[0] = (__bf16)v[0]; o[1] = (__bf16)v[1]; o[2] = (__bf16)v[2]; o[3] = (__bf16)v[3];
      *reinterpret_cast<bf16x4*>(ob + pix * pitch) = o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float r = (float)o[e];
        ss[e] += r;
        qq[e] = __builtin_fmaf(r, r, qq[e]);
      }
    }
  }
  if (!a.st_ws) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[ty][0][4 * tx + e] = ss[e]; red[ty][1][4 * tx + e] = qq[e]; }
  __syncthreads();
  const int C = a.Cout;
  const int per_grp = a.N / a.st_groups, grp = n / per_grp;
  const int tid = ty * 64 + tx;
  if (tid == 0 && blockIdx.y == 0 && pbk == 0 && n == grp * per_grp)
    bn_stats_tag(a.st_ws, grp, C, a.st_groups);
  for (int t = tid; t < 512; t += 256) {
    const int q = t >> 8, ch = t & 255;
    const int cc = (int)blockIdx.y * 256 + ch;
    if (cc < C) {
      const float v = (red[0][q][ch] + red[1][q][ch]) + (red[2][q][ch] + red[3][q][ch]);
      const int f = (int)(blockIdx.y * gridDim.x + blockIdx.x);
      bn_stats_add(a.st_ws, grp, f, a.st_ns, C, q, cc, v);
    }
  }
}

// The weights in the kernel's operand order, rounded to bf16 (lsi_conv_device.h's
// pack; D0, D1 multiples of 32: no edge tiles).
__global__ __launch_bounds__(256) void conv_pack_kernel(LsiPackJob a) {
  __shared__ float tile[PACK_TC][32][33];
  pack_tile<__bf16, false>(a, blockIdx.x, blockIdx.y, tile);   // block (x, y) = tile (d1, d0) / 32
}
__global__ __launch_bounds__(256) void conv_pack_many_kernel(const LsiPackJob* jobs, int njobs) {
  __shared__ float tile[PACK_TC][32][33];
  __shared__ int which;
  pack_job_tile<__bf16, false>(jobs, njobs, tile, &which);
}

constexpr size_t IG_LDS_CAP = 80 * 1024;  // two workgroups per CU

// Tile shape for the tap lists: the tallest row block whose patch + one weight
// stage fit the LDS share; G = as many taps per stage as fit next to the patch.
bool ig_shape(IgArgs& k, int* rw_out, int* nct_out, size_t* lds_out) {
  const int nct = (k.Cout % 64 == 0) ? 4 : 2;
  const int bn = 16 * nct;
  const ConvSpans sp = conv_tap_spans(k);
  const int spany = sp.spany, spanx = sp.spanx, maxoh = sp.maxoh;
  k.PW = 15 * k.s + spanx;
  static const char* rw_env = getenv("LSI_IGEMM_MAXRW");   // experiments
  const int rw_max = rw_env ? atoi(rw_env) : 8;
  for (int rw = rw_max; rw >= 1; rw >>= 1) {
    if (rw > 1 && 4 * (rw / 2) >= maxoh) continue;  // (a shorter block covers the rows)
    // (rows 8 per wave: 12 fragment reads for 32 MFMAs instead of 8 for 16 -- the
    // LDS read rate is what bounds the wide layers -- where the tile count still
    // fills the chip twice)
    if (rw == 8 && (long)((maxoh + 31) / 32) * ((k.cls[0].OWt + 15) / 16) * k.N * k.ncls *
                           (k.Cout / bn) < 1024)
      continue;
    // (... and shorter tiles while the launch would leave CUs without a
    // workgroup: `icnv5` 512 -> 256 at 16 x 48 had 96 workgroups of 16 rows,
    // 58 us; 192 of 8 rows: 40 us)
    static const char* fill_env = getenv("LSI_IGEMM_MINWG");   // experiments
    const long min_wg = fill_env ? atol(fill_env) : 256;
    if (rw > 1 && (long)((maxoh + 4 * rw - 1) / (4 * rw)) * ((k.cls[0].OWt + 15) / 16) * k.N *
                          k.ncls * (k.Cout / bn) < min_wg)
      continue;
    const int th = 4 * rw;
    k.PH = (th - 1) * k.s + spany;
    const size_t patch = (size_t)k.PH * k.PW * IG_PIX;
    if (k.PH * k.PW > 768) continue;
    if (patch + (size_t)bn * IG_PIX > IG_LDS_CAP) continue;
    // taps per weight stage: one of the instantiated counts -- the one that
    // wastes the fewest padded taps, then the fewest stages -- that fits
    static const int GS[4] = {9, 7, 5, 4};
    int g = 0, best_pad = 1 << 30, best_st = 1 << 30;
    for (int gi = 0; gi < 4; ++gi) {
      const int gc = GS[gi];
      if (patch + (size_t)gc * bn * IG_PIX > IG_LDS_CAP) continue;
      int pad = 0, st = 0;
      for (int c = 0; c < k.ncls; ++c) {
        const int n = k.cls[c].ntaps, stages = (n + gc - 1) / gc;
        pad += stages * gc - n; st += stages;
      }
      if (pad < best_pad || (pad == best_pad && st < best_st)) {
        best_pad = pad; best_st = st; g = gc;
      }
    }
    if (!g) continue;
    k.G = g;
    conv_tap_offsets(k, IG_PIX, IG_MAXTAPS + 7);
    *rw_out = rw; *nct_out = nct;
    *lds_out = patch + (size_t)g * bn * IG_PIX;
    return true;
  }
  return false;
}

// The plan of a launch (LSI_IGEMM_SPLITK: the workgroup count the split over the
// input channels aims at, 0 = never).
int ig_plan(IgArgs& k, ConvPlan* p) {
  static const char* env = getenv("LSI_IGEMM_SPLITK");   // experiments
  return conv_plan(k, ig_shape, LSI_EINVAL, env ? atol(env) : 512, p);
}

int ig_launch(IgArgs& k, hipStream_t stream, void* workspace = nullptr,
              size_t workspace_bytes = 0) {
  ConvPlan pl;
  const int prc = ig_plan(k, &pl);
  if (prc != LSI_OK) return prc;
  if (pl.grid.x == 0) return LSI_OK;
  const int rw = pl.rw, nct = pl.nct;
  const size_t lds = pl.lds;
  dim3 grid = pl.grid;
  conv_adopt_split(k, pl, workspace, workspace_bytes, &grid);
  {
    // (bijective only when the tiles split evenly over the eight XCDs.  Taken for
    // the parity classes of large maps only -- `upcnv1` 88 -> 71 us forward,
    // profiles/r06/conv_bench_swz{0,1}.txt; where the WEIGHTS are the traffic -- the
    // bottleneck maps, their splits and channel blocks -- the workgroups that share
    // weights are neighbours in the plain order and the swizzle costs 3 - 8 us.)
    static const char* env = getenv("LSI_IGEMM_SWZ");   // experiments
    const long tiles = (long)grid.x * grid.y * k.N;
    k.swz = (env ? atoi(env) != 0 : true) && k.ks == 1 && k.ncls > 1 && tiles >= 512 &&
            tiles % 8 == 0;
  }
  const void* fn = nullptr;
#define IG_CASE(R, C, GG) \
  if (rw == R && nct == C && k.G == GG) fn = (const void*)conv_igemm_kernel<R, C, GG>
#define IG_CASES(GG) \
  IG_CASE(8, 4, GG); IG_CASE(8, 2, GG); \
  IG_CASE(4, 4, GG); IG_CASE(2, 4, GG); IG_CASE(1, 4, GG); \
  IG_CASE(4, 2, GG); IG_CASE(2, 2, GG); IG_CASE(1, 2, GG)
  IG_CASES(9); IG_CASES(7); IG_CASES(5); IG_CASES(4);
#undef IG_CASES
#undef IG_CASE
  if (!fn) return LSI_EINVAL;
  {
    static const char* dbg = getenv("LSI_IG_DEBUG");   // (experiments: the plan of every call)
    if (dbg)
      fprintf(stderr, "ig N%d %dx%d cin %d cout %d s%d os%d ncls %d taps %d: RW %d NCT %d G %d grid %u x %u x %u = %u WGs (ks %d), lds %zu\n",
              k.N, k.H, k.W, k.Cin, k.Cout, k.s, k.os, k.ncls, k.cls[0].ntaps, rw, nct, k.G, grid.x, grid.y,
              grid.z, grid.x * grid.y * grid.z, k.ks, lds);
  }
  if (lsi_ensure_dynamic_lds(fn, lds) != LSI_OK) return LSI_ELAUNCH;
  void* kargs[1] = {&k};
  if (hipLaunchKernel(fn, grid, dim3(256), kargs, lds, stream) != hipSuccess) return LSI_ELAUNCH;
  if (hipGetLastError() != hipSuccess) return LSI_ELAUNCH;
  if (k.ks > 1) {
    FoldArgs f;
    f.part = k.part; f.out = k.out; f.out2 = k.out2; f.O1 = k.O1; f.Cout = k.Cout;
    f.N = k.N; f.ks = k.ks;
    f.npix = (long)k.OHF * k.OWF;
    // (pixel blocks per image: ~2 workgroups per CU over the launch, >= 4 pixels each)
    const int cb = (k.Cout + 255) / 256;
    long pb = 512 / ((long)k.N * cb);
    if (pb > (f.npix + 3) / 4) pb = (f.npix + 3) / 4;
    f.pb = pb < 1 ? 1 : (int)pb;
    f.st_ws = k.st_ws; f.st_groups = k.st_groups; f.st_ns = k.st_ns;
    hipLaunchKernelGGL(conv_splitk_fold_kernel, dim3(k.N * f.pb, cb), dim3(64, 4), 0, stream, f);
    if (hipGetLastError() != hipSuccess) return LSI_ELAUNCH;
  }
  return LSI_OK;
}

bool desc_ok(const LsiConvDesc* d) { return conv_desc_common(d, 32); }

}  // namespace

extern "C" int lsi_conv2d_supported(const LsiConvDesc* d) { return desc_ok(d) ? 1 : 0; }

extern "C" size_t lsi_conv2d_packed_bytes(const LsiConvDesc* d) {
  if (!desc_ok(d)) return 0;
  return (size_t)d->KH * d->KW * d->Cin * d->Cout * sizeof(__bf16);
}

extern "C" int lsi_conv2d_pack_job(const LsiConvDesc* d, int32_t mode, const float* weight,
                                   void* packed, size_t packed_bytes, LsiPackJob* job,
                                   int32_t* nblocks) {
  return conv_pack_job<IgArgs>(d, mode, weight, packed, packed_bytes, job, nblocks, desc_ok(d),
                               lsi_conv2d_packed_bytes(d));
}

extern "C" int lsi_conv2d_pack(const LsiConvDesc* d, int32_t mode, const float* weight,
                               void* packed, size_t packed_bytes, lsi_stream_t stream_) {
  LsiPackJob p;
  int32_t nb;
  const int rc = lsi_conv2d_pack_job(d, mode, weight, packed, packed_bytes, &p, &nb);
  if (rc != LSI_OK) return rc;
  hipLaunchKernelGGL(conv_pack_kernel, dim3(d->Cin / 32, d->Cout / 32), dim3(256), 0,
                     (hipStream_t)stream_, p);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

extern "C" int lsi_conv2d_pack_many(const LsiPackJob* jobs_device, int32_t njobs,
                                    int32_t total_blocks, lsi_stream_t stream_) {
  if (!jobs_device) return LSI_ENULL;
  if (njobs <= 0 || total_blocks <= 0) return LSI_EINVAL;
  hipLaunchKernelGGL(conv_pack_many_kernel, dim3(total_blocks), dim3(256), 0,
                     (hipStream_t)stream_, jobs_device, njobs);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

struct IgStats {
  float* ws; int groups;
};

static int ig_run(const LsiConvDesc* d, int mode, const void* src, const void* packed,
                  void* dst, lsi_stream_t stream_, const IgStats* st = nullptr,
                  const void* src2 = nullptr, int c1 = 0, void* dst2 = nullptr,
                  void* workspace = nullptr, size_t workspace_bytes = 0) {
  if (!d || !src || !packed || !dst) return LSI_ENULL;
  if (!desc_ok(d)) return LSI_EUNSUPPORTED;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 7) || ((uintptr_t)packed & 15)) return LSI_EINVAL;
  IgArgs k;
  int8_t tap[56];
  conv_classes(d, mode, k, tap);
  k.x = (const __bf16*)src; k.wp = (const __bf16*)packed; k.out = (__bf16*)dst;
  k.C1 = k.Cin;
  k.O1 = k.Cout;
  k.ks = 1;
  if (dst2) {   // the data gradient as two tensors
    const int bn = (k.Cout % 64 == 0) ? 64 : 32;
    if (mode != 1 || ((uintptr_t)dst2 & 7)) return LSI_EINVAL;
    if (c1 <= 0 || c1 >= k.Cout || c1 % bn) return LSI_EINVAL;
    k.out2 = (__bf16*)dst2;
    k.O1 = c1;
  }
  if (src2) {   // the input as two tensors (forward only)
    if (mode != 0 || ((uintptr_t)src2 & 15)) return LSI_EINVAL;
    if (c1 <= 0 || c1 >= k.Cin || c1 % 32) return LSI_EINVAL;
    k.x2 = (const __bf16*)src2;
    k.C1 = c1;
  }
  if (st) {
    if (!st->ws) return LSI_ENULL;
    // (the accumulators of a group are 2 x 2048 floats; whole images per group)
    if (st->groups < 1 || k.N % st->groups || k.Cout > 2048) return LSI_EINVAL;
    k.st_ws = st->ws; k.st_groups = st->groups; k.st_ns = lsi_bn_stat_slots(k.Cout);
  }
  return ig_launch(k, (hipStream_t)stream_, workspace, workspace_bytes);
}

extern "C" size_t lsi_conv2d_workspace_bytes(const LsiConvDesc* d, int32_t mode) {
  if (!desc_ok(d) || mode < 0 || mode > 1) return 0;
  IgArgs k;
  int8_t tap[56];
  conv_classes(d, mode, k, tap);
  k.C1 = k.Cin; k.O1 = k.Cout; k.ks = 1;
  ConvPlan pl;
  if (ig_plan(k, &pl) != LSI_OK || pl.grid.x == 0) return 0;
  return conv_part_bytes(k, pl.ks);
}

extern "C" int lsi_conv2d_run(const LsiConvDesc* d, int32_t mode, const LsiConvIO* io,
                              lsi_stream_t stream) {
  if (!io) return LSI_ENULL;
  if (mode < 0 || mode > 1) return LSI_EINVAL;
  if (io->workspace_bytes && !io->workspace) return LSI_ENULL;
  const IgStats st = {io->bn_workspace, io->groups};
  if (mode == 0 && io->out2) return LSI_EINVAL;
  if (mode == 1 && io->x2) return LSI_EINVAL;
  return ig_run(d, mode, io->x, io->packed, io->out, stream, io->bn_workspace ? &st : nullptr,
                io->x2, io->c1, io->out2, io->workspace, io->workspace_bytes);
}

extern "C" int lsi_conv2d_fwd(const LsiConvDesc* d, const void* x, const void* packed,
                              void* out, lsi_stream_t stream) {
  return ig_run(d, 0, x, packed, out, stream);
}

extern "C" int lsi_conv2d_bwd_data(const LsiConvDesc* d, const void* gy, const void* packed,
                                   void* gx, lsi_stream_t stream) {
  return ig_run(d, 1, gy, packed, gx, stream);
}

extern "C" int lsi_conv2d_fwd_bnstats(const LsiConvDesc* d, const void* x, const void* packed,
                                      void* out, float* bn_workspace, int32_t groups,
                                      lsi_stream_t stream) {
  const IgStats st = {bn_workspace, groups};
  return ig_run(d, 0, x, packed, out, stream, &st);
}

extern "C" int lsi_conv2d_fwd_cat(const LsiConvDesc* d, const void* x1, const void* x2,
                                  int32_t c1, const void* packed, void* out,
                                  float* bn_workspace, int32_t groups, lsi_stream_t stream) {
  if (!x2) return LSI_ENULL;
  const IgStats st = {bn_workspace, groups};
  return ig_run(d, 0, x1, packed, out, stream, bn_workspace ? &st : nullptr, x2, c1);
}

extern "C" int lsi_conv2d_bwd_data_cat(const LsiConvDesc* d, const void* gy, const void* packed,
                                       void* gx1, void* gx2, int32_t c1, lsi_stream_t stream) {
  if (!gx2) return LSI_ENULL;
  return ig_run(d, 1, gy, packed, gx1, stream, nullptr, nullptr, c1, gx2);
}

extern "C" int lsi_conv2d_bwd_data_bnstats(const LsiConvDesc* d, const void* gy,
                                           const void* packed, void* gx, float* bn_workspace,
                                           int32_t groups, lsi_stream_t stream) {
  const IgStats st = {bn_workspace, groups};
  return ig_run(d, 1, gy, packed, gx, stream, &st);
}
