// Contact sheet of an evaluation iteration's visuals (gfx950): up to 256 fp32
// tensors of their own size, strides and value range are quantised to bytes
// and laid out on a regular grid of cells in ONE launch, so that one
// device-to-host copy carries everything a saved iteration shows
// (the list of cells is the reference's ldi_pred_eval.py
// define_visuals).
//
// The kernel is one pass over OUTPUT pixels: every byte of the sheet inside
// 3 x width is written exactly once, background included, and no byte beyond
// it.  The cell of a pixel follows from its coordinates by division (grid
// period = cell + gutter), the item from the cell, the source texel from the
// offset in the cell divided by the zoom.
//
// Bound: launch latency and the gathers (a sheet is a few MB).  A workgroup is
// 4 waves, wave w on output row 4 by + w and 256 consecutive pixels of it, a
// lane on 4 pixels = 12 bytes = three dword stores (rows are 4-byte aligned by
// the out_row_bytes rule; only the last run of a row may be partial and is
// stored by bytes).  The cell row is the wave's; where its 256 pixels lie in one
// cell column as well -- cells are wider than that at evaluation sizes -- the
// item index is made a scalar and the descriptor arrives in scalar loads;
// waves that straddle a column read it per pixel.  The 768-byte table is staged
// in LDS once per workgroup.
//
// Arithmetic (the whole contract; fp32, no FMA contraction, -ffp-contract=off):
//   v NaN -> the marker colour;  t = (v - lo) * inv;  t = min(max(t, 0), 1);
//   q = (int)floorf(t * 255 + 0.5).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsi_hip.h"

namespace {

constexpr int RUN = 4;            // pixels per lane
constexpr int LANES = 64;
constexpr int ROWS = 4;           // waves (output rows) per workgroup
constexpr int THREADS = LANES * ROWS;
constexpr int TILE_PX = LANES * RUN;

struct VisArgs {
  LsiVisSheet s;
  int Hs, Ws, tiles_x;
  const LsiVisItem* items;
  const uint8_t* lut;
  uint8_t* out;
  int64_t out_row_bytes;
};

__device__ __forceinline__ uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) {
  return r | (g << 8) | (b << 16);
}

// the byte of a value, or -1 for NaN
__device__ __forceinline__ int quantise(float v, float lo, float inv) {
  if (v != v) return -1;
  float t = (v - lo) * inv;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  return (int)floorf(t * 255.0f + 0.5f);
}

// the colour of pixel (iy, ix) of the cell that shows `it`, as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t shade(const LsiVisItem& it, int iy, int ix,
                                          uint32_t bg, uint32_t nan,
                                          const uint8_t* lut) {
  if (it.kind == LSI_VIS_SKIP) return bg;
  const int sy = iy / it.zoom, sx = ix / it.zoom;
  if (sy >= it.H || sx >= it.W) return bg;
  const float* a = it.src + ((int64_t)sy * it.s_y + (int64_t)sx * it.s_x);
  if (it.kind == LSI_VIS_RGB) {
    const int r = quantise(a[0], it.lo, it.inv);
    const int g = quantise(a[it.s_c], it.lo, it.inv);
    const int b = quantise(a[2 * it.s_c], it.lo, it.inv);
    return (r | g | b) < 0 ? nan : rgb(r, g, b);
  }
  float v = a[0];
  if (it.kind == LSI_VIS_ABSDIFF) {
    const float* b = it.ref + ((int64_t)sy * it.r_y + (int64_t)sx * it.r_x);
    v = fabsf(v - b[0]);
    if (it.C == 3) {
      v = v + fabsf(a[it.s_c] - b[it.r_c]);
      v = v + fabsf(a[2 * it.s_c] - b[2 * it.r_c]);
      v = v * (1.0f / 3.0f);
    }
  }
  const int q = quantise(v, it.lo, it.inv);
  if (q < 0) return nan;
  if (it.kind == LSI_VIS_GRAY) return rgb(q, q, q);
  return rgb(lut[3 * q], lut[3 * q + 1], lut[3 * q + 2]);
}

__global__ __launch_bounds__(THREADS) void visual_pack_kernel(VisArgs a) {
  __shared__ __attribute__((aligned(4))) uint8_t lut[768];
  if (a.lut != nullptr) {  // (uniform: a kernel argument)
    if (threadIdx.x < 192)
      reinterpret_cast<uint32_t*>(lut)[threadIdx.x] =
          reinterpret_cast<const uint32_t*>(a.lut)[threadIdx.x];
    __syncthreads();
  }
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / LANES);
  const int lane = (int)threadIdx.x % LANES;
  const int y = tile_y * ROWS + wave;
  const int x0 = tile_x * TILE_PX + lane * RUN;
  if (y >= a.Hs || x0 >= a.Ws) return;

  const int cols = a.s.cols, g = a.s.gutter;
  const uint32_t bg = rgb(a.s.bg[0], a.s.bg[1], a.s.bg[2]);
  const uint32_t nan = rgb(a.s.nan[0], a.s.nan[1], a.s.nan[2]);
  // the wave's cell row: r, and the row inside the cell (negative: the gutter)
  const int ph = a.s.cell_h + g, pw = a.s.cell_w + g;
  const int r = y / ph, iy = y - r * ph - g;
  const bool row_ok = r < a.s.rows && iy >= 0;
  // the cell column of this lane's pixels; the right border counts to no column
  int c = x0 / pw, ix = x0 - c * pw - g;
  const int c_last = (x0 + RUN - 1) / pw;
  const int c_wave = __builtin_amdgcn_readfirstlane(c);
  const bool one_column = __all(c == c_wave && c_last == c_wave);

  uint32_t px[RUN];
  if (one_column) {  // the item index is a scalar, and so is the descriptor
    const int k = r * cols + c_wave;
    const bool cell_ok = row_ok && c_wave < cols && k < a.s.n_items;
#pragma unroll
    for (int p = 0; p < RUN; ++p)
      px[p] = cell_ok && ix + p >= 0 ? shade(a.items[k], iy, ix + p, bg, nan, lut) : bg;
  } else {
#pragma unroll
    for (int p = 0; p < RUN; ++p) {
      const int k = r * cols + c;
      px[p] = row_ok && c < cols && ix >= 0 && k < a.s.n_items
                  ? shade(a.items[k], iy, ix, bg, nan, lut)
                  : bg;
      if (++ix == a.s.cell_w) {
        ix = -g;
        ++c;
      }
    }
  }

  uint8_t* o = a.out + (int64_t)y * a.out_row_bytes + (int64_t)x0 * 3;
  if (x0 + RUN <= a.Ws) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);  // 12 x0 bytes into an aligned row
    o4[0] = px[0] | (px[1] << 24);
    o4[1] = (px[1] >> 8) | (px[2] << 16);
    o4[2] = (px[2] >> 16) | (px[3] << 8);
  } else {  // the row's tail: 1 to 3 pixels
    for (int p = 0; p < a.Ws - x0; ++p) {
      o[3 * p] = (uint8_t)px[p];
      o[3 * p + 1] = (uint8_t)(px[p] >> 8);
      o[3 * p + 2] = (uint8_t)(px[p] >> 16);
    }
  }
}

}  // namespace

extern "C" {

int lsi_visual_sheet_size(const LsiVisSheet* s, int64_t* height, int64_t* width) {
  if (!s || !height || !width) return LSI_ENULL;
  if (s->rows <= 0 || s->cols <= 0 || s->cell_h <= 0 || s->cell_w <= 0 || s->gutter < 0)
    return LSI_EINVAL;
  *height = (int64_t)s->rows * s->cell_h + ((int64_t)s->rows + 1) * s->gutter;
  *width = (int64_t)s->cols * s->cell_w + ((int64_t)s->cols + 1) * s->gutter;
  return LSI_OK;
}

int lsi_visual_pack_u8(const LsiVisSheet* sheet, const LsiVisItem* items_host,
                       const LsiVisItem* items_dev, const uint8_t* lut_dev,
                       uint8_t* out, int64_t out_row_bytes, lsi_stream_t stream) {
  if (!sheet || !out) return LSI_ENULL;
  int64_t Hs, Ws;
  const int rc = lsi_visual_sheet_size(sheet, &Hs, &Ws);
  if (rc != LSI_OK) return rc;
  const int n = sheet->n_items;
  if (n < 0 || n > LSI_VIS_MAX_ITEMS || n > (int64_t)sheet->rows * sheet->cols)
    return LSI_EINVAL;
  if (n > 0 && (!items_host || !items_dev)) return LSI_ENULL;
  if (((uintptr_t)out & 3) || (out_row_bytes & 3) || out_row_bytes < 3 * Ws ||
      Hs > INT32_MAX / out_row_bytes)
    return LSI_EINVAL;
  if (((uintptr_t)items_dev & 7) || ((uintptr_t)lut_dev & 3)) return LSI_EINVAL;
  for (int k = 0; k < n; ++k) {
    const LsiVisItem& it = items_host[k];
    if (it.kind == LSI_VIS_SKIP) continue;
    if (it.kind != LSI_VIS_RGB && it.kind != LSI_VIS_GRAY && it.kind != LSI_VIS_LUT &&
        it.kind != LSI_VIS_ABSDIFF)
      return LSI_EINVAL;
    const bool c_ok = it.kind == LSI_VIS_RGB ? it.C == 3
                      : it.kind == LSI_VIS_ABSDIFF ? (it.C == 1 || it.C == 3)
                                                   : it.C == 1;
    if (!c_ok || it.zoom < 1 || it.H <= 0 || it.W <= 0) return LSI_EINVAL;
    if ((int64_t)it.H * it.zoom > sheet->cell_h || (int64_t)it.W * it.zoom > sheet->cell_w)
      return LSI_EINVAL;
    if (it.s_y < 0 || it.s_x < 0 || it.s_c < 0) return LSI_EINVAL;
    if (!isfinite(it.lo) || !isfinite(it.inv) || !(it.inv > 0.0f)) return LSI_EINVAL;
    if (!it.src) return LSI_ENULL;
    if (it.kind == LSI_VIS_ABSDIFF) {
      if (it.r_y < 0 || it.r_x < 0 || it.r_c < 0) return LSI_EINVAL;
      if (!it.ref) return LSI_ENULL;
    }
    if ((it.kind == LSI_VIS_LUT || it.kind == LSI_VIS_ABSDIFF) && !lut_dev)
      return LSI_ENULL;
  }
  VisArgs a;
  a.s = *sheet;
  a.Hs = (int)Hs;
  a.Ws = (int)Ws;
  a.tiles_x = (a.Ws + TILE_PX - 1) / TILE_PX;
  a.items = items_dev;
  a.lut = lut_dev;
  a.out = out;
  a.out_row_bytes = out_row_bytes;
  const int64_t blocks = (int64_t)a.tiles_x * ((a.Hs + ROWS - 1) / ROWS);
  if (blocks * THREADS > (int64_t)UINT32_MAX) return LSI_EINVAL;
  hipLaunchKernelGGL(visual_pack_kernel, dim3((unsigned)blocks), dim3(THREADS), 0,
                     (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

}  // extern "C"
