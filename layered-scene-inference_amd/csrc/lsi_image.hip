// Exact AREA resize of a ragged batch of uint8 images (gfx950): the arithmetic
// of lsi/data/kitti/data.py:area_resize applied to decode_png(path) * (1/255)
// (reference lsi/data/kitti/data.py:247-266, tf.image.resize_images(AREA)), for
// n images of their own H x W in ONE launch.
//
// Integers: in units of 1/Ho the overlap of output row i with input row y is
// oy = min((i+1) H, (y+1) Ho) - max(i H, y Ho), columns alike with W, Wo, and the
// normalised weight is oy ox / (H W) exactly.  sum oy ox u8 <= 255 H W < 2^32 is
// accumulated in uint32 -- no rounding, any order -- and finished by one
// conversion and one fp32 multiply by fl(1 / (255 H W)): within 1.5 ulp of the
// exact rational, bitwise reproducible, 0 where the covered input is 0.
//
// Bound: HBM streaming (every input byte once per tile that covers it, 4 output
// bytes per input byte at most); about 30 MB for 8 KITTI images, so the fixed
// costs count: one launch, 256 threads per tile of 8 output rows x 32 RGB pixels
// (12 bytes per thread, the lanes of a row contiguous) or x 128 one-channel
// pixels (one float4 per thread); a pixel's column weight is formed once for
// its channels.
// Loads: the input rows of a tile start at any byte address (W C = 183 is legal).
// They are staged through LDS in chunks of CHUNK_ROWS rows x at most
// CHUNK_BYTES bytes with aligned 16-byte loads: a row is read from its address
// rounded down to 16 and its phase (0..15) is kept in LDS, so the taps read
// lds[row][phase + byte].  The buffer is 16-byte aligned and a multiple of 16
// bytes long, so an aligned 16-byte load that holds one valid byte lies inside
// it.  The tap loops run over whatever the ratio gives (1-2 taps when
// upscaling, 7 x 7 for a factor 5); tiles whose input exceeds one chunk loop
// over chunks with the sums kept in registers.
//
// lsi_augment_resize_u8 is the same kernel template with a per-image crop
// window, flip bit, tone table and channel gains:
//   window  H, W of everything above become the window's ch, cw (the overlaps,
//           the uint32 bound 255 ch cw < 2^32, scale = fl(1 / (255 ch cw)));
//           input row y, column x of the window is byte ((y0 + y) W + x0 + x) C
//           of the image, rows stay W C bytes apart.  The load argument above
//           still holds: a 16-byte load is issued only when it holds a byte of
//           a window row, the window lies inside the image (validated) and the
//           image inside the 16-byte aligned buffer.
//   table   uint8[C][256], 16-byte aligned in the same packed buffer, copied to
//           LDS once per workgroup and applied to the staged bytes as they are
//           written to LDS -- once per staged byte, not once per tap; the tap
//           loops are the plain kernel's.  Outputs are <= 255: the bound holds.
//   gains   min(fl(fl((float)acc * scale) * gain[c]), 1): two roundings, no
//           contraction (there is no add), then the clamp.
//   flip    the tile is computed in unflipped coordinates and stored mirrored:
//           pixel k goes to column Wo - 1 - k; the float4 of one-channel pixels
//           kb .. kb + 3 goes, reversed, to columns Wo - 4 - kb .. (a multiple
//           of 4 when Wo and kb are).
// The plain instances compile to the code they were before the template.
//
// lsi_augment_sample_u16 (a kernel of its own, below the template) samples
// 16-bit disparity maps by nearest neighbour through the same descriptors and
// packed buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/lsi_hip.h"

namespace {

constexpr int TILE_ROWS = 8;     // output rows per workgroup
constexpr int TILE_COLS = 32;    // threads along a row
constexpr int THREADS = TILE_ROWS * TILE_COLS;
constexpr int CHUNK_ROWS = 16;
constexpr int PITCH = 256;                 // LDS bytes per staged row
constexpr int CHUNK_BYTES = PITCH - 16;    // payload: the phase takes up to 15
constexpr int ROW_VECS = PITCH / 16;

// pixels per thread: one RGB pixel (a 12-byte store, lanes contiguous) or four
// one-channel pixels (a float4)
__host__ __device__ constexpr int pixels_per_thread(int C) { return C == 1 ? 4 : 1; }

struct ImageArgs {
  static constexpr bool AUG = false;
  int n, Ho, Wo;
  int vec_store;  // C = 1: Wo is a multiple of 4 and out is 16-byte aligned
  const LsiImageDesc* desc;
  const uint8_t* packed;
  float* out;
};

struct AugmentArgs {
  static constexpr bool AUG = true;
  int n, Ho, Wo;
  int vec_store;
  const LsiAugmentDesc* desc;
  const uint8_t* packed;
  const uint8_t* tables;  // packed + tables_offset: uint8[n_tables][C][256]
  float* out;
};

__device__ __forceinline__ int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Args = ImageArgs: H, W are the image's.  Args = AugmentArgs: H, W are the
// crop window's and (wy0, wx0, pitch_px) place it in the image.
template <int C, typename Args>
__global__ __launch_bounds__(THREADS) void area_resize_u8_kernel(Args a) {
  constexpr bool AUG = Args::AUG;
  constexpr int P = pixels_per_thread(C);
  constexpr int TILE_PX = TILE_COLS * P;
  constexpr int CHUNK_COLS = CHUNK_BYTES / C;
  __shared__ __attribute__((aligned(16))) uint8_t lds[CHUNK_ROWS * PITCH];
  __shared__ __attribute__((aligned(16))) uint8_t tab[AUG ? C * 256 : 16];
  const auto d = a.desc[blockIdx.z];
  int H, W, wy0 = 0, wx0 = 0, pitch_px;
  bool tone = false;
  if constexpr (AUG) {
    H = d.ch; W = d.cw; wy0 = d.y0; wx0 = d.x0; pitch_px = d.W;
    tone = d.table >= 0;
    if (tone) {  // read after the chunk loop's first barrier
      const uint4* t =
          reinterpret_cast<const uint4*>(a.tables + (size_t)d.table * (C * 256));
      for (int s = threadIdx.x; s < C * 16; s += THREADS)
        reinterpret_cast<uint4*>(tab)[s] = t[s];
    }
  } else {
    H = d.H; W = d.W; pitch_px = W;
  }
  const int Ho = a.Ho, Wo = a.Wo;
  const uint8_t* src = a.packed + d.offset;  // 16-byte aligned (validated)
  // byte offset in the image of window row y, window column x
  auto byte_of = [&](int y, int x) { return ((wy0 + y) * pitch_px + wx0 + x) * C; };

  // the tile: output rows [i0, i1), output pixels [k0, k1) of each row
  const int i0 = blockIdx.y * TILE_ROWS, i1 = min(i0 + TILE_ROWS, Ho);
  const int k0 = blockIdx.x * TILE_PX, k1 = min(k0 + TILE_PX, Wo);
  // ... and the input rows / columns it covers (products < 2^31: validated)
  const int ty0 = (i0 * H) / Ho, ty1 = ceil_div(i1 * H, Ho);
  const int tx0 = (k0 * W) / Wo, tx1 = ceil_div(k1 * W, Wo);

  // this thread: output row i, pixels [kb, kb + P)
  const int i = i0 + (int)threadIdx.x / TILE_COLS;
  const int kb = k0 + P * ((int)threadIdx.x % TILE_COLS);
  const bool row_ok = i < i1;
  int xs[P], xe[P];
  uint32_t acc[P * C];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const bool ok = row_ok && kb + p < k1;
    xs[p] = ok ? ((kb + p) * W) / Wo : 0;
    xe[p] = ok ? ceil_div((kb + p + 1) * W, Wo) : 0;  // empty range: no taps
#pragma unroll
    for (int c = 0; c < C; ++c) acc[p * C + c] = 0u;
  }
  const int ys = row_ok ? (i * H) / Ho : 0;
  const int ye = row_ok ? ceil_div((i + 1) * H, Ho) : 0;

  for (int cy = ty0; cy < ty1; cy += CHUNK_ROWS) {
    const int rows = min(CHUNK_ROWS, ty1 - cy);
    for (int cx = tx0; cx < tx1; cx += CHUNK_COLS) {
      const int ncols = min(CHUNK_COLS, tx1 - cx);
      const int nbytes = ncols * C;
      __syncthreads();  // the previous chunk has been read
      for (int s = threadIdx.x; s < rows * ROW_VECS; s += THREADS) {
        const int r = s / ROW_VECS, q = s - r * ROW_VECS;
        const int first = byte_of(cy + r, cx);
        const int phase = first & 15;
        if (q * 16 < phase + nbytes) {
          uint4 v =
              *reinterpret_cast<const uint4*>(src + (first - phase) + q * 16);
          if constexpr (AUG) {
            if (tone) {
              // LDS byte q 16 + b is byte q 16 + b - phase of the row, whose
              // first byte is channel 0 (bytes ahead of it are never read):
              // byte b of this vector is channel (c0 + b) % 3 with c0 below
              // (q 16 - phase + 15 >= 0 and 15 % 3 == 0) -- three table rows,
              // picked by constants
              const int c0 = C == 1 ? 0 : (q * 16 - phase + 15) % 3;
              const uint8_t* const rows[3] = {
                  tab + c0 * 256, tab + (C == 1 ? 0 : (c0 + 1) % 3) * 256,
                  tab + (C == 1 ? 0 : (c0 + 2) % 3) * 256};
              uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                uint32_t o = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                  o |= (uint32_t)rows[(4 * j + b) % 3][(w4[j] >> (8 * b)) & 255u]
                       << (8 * b);
                w4[j] = o;
              }
              v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
            }
          }
          *reinterpret_cast<uint4*>(lds + r * PITCH + q * 16) = v;
        }
      }
      __syncthreads();
      const int y_lo = max(ys, cy), y_hi = min(ye, cy + rows);
      for (int y = y_lo; y < y_hi; ++y) {
        const uint32_t oy = (uint32_t)(min((i + 1) * H, (y + 1) * Ho) - max(i * H, y * Ho));
        const uint8_t* row = lds + (y - cy) * PITCH + (byte_of(y, cx) & 15);
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const int k = kb + p;
          const int x_lo = max(xs[p], cx), x_hi = min(xe[p], cx + ncols);
          uint32_t sx[C];
#pragma unroll
          for (int c = 0; c < C; ++c) sx[c] = 0u;
          for (int x = x_lo; x < x_hi; ++x) {
            const uint32_t ox =
                (uint32_t)(min((k + 1) * W, (x + 1) * Wo) - max(k * W, x * Wo));
#pragma unroll
            for (int c = 0; c < C; ++c) sx[c] += ox * row[(x - cx) * C + c];
          }
#pragma unroll
          for (int c = 0; c < C; ++c) acc[p * C + c] += oy * sx[c];
        }
      }
    }
  }

  if (!row_ok || kb >= k1) return;
  const float scale = (float)(1.0 / (255.0 * (double)H * (double)W));
  if constexpr (AUG) {
    const bool flip = (d.flags & LSI_AUG_FLIP) != 0;
    float val[P * C];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int c = 0; c < C; ++c)
        val[p * C + c] = fminf(((float)acc[p * C + c] * scale) * d.gain[c], 1.0f);
    float* orow = a.out + ((size_t)blockIdx.z * Ho + i) * Wo * C;
    if constexpr (C == 3) {
      float* o = orow + (flip ? Wo - 1 - kb : kb) * 3;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = val[c];
    } else if (a.vec_store) {  // kb + 4 <= k1; Wo - 4 - kb is a multiple of 4
      if (flip)
        *reinterpret_cast<float4*>(orow + (Wo - 4 - kb)) =
            make_float4(val[3], val[2], val[1], val[0]);
      else
        *reinterpret_cast<float4*>(orow + kb) = make_float4(val[0], val[1], val[2], val[3]);
    } else {
#pragma unroll
      for (int p = 0; p < P; ++p)
        if (kb + p < k1) orow[flip ? Wo - 1 - kb - p : kb + p] = val[p];
    }
    return;
  }
  float* o = a.out + (((size_t)blockIdx.z * Ho + i) * Wo + kb) * C;
  if constexpr (C == 3) {  // 12 bytes per lane, the lanes of a row contiguous
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (float)acc[c] * scale;
  } else {
    if (a.vec_store) {  // kb + 4 <= k1: both are multiples of 4
      float4 v;
      v.x = (float)acc[0] * scale;
      v.y = (float)acc[1] * scale;
      v.z = (float)acc[2] * scale;
      v.w = (float)acc[3] * scale;
      *reinterpret_cast<float4*>(o) = v;
    } else {
#pragma unroll
      for (int p = 0; p < P; ++p)
        if (kb + p < k1) o[p] = (float)acc[p] * scale;
    }
  }
}

// the checks the two entry points share; H, W: what the overlaps run over
bool bad_call(int32_t n, int32_t Ho, int32_t Wo, int32_t Co, const uint8_t* packed,
              size_t packed_bytes, const float* out, const void* desc_dev) {
  if (n <= 0 || n > 65535 || Ho <= 0 || Wo <= 0 || (Co != 1 && Co != 3)) return true;
  if (((uintptr_t)packed & 15) || (packed_bytes & 15) || ((uintptr_t)out & 3) ||
      ((uintptr_t)desc_dev & 7))
    return true;
  return (int64_t)Wo * Co > INT32_MAX - 4 * THREADS;
}

template <typename Args>
int launch(const Args& a, int32_t n, int32_t Ho, int32_t Wo, int32_t Co,
           lsi_stream_t stream) {
  const int tile_px = TILE_COLS * pixels_per_thread(Co);
  const dim3 grid((Wo + tile_px - 1) / tile_px, (Ho + TILE_ROWS - 1) / TILE_ROWS, n);
  if (grid.y > 65535u) return LSI_EINVAL;
  if (Co == 1)
    hipLaunchKernelGGL((area_resize_u8_kernel<1, Args>), grid, dim3(THREADS), 0,
                       (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((area_resize_u8_kernel<3, Args>), grid, dim3(THREADS), 0,
                       (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

// lsi_augment_sample_u16: nearest-neighbour samples of 16-bit
// disparity maps through the same descriptors.  Output pixel (i, k) of map m
// reads window row min(((2 i + 1) ch) / (2 Ho), ch - 1), column alike -- the
// pixel under the output pixel's centre -- and stores
//   (float)(((double)raw * (1 / 256)) * ((double)Wo / (double)cw))
// (the first product is exact; one fp64 division, one fp64 product, one
// rounding to fp32: augment.sample_disparity_px's bits) at column k, or
// Wo - 1 - k under LSI_AUG_FLIP.
// Bound: 4 output bytes written per 2-byte gather, nothing shared between
// threads, so there is no LDS: a thread gathers four adjacent columns of one
// row and stores them as one float4 (reversed, at Wo - 4 - kb, when mirrored);
// the lanes of a wave write 1 KiB of one output row.
constexpr int SAMPLE_COLS = 64;   // threads along a row, four columns each
constexpr int SAMPLE_ROWS = 4;    // output rows per workgroup

struct SampleArgs {
  int Ho, Wo;
  int vec_store;  // Wo is a multiple of 4 and out is 16-byte aligned
  const LsiAugmentDesc* desc;
  const uint8_t* packed;
  float* out;
};

__global__ __launch_bounds__(SAMPLE_COLS * SAMPLE_ROWS) void augment_sample_u16_kernel(
    SampleArgs a) {
  const int i = blockIdx.y * SAMPLE_ROWS + (int)threadIdx.x / SAMPLE_COLS;
  const int kb = 4 * (blockIdx.x * SAMPLE_COLS + (int)threadIdx.x % SAMPLE_COLS);
  const int Ho = a.Ho, Wo = a.Wo;
  if (i >= Ho || kb >= Wo) return;
  const LsiAugmentDesc d = a.desc[blockIdx.z];
  const bool flip = (d.flags & LSI_AUG_FLIP) != 0;
  // (2 i + 1) ch <= (2 Ho + 1)(ch + 1) < 2^31 (validated), columns alike
  const int y = d.y0 + min(((2 * i + 1) * d.ch) / (2 * Ho), d.ch - 1);
  const uint16_t* row = reinterpret_cast<const uint16_t*>(a.packed + d.offset) +
                        (int64_t)y * d.W + d.x0;
  const double scale = (double)Wo / (double)d.cw;
  float v[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // (past the row's end the last column is read again and not stored)
    const int k = min(kb + p, Wo - 1);
    const int x = min(((2 * k + 1) * d.cw) / (2 * Wo), d.cw - 1);
    v[p] = (float)(((double)row[x] * (1.0 / 256.0)) * scale);
  }
  float* o = a.out + ((int64_t)blockIdx.z * Ho + i) * Wo;
  if (a.vec_store) {  // kb + 4 <= Wo: both are multiples of 4
    if (flip)
      *reinterpret_cast<float4*>(o + (Wo - 4 - kb)) = make_float4(v[3], v[2], v[1], v[0]);
    else
      *reinterpret_cast<float4*>(o + kb) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (kb + p < Wo) o[flip ? Wo - 1 - (kb + p) : kb + p] = v[p];
  }
}

}  // namespace

extern "C" {

int lsi_augment_sample_u16(int32_t n, const LsiAugmentDesc* desc_host,
                           const LsiAugmentDesc* desc_dev, const uint8_t* packed,
                           size_t packed_bytes, int32_t Ho, int32_t Wo, float* out,
                           lsi_stream_t stream) {
  if (!desc_host || !desc_dev || !packed || !out) return LSI_ENULL;
  if (bad_call(n, Ho, Wo, 1, packed, packed_bytes, out, desc_dev)) return LSI_EINVAL;
  for (int32_t m = 0; m < n; ++m) {
    const LsiAugmentDesc& d = desc_host[m];
    if (d.H <= 0 || d.W <= 0 || d.C != 1) return LSI_EINVAL;
    if (d.y0 < 0 || d.x0 < 0 || d.ch < 1 || d.cw < 1 ||
        (int64_t)d.y0 + d.ch > d.H || (int64_t)d.x0 + d.cw > d.W)
      return LSI_EINVAL;
    // the kernel's int32 products (2 i + 1) ch, (2 k + 1) cw
    if ((int64_t)(2 * (int64_t)Ho + 1) * ((int64_t)d.ch + 1) > INT32_MAX ||
        (int64_t)(2 * (int64_t)Wo + 1) * ((int64_t)d.cw + 1) > INT32_MAX)
      return LSI_EINVAL;
    if (d.flags & ~(uint32_t)LSI_AUG_FLIP) return LSI_EINVAL;
    if (d.table != -1) return LSI_EINVAL;
    const uint64_t bytes = 2 * (uint64_t)d.H * (uint64_t)d.W;   // < 2^63
    if (d.offset < 0 || (d.offset & 15) || (uint64_t)d.offset > packed_bytes ||
        bytes > packed_bytes - (uint64_t)d.offset)
      return LSI_EINVAL;
  }
  SampleArgs a;
  a.Ho = Ho; a.Wo = Wo;
  a.vec_store = (Wo % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  a.desc = desc_dev; a.packed = packed; a.out = out;
  const int quads = (Wo + 3) / 4;
  const dim3 grid((quads + SAMPLE_COLS - 1) / SAMPLE_COLS,
                  (Ho + SAMPLE_ROWS - 1) / SAMPLE_ROWS, n);
  if (grid.y > 65535u) return LSI_EINVAL;
  hipLaunchKernelGGL(augment_sample_u16_kernel, grid, dim3(SAMPLE_COLS * SAMPLE_ROWS), 0,
                     (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? LSI_OK : LSI_ELAUNCH;
}

int lsi_area_resize_u8(int32_t n, const LsiImageDesc* desc_host,
                       const LsiImageDesc* desc_dev, const uint8_t* packed,
                       size_t packed_bytes, int32_t Ho, int32_t Wo, int32_t Co,
                       float* out, lsi_stream_t stream) {
  if (!desc_host || !desc_dev || !packed || !out) return LSI_ENULL;
  if (bad_call(n, Ho, Wo, Co, packed, packed_bytes, out, desc_dev)) return LSI_EINVAL;
  for (int32_t m = 0; m < n; ++m) {
    const LsiImageDesc& d = desc_host[m];
    if (d.H <= 0 || d.W <= 0 || d.C != Co) return LSI_EINVAL;
    // the uint32 accumulator: 255 H W < 2^32
    if ((int64_t)d.H * d.W > LSI_IMAGE_MAX_PIXELS) return LSI_EINVAL;
    // the kernel's int32 products (i + 1) H, (y + 1) Ho, (k + 1) W, (x + 1) Wo
    if ((int64_t)(Ho + 1) * (d.H + 1) > INT32_MAX ||
        (int64_t)(Wo + 1) * (d.W + 1) > INT32_MAX)
      return LSI_EINVAL;
    const int64_t bytes = (int64_t)d.H * d.W * d.C;
    if (d.offset < 0 || (d.offset & 15) || (uint64_t)d.offset > packed_bytes ||
        (uint64_t)bytes > packed_bytes - (uint64_t)d.offset)
      return LSI_EINVAL;
  }
  ImageArgs a;
  a.n = n; a.Ho = Ho; a.Wo = Wo;
  a.vec_store = (Wo % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  a.desc = desc_dev; a.packed = packed; a.out = out;
  return launch(a, n, Ho, Wo, Co, stream);
}

int lsi_augment_resize_u8(int32_t n, const LsiAugmentDesc* desc_host,
                          const LsiAugmentDesc* desc_dev, const uint8_t* packed,
                          size_t packed_bytes, int64_t tables_offset,
                          int32_t n_tables, int32_t Ho, int32_t Wo, int32_t Co,
                          float* out, lsi_stream_t stream) {
  if (!desc_host || !desc_dev || !packed || !out) return LSI_ENULL;
  if (bad_call(n, Ho, Wo, Co, packed, packed_bytes, out, desc_dev)) return LSI_EINVAL;
  if (n_tables < 0 || n_tables > 65535) return LSI_EINVAL;
  if (n_tables > 0 &&
      (tables_offset < 0 || (tables_offset & 15) ||
       (uint64_t)tables_offset > packed_bytes ||
       (uint64_t)n_tables * Co * 256 > packed_bytes - (uint64_t)tables_offset))
    return LSI_EINVAL;
  for (int32_t m = 0; m < n; ++m) {
    const LsiAugmentDesc& d = desc_host[m];
    if (d.H <= 0 || d.W <= 0 || d.C != Co) return LSI_EINVAL;
    // (also keeps the byte offsets ((y0 + y) W + x0 + x) C below 2^31)
    if ((int64_t)d.H * d.W > LSI_IMAGE_MAX_PIXELS) return LSI_EINVAL;
    // the window: inside the image, not empty; 255 ch cw <= 255 H W < 2^32
    if (d.y0 < 0 || d.x0 < 0 || d.ch < 1 || d.cw < 1 ||
        (int64_t)d.y0 + d.ch > d.H || (int64_t)d.x0 + d.cw > d.W)
      return LSI_EINVAL;
    // the kernel's int32 products (i + 1) ch, (y + 1) Ho, (k + 1) cw, (x + 1) Wo
    if ((int64_t)(Ho + 1) * (d.ch + 1) > INT32_MAX ||
        (int64_t)(Wo + 1) * (d.cw + 1) > INT32_MAX)
      return LSI_EINVAL;
    if (d.flags & ~(uint32_t)LSI_AUG_FLIP) return LSI_EINVAL;
    if (d.table < -1 || d.table >= n_tables) return LSI_EINVAL;
    for (int c = 0; c < Co; ++c)
      if (!std::isfinite(d.gain[c]) || d.gain[c] < 0.0f) return LSI_EINVAL;
    const int64_t bytes = (int64_t)d.H * d.W * d.C;
    if (d.offset < 0 || (d.offset & 15) || (uint64_t)d.offset > packed_bytes ||
        (uint64_t)bytes > packed_bytes - (uint64_t)d.offset)
      return LSI_EINVAL;
  }
  AugmentArgs a;
  a.n = n; a.Ho = Ho; a.Wo = Wo;
  a.vec_store = (Wo % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  a.desc = desc_dev; a.packed = packed; a.out = out;
  a.tables = packed + (n_tables > 0 ? tables_offset : 0);
  return launch(a, n, Ho, Wo, Co, stream);
}

}  // extern "C"
