/*
 * lsi_hip.h -- C ABI of liblsi_hip.so, the MI355X (gfx950) implementation of
 * the layered-depth-image renderer hot path of google/layered-scene-inference.
 *
 * The reference has no FFI/plugin interface of its own: the boundary it offers
 * is the Python function surface of lsi.geometry.* / lsi.nnutils.helpers
 * (SURVEY.md section 8b).  Each entry point below names the reference
 * function(s) (paths relative to /root/reference) whose arithmetic it replaces;
 * the Python package in layered-scene-inference_amd/lsi/ binds them with ctypes
 * (binding shown in INTEGRATION.md).
 *
 * This file is the binding's only source: lsi/_C.py parses it at import and
 * derives every LSI_* constant, struct layout and argument list from it, and
 * refuses a declaration it cannot map.  Keep to the style below --
 *   #define LSI_NAME <integer>[u]
 *   typedef struct Name { <fixed-width scalars, T x[N], pointers> } Name;
 *   one prototype per entry point, parameters of these kinds:
 *     const Struct* d     ONE record, read on the host: the binding types it
 *                         (ctypes.POINTER(Struct)) and refuses another class
 *     const Struct d[]    an ARRAY of records, given by its address (a NumPy
 *                         array's, a device copy's): c_void_p
 *     any other T* p      a data pointer, given by its address: c_void_p
 *     lsi_stream_t        c_void_p
 * -- and tests/test_abi.py holds the derived layouts to the compiler's.
 *
 * Conventions
 *   - plain C: POD structs, raw device pointers, sizes; no C++/torch types.
 *   - every function returns LSI_OK (0) or a negative LSI_E* code, never throws,
 *     never allocates device memory, never synchronises the host.
 *   - all pointers are DEVICE pointers valid on the device the stream belongs
 *     to; work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 *     the legacy default stream) and the call returns immediately.
 *   - tensors are fp32.  Inputs carry explicit ELEMENT strides so that both the
 *     reference's channels-last L x B x H x W x C layout and planar (permuted
 *     NCHW) conv outputs are consumed without a copy.  Outputs are contiguous
 *     in the reference's logical shape.
 *   - pixel centres are at +0.5 (helpers.py:107-110); coordinates are (x, y).
 *   - the library keeps no state between calls.
 */
#ifndef LSI_HIP_H_
#define LSI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSI_VERSION 100 /* 0.1.0 */

/* error codes */
#define LSI_OK 0
#define LSI_EINVAL -1        /* bad shape / stride / flag combination        */
#define LSI_ENULL -2         /* required pointer is NULL                      */
#define LSI_EWORKSPACE -3    /* workspace too small                           */
#define LSI_ELAUNCH -4       /* kernel launch failed (hipGetLastError != 0)   */
#define LSI_EUNSUPPORTED -5  /* valid request this build does not implement   */

/* LsiSplatDesc.flags */
#define LSI_COMPOSE 1u       /* compose_layers=True  (ldi.py:167-171)         */
#define LSI_WANT_DISP 2u     /* compute_trg_disp=True (ldi.py:179-180)        */
#define LSI_HAS_MASK 4u      /* mask pointer is given (else mask == 1)        */
#define LSI_WS_KEEP 8u       /* workspace state is kept between calls (below) */
#define LSI_DETERMINISTIC 16u /* bitwise run-to-run reproducible results: the  */
                             /* STREAM path then adds its partial sums in a   */
                             /* fixed order (slower); TILE is always          */
                             /* reproducible, ATOMIC / ROWBAND never are      */

#define LSI_PACKED_RGBD 32u  /* the caller asserts: tex and disp are views of   */
                             /* ONE buffer of RGBD pixels -- disp == tex + 3   */
                             /* floats, tex_sc == 1, tex_sx == disp_sx == 4,   */
                             /* equal layer / batch / row strides, 16-byte     */
                             /* aligned (what a channels-last conv head with   */
                             /* 4 outputs writes).  One 16-byte load then      */
                             /* fetches a pixel's colour and disparity.  The   */
                             /* entry points verify it (LSI_EINVAL if not).    */
#define LSI_GRAD_M 64u       /* backward only: the gradient w.r.t. the B x 4 x 4 */
                             /* matrices M as well (lsi_splat_bwd_m,           */
                             /* lsi_splat_bwd_both_m; the entries without _m   */
                             /* refuse it with LSI_EINVAL)                     */

/* LsiSplatDesc.path: which kernel family renders the splat.                  */
#define LSI_PATH_AUTO 0      /* library decides from the descriptor          */
#define LSI_PATH_ATOMIC 1    /* source-parallel, global fp32 atomics; any M   */
#define LSI_PATH_ROWBAND 2   /* target-row-band tiles accumulated in LDS with */
                             /* fp32 LDS atomics; requires M[b][1][3] ==      */
                             /* M[b][2][3] == 0 for every b (target row       */
                             /* independent of disparity) -- lsi_rowband_ok.  */
#define LSI_PATH_STREAM 3    /* row-uniform projections (additionally         */
                             /* M[b][1][0] == M[b][2][0] == 0: rectified      */
                             /* stereo): wave-private LDS row windows updated */
                             /* by plain read-modify-write, merged into an    */
                             /* LDS tile of the band -- lsi_stream_ok.        */

#define LSI_PATH_TILE 4      /* any M: source pixels binned per target tile   */
                             /* with integer LDS exchanges, every target cell */
                             /* summed by its owner thread; no fp32 atomics.  */
                             /* What AUTO resolves to inside lsi_splat_fwd.   */

typedef void* lsi_stream_t; /* hipStream_t */

/*
 * Descriptor of one forward_splat call (ldi.py:71-182).
 *   tex  [l,b,y,x,c]  c in 0..2     element strides tex_s{l,b,y,x,c}
 *   disp [l,b,y,x]                  element strides disp_s{l,b,y,x}
 *   mask [l,b,y,x]   (optional)     element strides mask_s{l,b,y,x}
 * Ht = H * trg_downsampling and Wt = W * trg_downsampling must be integral
 * (the reference only works then: ldi.py:113-125).
 */
/*
 * Caller-owned state of the compact STREAM kernel's adaptive build choice (see
 * lsi_stream_adapt_state below).  Zero-initialise, point ctr_dev at 16 bytes of
 * device memory and ctr_host at 16 bytes of zeroed PINNED host memory, keep both
 * alive as long as the record is used, and do not let two calls that use the
 * same record overlap (one record per device, stream and call geometry).
 */
typedef struct LsiStreamAdapt {
  int32_t state;      /* 0 undecided, 1 twelve waves x 2 sets, 2 sixteen x 1  */
  int32_t pending;    /* a probe's counts are on their way to ctr_host        */
  uint32_t seq;       /* that probe's number                                  */
  uint32_t calls;
  uint32_t* ctr_dev;            /* {folded items, all items, seq}: device     */
  volatile uint32_t* ctr_host;  /* the same three words, pinned host memory   */
} LsiStreamAdapt;

typedef struct LsiSplatDesc {
  int32_t L, B, H, W, Ht, Wt;
  int64_t tex_sl, tex_sb, tex_sy, tex_sx, tex_sc;
  int64_t disp_sl, disp_sb, disp_sy, disp_sx;
  int64_t mask_sl, mask_sb, mask_sy, mask_sx;
  float trg_downsampling; /* s                                              */
  float max_disp;
  float zbuf_scale;       /* |zbuf_scale| <= 160 (else LSI_EINVAL)           */
  float bg_wt;            /* lsi_bg_weight(bg_layer_disp, max_disp, scale)   */
  uint32_t flags;
  int32_t path;
  /* Tuning knobs, 0 = library default: target rows per workgroup, threads   */
  /* per workgroup, and (STREAM) LDS window cells per wave = lsi_stream_ok(). */
  /* reserved: 0.  (tools/ set timing-experiment bits in it; results may then */
  /* be wrong -- see the `dbg` uses in csrc/lsi_splat_stream.hip.)            */
  int32_t tune_rows, tune_threads, tune_window, reserved;
  /* NULL, or the caller's record for the adaptive build choice of the compact */
  /* STREAM kernel (composed output): the library itself keeps no such state.  */
  LsiStreamAdapt* adapt;
} LsiSplatDesc;

/* Library version (LSI_VERSION of the build). */
int lsi_version(void);

/* Human-readable text for an LSI_E* code. */
const char* lsi_strerror(int code);

/*
 * Background weight of the white canvas, ldi.py:115-116:
 *   zbuffer_weights(bg_layer_disp / max_disp, zbuf_scale)   (helpers.py:180-193)
 * with the python-float division done in double, as the reference does.
 * Host function (no GPU work).
 */
float lsi_bg_weight(double bg_layer_disp, double max_disp, double zbuf_scale);

/*
 * Host-side test on a HOST copy of the B projection matrices (row-major 4x4):
 * returns 1 when LSI_PATH_ROWBAND renders this call exactly (target row of a
 * source pixel does not depend on its disparity and the normaliser is positive
 * over the whole source image), else 0.
 */
int lsi_rowband_ok(const LsiSplatDesc* desc, const float* M_host);

/*
 * Host-side test for LSI_PATH_STREAM on a HOST copy of the matrices: returns 0
 * when the path does not apply (projection not row-uniform, unsupported
 * strides/alignment), else the number of LDS window cells per wave the call
 * needs, plus flag bits (put the value in desc->tune_window unchanged).
 * LSI_WANT_DISP is rendered for composed output of unit-normaliser pairs
 * (channels-last or RGBD-pixel textures, no mask, at most 15 layers: the
 * composed view, then a second launch with one tile per layer for the
 * disparity, ldi.py:147-180); LSI_PACKED_RGBD inputs under the same
 * conditions; other requests return 0 (LSI_PATH_TILE renders them).
 */
int lsi_stream_ok(const LsiSplatDesc* desc, const float* M_host);

/*
 * Bytes of device workspace lsi_splat_fwd needs for this descriptor (16-byte
 * aligned; any path).  The ATOMIC path keeps its canvases there, the TILE path a
 * per-view disparity range.  The STREAM
 * path uses it to combine the target rows shared by two neighbouring row bands:
 * a few arrival counters at its start, then partial rows.  The counters must be
 * zero when a call starts and every call leaves them zero; lsi_splat_fwd clears
 * them itself (one small memset on the stream) unless LSI_WS_KEEP promises that
 * the buffer was zero-filled once and has only been used by completed or
 * stream-ordered STREAM-path lsi_splat_fwd calls WITH THE SAME L, B, Ht, Wt AND
 * flags since (the place of the counters depends on those; the other paths
 * write over them).  One workspace must not be used by
 * two calls that can run concurrently.  desc->path AUTO or ATOMIC: the size
 * that serves any path (the ATOMIC canvases dominate); STREAM or TILE: what
 * that path needs (counters, boundary rows, disparity ranges: kilobytes).
 */
size_t lsi_splat_workspace_bytes(const LsiSplatDesc* desc);

/*
 * forward_splat, ldi.py:71-182, with its callees fused into the launch:
 *   projection of every source pixel      helpers.py:116-137 (transform_pts)
 *   divide_safe                           helpers.py:82-85
 *   soft z-buffer weight                  helpers.py:180-193
 *   4-corner bilinear splat x3            sampling.py:171-254
 *   normalise / compose epilogue          ldi.py:157-182
 * M is the B x 4 x 4 src->trg matrix (projection.py:71-86), passed as data.
 * Outputs (contiguous; nl = 1 if LSI_COMPOSE else L):
 *   out_img  [nl,B,Ht,Wt,3]   out_wts [nl,B,Ht,Wt,1] (un-normalised weight sum)
 *   out_disp [nl,B,Ht,Wt,1]   required iff LSI_WANT_DISP
 * mask may be NULL (then LSI_HAS_MASK must be clear).
 */
int lsi_splat_fwd(const LsiSplatDesc* desc, const float* tex, const float* disp,
                  const float* mask, const float* M, float* out_img,
                  float* out_wts, float* out_disp, void* workspace,
                  size_t workspace_bytes, lsi_stream_t stream);

/*
 * Gradient of lsi_splat_fwd w.r.t. tex, disp and mask given the gradients of
 * out_img (g_img, [nl,B,Ht,Wt,3]) and optionally out_wts (g_wts, may be NULL).
 * The reference has no hand-written backward (TF autodiff, train_utils.py:113);
 * this implements the closed form of SURVEY.md section 3.5, reproducing TF's
 * zero-gradient conventions (floor, comparisons, clamps on the closed interval).
 * out_img / out_wts are the forward outputs.  g_tex [L,B,H,W,3], g_disp_in
 * [L,B,H,W], g_mask [L,B,H,W] (NULL unless LSI_HAS_MASK) are contiguous.
 * Gradients through out_disp are not implemented (it feeds no loss:
 * ldi_enc_dec.py:302-357) -- LSI_WANT_DISP is ignored here.
 * workspace: lsi_splat_bwd_workspace_bytes(desc) bytes of device scratch (one
 * float4 per output pixel: the gradient w.r.t. the un-normalised canvases).
 * When desc carries the forward's STREAM verdict for rectified pairs (path
 * LSI_PATH_STREAM + tune_window as lsi_stream_ok returned it), channels-last
 * textures (or RGBD pixels) with W % 4 == 0 (a mask, if any, with unit pixel
 * stride), the streamed kernel
 * (csrc/lsi_splat_bwd_stream.hip) derives that canvas in LDS and leaves the
 * workspace untouched; other descriptors take a pre-pass + one thread per
 * source pixel.  With LSI_GRAD_M in desc->flags the workspace also holds one
 * 16-float partial of the matrix gradient per workgroup (lsi_splat_bwd_m).
 * The entries without _m refuse LSI_GRAD_M (LSI_EINVAL) and otherwise are
 * lsi_splat_bwd_m / lsi_splat_bwd_both_m with g_M = NULL.
 */
size_t lsi_splat_bwd_workspace_bytes(const LsiSplatDesc* desc);

int lsi_splat_bwd(const LsiSplatDesc* desc, const float* tex, const float* disp,
                  const float* mask, const float* M, const float* out_img,
                  const float* out_wts, const float* g_img, const float* g_wts,
                  float* g_tex, float* g_disp_in, float* g_mask,
                  void* workspace, size_t workspace_bytes, lsi_stream_t stream);

/*
 * lsi_splat_bwd plus the gradient w.r.t. M, the B x 4 x 4 src->trg matrices
 * (projection.py:71-86 -> ldi.py:134-140: q = M p for p = (x+.5, y+.5, 1, d),
 * u = q0/n' * s, v = q1/n' * s, dd = q3/n', n' = divide_safe(q2)), what TF
 * autodiff of the reference gives k_s, k_t, rot and t through
 * tf.matrix_inverse / tf.matmul:
 *   g_M[b][j][k] = sum over l, y, x of dL/dq_j * p_k   (dL/dq_2 = dL/dn')
 * with the same zero-gradient conventions as the rest of the backward (floor,
 * clip, the 1e-3 corner clamp, dropped non-finite pixels: 0).  Requested by
 * LSI_GRAD_M in desc->flags: then g_M (B x 4 x 4 fp32, contiguous,
 * overwritten) must not be NULL (LSI_ENULL); without the flag it must be NULL
 * (LSI_EINVAL) and the call is lsi_splat_bwd's, launch for launch.  Each
 * workgroup of the backward kernel sums its pixels' shares in registers and
 * across its waves, and writes one 16-float partial to the workspace; one more
 * kernel adds the partials of each batch element in a fixed order (no float
 * atomics: g_M is bitwise reproducible whatever LSI_DETERMINISTIC says).  The
 * other outputs are bitwise those of the call without the flag.
 */
int lsi_splat_bwd_m(const LsiSplatDesc* desc, const float* tex,
                    const float* disp, const float* mask, const float* M,
                    const float* out_img, const float* out_wts,
                    const float* g_img, const float* g_wts, float* g_tex,
                    float* g_disp_in, float* g_mask, float* g_M, void* workspace,
                    size_t workspace_bytes, lsi_stream_t stream);

/*
 * lsi_splat_bwd_m plus the gradient through out_disp, the target disparity
 * (ldi.py:147-171: the third splat of D * pw, divide_safe, reduce_max), as TF
 * autodiff gives it.  desc is the forward's descriptor and must carry
 * LSI_WANT_DISP (else LSI_EINVAL); out_disp [nl,B,Ht,Wt,1] is the forward's
 * output and g_disp_out its incoming gradient (same layout, contiguous; both
 * required, LSI_ENULL).  Everything else is as lsi_splat_bwd_m: g_M B x 4 x 4
 * required iff LSI_GRAD_M (it then includes the disparity's share), the other
 * pointers and layouts as lsi_splat_bwd.  Per target cell and layer l, with
 * S_l = sum c_k pw D (no background) and W_l = bg + sum c_k pw:
 *   disp_l = S_l / W'_l,  W'_l = W_l + 1e-8 [W_l == 0]   (divide_safe: bg = 0
 *            and no pixel landing gives W' = 1e-8; its indicator has no gradient)
 *   composed: out = max_l disp_l, g_l = g [disp_l == out] / n with n the
 *            number of layers at the maximum (TF's reduce_max gradient: an even
 *            split among ties -- every cell no layer reaches is an L-way tie at
 *            0; a tie here is disp_l >= out - |out| 2^-19, see below); per
 *            layer: g_l = g
 *   gS_l = g_l / W'_l,  gW_l = g_l * (-disp_l / W'_l)
 * and a source pixel's corner k gains gW_l + D gS_l on dL/d(c_k pw) and
 * pw c_k gS_l on dL/dD; the zero-gradient conventions of lsi_splat_bwd hold
 * (a landed pixel whose pw is 0, e.g. mask 0, still gives its mask c_k D zw gS).
 * Composed calls do not have the per-layer W_l and disp_l: this call renders
 * them again from tex / disp / mask / M (one per-layer LSI_PATH_TILE forward
 * into the workspace), so the tie set is taken from the same per-layer values
 * as the canvas gradients; per-layer calls read them from out_wts / out_disp.
 * That render adds each cell's terms in no fixed order, so layers equal in
 * exact arithmetic may differ in their last bits (hence the 2^-19 tie
 * window), and a composed call's gradients are reproducible to rounding, not
 * bitwise; per-layer calls are bitwise reproducible for the same outputs.
 * A pre-pass writes the per-layer (gS, gW) canvases; the backward kernel of
 * lsi_splat_bwd_m (streamed or gather, chosen as there for the descriptor
 * without LSI_WANT_DISP) reads them at each pixel's corners.
 * workspace: lsi_splat_bwd_disp_workspace_bytes(desc) bytes of device scratch.
 */
size_t lsi_splat_bwd_disp_workspace_bytes(const LsiSplatDesc* desc);

int lsi_splat_bwd_disp(const LsiSplatDesc* desc, const float* tex,
                       const float* disp, const float* mask, const float* M,
                       const float* out_img, const float* out_wts,
                       const float* out_disp, const float* g_img,
                       const float* g_wts, const float* g_disp_out,
                       float* g_tex, float* g_disp_in, float* g_mask,
                       float* g_M, void* workspace, size_t workspace_bytes,
                       lsi_stream_t stream);

/*
 * forward_splat's two variants of one source view in ONE sweep: the reference's
 * training step renders every LDI twice, once per layer (compose_layers=False)
 * and once composed (compose_layers=True), ldi_enc_dec.py:302-334, repeating
 * identical per-layer splats (ldi.py:129-155).  desc->flags must not contain
 * LSI_COMPOSE or LSI_WANT_DISP.  Outputs: out_img / out_wts [L,B,Ht,Wt,3|1]
 * (per layer) and out_img_c / out_wts_c [1,B,Ht,Wt,3|1] (composed).  The STREAM
 * path sums the layers' tiles in LDS; the other paths render per layer and
 * derive the composed view from those outputs.  Workspace as lsi_splat_fwd.
 */
int lsi_splat_fwd_both(const LsiSplatDesc* desc, const float* tex,
                       const float* disp, const float* mask, const float* M,
                       float* out_img, float* out_wts, float* out_img_c,
                       float* out_wts_c, void* workspace,
                       size_t workspace_bytes, lsi_stream_t stream);

/*
 * Gradient of lsi_splat_fwd_both: the per-layer canvases receive the gradients
 * of both outputs (g_img / g_wts for the per-layer ones, g_img_c / g_wts_c for
 * the composed one; either pair may be NULL).  One gather pass over the source
 * pixels.  Workspace: lsi_splat_bwd_workspace_bytes(desc).
 */
int lsi_splat_bwd_both(const LsiSplatDesc* desc, const float* tex,
                       const float* disp, const float* mask, const float* M,
                       const float* out_img, const float* out_wts,
                       const float* out_img_c, const float* out_wts_c,
                       const float* g_img, const float* g_wts,
                       const float* g_img_c, const float* g_wts_c, float* g_tex,
                       float* g_disp_in, float* g_mask, void* workspace,
                       size_t workspace_bytes, lsi_stream_t stream);

/*
 * lsi_splat_bwd_both plus the gradient w.r.t. M (both outputs' share), as
 * lsi_splat_bwd_m: LSI_GRAD_M in desc->flags, g_M B x 4 x 4, overwritten.
 */
int lsi_splat_bwd_both_m(const LsiSplatDesc* desc, const float* tex,
                         const float* disp, const float* mask, const float* M,
                         const float* out_img, const float* out_wts,
                         const float* out_img_c, const float* out_wts_c,
                         const float* g_img, const float* g_wts,
                         const float* g_img_c, const float* g_wts_c,
                         float* g_tex, float* g_disp_in, float* g_mask,
                         float* g_M, void* workspace, size_t workspace_bytes,
                         lsi_stream_t stream);

/*
 * Parity/debug view of the projection stage: for every source pixel the four
 * flat target indices (tl,tr,bl,br; x + y*Wt within the batch element,
 * sampling.py:234-241) and the four updates of the weight splat,
 * zbuffer_weight * mask * corner_weight (ldi.py:145-153, sampling.py:213-232).
 *   idx4 [L,B,H*W,4] int32      upd4 [L,B,H*W,4] fp32
 */
int lsi_project_indices(const LsiSplatDesc* desc, const float* disp,
                        const float* mask, const float* M, int32_t* idx4,
                        float* upd4, lsi_stream_t stream);

/*
 * sampling.splat, sampling.py:171-254: 4-corner bilinear forward scatter-add
 * of a C-channel image at float coordinates onto an initial canvas.
 *   src [B,Hs,Ws,C], coords [B,Hs,Ws,2] (x,y), out [B,Ht,Wt,C]; all contiguous.
 * `out` must already hold init_trg_image; updates are added to it in place.
 * Sizes, for this and the bilinear entry points below (LSI_EINVAL otherwise,
 * before any pointer is looked at): B <= 65535; the canvas (here) or the
 * sampled image (there) has fewer than 2^24 pixels; the number of points,
 * Hs*Ws here and Ht*Wt there, is at most 2^31 - 256.  A point with a non-finite
 * coordinate adds and samples nothing and gets zero gradients.
 */
int lsi_splat_generic(int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ht,
                      int32_t Wt, const float* src, const float* coords,
                      float* out, lsi_stream_t stream);

/* Gradients of lsi_splat_generic w.r.t. src and coords (g_out [B,Ht,Wt,C]). */
int lsi_splat_generic_bwd(int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                          int32_t Ht, int32_t Wt, const float* src,
                          const float* coords, const float* g_out, float* g_src,
                          float* g_coords, lsi_stream_t stream);

/*
 * projection.forward_projection_matrix (inverse = 0; projection.py:71-86:
 * pad(K_t) [R t; 0 1] pad(K_s^-1)) or inverse_projection_matrix (inverse = 1;
 * :89-106) for B cameras, on the HOST (no device work): k_s, k_t, rot [B,3,3],
 * t [B,3,1], M [B,4,4], all host fp32.  The 3x3 inverse is evaluated in fp64
 * and rounded once; the 4x4 products accumulate sequentially over k with every
 * multiply and add rounded on its own -- the matrices lsi_splat_fwd's
 * bit-exactness contract is stated on (the Python mirror computes the same
 * values with torch ops).
 */
int lsi_projection_matrices(int32_t B, const float* k_s, const float* k_t,
                            const float* rot, const float* t, int32_t inverse,
                            float* M);

/*
 * sampling.batch_scatter_add_tensor, sampling.py:287-313 (and scatter_add_tensor
 * :257-284 with B = 1): out[b, idx[b,i]] += upd[b,i]; duplicates add.
 *   out [B,P] (holds init on entry), idx [B,N] int32 in [0,P), upd [B,N].
 * Out-of-range indices are skipped (TF raises; the Python mirror checks).
 */
int lsi_scatter_add(int32_t B, int64_t P, int64_t N, const int32_t* idx,
                    const float* upd, float* out, lsi_stream_t stream);

/*
 * sampling.bilinear (compose=True), sampling.py:41-132: 4-tap gather with zero
 * outside.  imgs [B,Hs,Ws,C], coords [B,Ht,Wt,2] (x,y), out [B,Ht,Wt,C].
 */
int lsi_bilinear_fwd(int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ht,
                     int32_t Wt, const float* imgs, const float* coords,
                     float* out, lsi_stream_t stream);

/*
 * sampling.bilinear (compose=False), sampling.py:124-130: the four taps, each
 * multiplied by its border-validity mask, and the four un-masked bilinear
 * weights, in the reference's order (x0,y0), (x0,y1), (x1,y0), (x1,y1).
 *   taps [4,B,Ht,Wt,C], wts [4,B,Ht,Wt,1].
 * lsi_bilinear_taps_bwd: TF autodiff of that form -- the taps' gradients are
 * scatter-added (through the masks) into g_imgs [B,Hs,Ws,C] (zero on entry; may
 * be NULL), the weights' gradients g_wts [4,B,Ht,Wt,1] (may be NULL: zero) give
 * g_coords [B,Ht,Wt,2] (may be NULL): d wts / d x = (-wy0, -wy1, +wy0, +wy1),
 * d wts / d y = (-wx0, +wx0, -wx1, +wx1); floor / clip / equal carry no gradient,
 * so the taps contribute nothing to g_coords.
 */
int lsi_bilinear_taps(int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ht,
                      int32_t Wt, const float* imgs, const float* coords,
                      float* taps, float* wts, lsi_stream_t stream);
int lsi_bilinear_taps_bwd(int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ht,
                          int32_t Wt, const float* coords, const float* g_taps,
                          const float* g_wts, float* g_imgs, float* g_coords,
                          lsi_stream_t stream);

/*
 * Gradients of lsi_bilinear_fwd.  g_imgs [B,Hs,Ws,C] must be zero on entry
 * (scatter-add target); g_coords [B,Ht,Wt,2] may be NULL.
 */
int lsi_bilinear_bwd(int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ht,
                     int32_t Wt, const float* imgs, const float* coords,
                     const float* g_out, float* g_imgs, float* g_coords,
                     lsi_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Losses on LDIs / rendered views and layer composition: one fused pass     */
/* each (csrc/lsi_loss.hip).  Scalars are DEVICE floats (no host sync);      */
/* gradients come out contiguous in the inputs' logical shape.               */
/* ------------------------------------------------------------------------ */

/* Inputs of zbuffer_composition_loss (lsi/loss/loss.py:66-115), element     */
/* strides: imgs [l,b,y,x,c] c in 0..2, masks/disps [l,b,y,x], trg [b,y,x,c] */
typedef struct LsiLossDesc {
  int32_t L, B, H, W;
  int64_t img_sl, img_sb, img_sy, img_sx, img_sc;
  int64_t mask_sl, mask_sb, mask_sy, mask_sx;
  int64_t disp_sl, disp_sb, disp_sy, disp_sx;
  int64_t trg_sb, trg_sy, trg_sx, trg_sc;
  float bg_layer_disp, max_disp, zbuf_scale;
  int32_t reserved;
} LsiLossDesc;

/* Bytes of device scratch every *_loss_fwd needs (partial sums). */
size_t lsi_loss_workspace_bytes(void);

/*
 * loss.zbuffer_composition_loss, lsi/loss/loss.py:66-115: white background
 * layer at bg_layer_disp appended; p_l = zbuffer_weights(d_l/max_disp)*m_l
 * normalised over the layers; 0.5 * mean(sum_l (img_l - trg)^2 * p_l).
 * masks may be NULL (ones).  out_loss: one device float.
 */
int lsi_zbuf_comp_loss_fwd(const LsiLossDesc* desc, const float* imgs,
                           const float* masks, const float* disps,
                           const float* trg, float* out_loss, void* workspace,
                           size_t workspace_bytes, lsi_stream_t stream);
/* Gradients w.r.t. imgs [L,B,H,W,3], masks [L,B,H,W] (NULL when masks is) and
 * disps [L,B,H,W], scaled by the device scalar g_loss. */
int lsi_zbuf_comp_loss_bwd(const LsiLossDesc* desc, const float* imgs,
                           const float* masks, const float* disps,
                           const float* trg, const float* g_loss, float* g_imgs,
                           float* g_masks, float* g_disps, lsi_stream_t stream);

/*
 * The two regularisers of the disparities in one read of disp [l,b,y,x]:
 *   out2[0] = ldi.disp_smoothness_loss  (lsi/geometry/ldi.py:33-68): mean |d_xx|
 *             + mean |d_xy| + mean |d_yx| + mean |d_yy| of forward differences
 *   out2[1] = loss.decreasing_disp_loss (lsi/loss/loss.py:48-63): mean relu(
 *             d_{l+1} - stop_gradient(d_l)); 0 when L == 1
 */
int lsi_disp_reg_loss_fwd(int32_t L, int32_t B, int32_t H, int32_t W,
                          int64_t sl, int64_t sb, int64_t sy, int64_t sx,
                          const float* disp, float* out2, void* workspace,
                          size_t workspace_bytes, lsi_stream_t stream);
/* g_disp [L,B,H,W] = g2[0] * d out2[0]/d disp + g2[1] * d out2[1]/d disp. */
int lsi_disp_reg_loss_bwd(int32_t L, int32_t B, int32_t H, int32_t W,
                          int64_t sl, int64_t sb, int64_t sy, int64_t sx,
                          const float* disp, const float* g2, float* g_disp,
                          lsi_stream_t stream);

/*
 * View-synthesis loss of the training script, ldi_enc_dec.py:337-357: AREA
 * resize of target [B,H,W,3] (element strides) to Ht x Wt (integer factors),
 * mean_c |t - r_l|, min over the nl layers of recons [nl,B,Ht,Wt,3]
 * (contiguous), crop x_min / y_min pixels on every side, mean.
 */
int lsi_view_synth_loss_fwd(int32_t nl, int32_t B, int32_t Ht, int32_t Wt,
                            int32_t H, int32_t W, int32_t x_min, int32_t y_min,
                            const float* recons, const float* target,
                            int64_t t_sb, int64_t t_sy, int64_t t_sx,
                            int64_t t_sc, float* out_loss, void* workspace,
                            size_t workspace_bytes, lsi_stream_t stream);
/* g_recons [nl,B,Ht,Wt,3]; reduce_min's gradient is split among tied layers. */
int lsi_view_synth_loss_bwd(int32_t nl, int32_t B, int32_t Ht, int32_t Wt,
                            int32_t H, int32_t W, int32_t x_min, int32_t y_min,
                            const float* recons, const float* target,
                            int64_t t_sb, int64_t t_sy, int64_t t_sx,
                            int64_t t_sc, const float* g_loss, float* g_recons,
                            lsi_stream_t stream);

/*
 * SSIM view-synthesis loss and metric (csrc/lsi_ssim.hip; no reference
 * counterpart, the definition is DESIGN.md section 4.13).  recons
 * [nl,B,Ht,Wt,3] contiguous, target [B,H,W,3] with the element strides t_s*,
 * H % Ht == 0 and W % Wt == 0; t = the AREA resize of target as in
 * lsi_view_synth_loss_fwd.  A window is a win x win patch (win odd, 3 .. 11)
 * wholly inside the crop [y_min, Ht - y_min) x [x_min, Wt - x_min); its weights
 * are g[i] g[j] with g from lsi_ssim_window.  Per window, layer and channel,
 * with the weighted means mu_x, mu_y, E_xx, E_yy, E_xy of x = recons, y = t:
 *   S = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2))
 *   d = (1 - (S_0 + S_1 + S_2) / 3) / 2
 * LSI_EINVAL for an even or out-of-range win, a crop that leaves no window or
 * non-integer factors, then LSI_ENULL, then LSI_EWORKSPACE (workspace:
 * lsi_loss_workspace_bytes()), all before any launch.  No atomics: the same
 * inputs give the same bits.
 */
typedef struct LsiSsimDesc {
  int32_t nl, B, Ht, Wt, H, W, x_min, y_min, win;
  float sigma, c1, c2;     /* sigma <= 0: the box window 1 / win              */
  int64_t t_sb, t_sy, t_sx, t_sc;
} LsiSsimDesc;

/* Host only: the win weights the kernels use, g[i] ~ exp(-(i - (win - 1) / 2)^2
 * / (2 sigma^2)) normalised to sum 1 in double and rounded to fp32. */
int lsi_ssim_window(int32_t win, float sigma, float* out);
/* out_loss (one device float) = mean over b and the windows of min_l d. */
int lsi_ssim_loss_fwd(const LsiSsimDesc* desc, const float* recons,
                      const float* target, float* out_loss, void* workspace,
                      size_t workspace_bytes, lsi_stream_t stream);
/* g_recons [nl,B,Ht,Wt,3], scaled by the device scalar g_loss: a window's share
 * goes to the layers whose d equals the minimum bit for bit, split evenly.
 * Every element is written; pixels outside the crop get 0. */
int lsi_ssim_loss_bwd(const LsiSsimDesc* desc, const float* recons,
                      const float* target, const float* g_loss, float* g_recons,
                      lsi_stream_t stream);
/* Adds the sum over b and the windows of layer 0's (S_0 + S_1 + S_2) / 3 to
 * acc2[0] and the number of windows to acc2[1] (device doubles, zeroed by the
 * caller once) in a one-block finishing kernel: no host synchronisation. */
int lsi_eval_ssim(const LsiSsimDesc* desc, const float* recons, const float* target,
                  double* acc2, void* workspace, size_t workspace_bytes,
                  lsi_stream_t stream);

/*
 * Edge-aware disparity smoothness loss (csrc/lsi_edge_smooth.hip; no reference
 * counterpart, the definition is DESIGN.md section 4.14).  disp [L,B,H,W,1]
 * with the element strides d_s*, guide 3 channels with the element strides
 * g_s* (g_sl = 0: one image [B,H,W,3] shared by all layers), o = order (1 or
 * 2), N = H W, p runs over the L B planes.  Stencils on the raw disparity d of a
 * plane, G its guide:
 *   order 1   sx[y,x] = d[y,x] - d[y,x+1],              x in [0, W-2]
 *             ex[y,x] = mean_c |G[y,x,c] - G[y,x+1,c]|
 *   order 2   sx[y,x] = d[y,x-1] - 2 d[y,x] + d[y,x+1], x in [1, W-2]
 *             ex[y,x] = 1/2 mean_c |G[y,x+1,c] - G[y,x-1,c]|
 * sy, ey the same along y.  wx = exp(-alpha ex), wy = exp(-alpha ey),
 *   A_p = sum |sx| wx,  B_p = sum |sy| wy,  S_p = sum d   (over plane p)
 *   k_p = 1 / (S_p / N + eps) if normalise, else 1
 *   loss = 1 / (L B) sum_p k_p [A_p / (H (W-o)) + B_p / ((H-o) W)]
 * i.e. mean(|sx| wx) + mean(|sy| wy), with normalise of d / (mean_plane(d) +
 * eps).  The guide is data: the gradient is w.r.t. disp only, sign(0) = 0:
 *   dloss/dd_i = k_p / (L B) [gx_i / (H (W-o)) + gy_i / ((H-o) W)]
 *                - [normalise] k_p^2 / (N L B) [A_p / (H (W-o)) + B_p / ((H-o) W)]
 * where gx_i, gy_i gather sign(s) w over the stencils that touch pixel i with
 * that stencil's coefficient (+1, -1 at order 1; +1, -2, +1 at order 2).
 * LSI_EINVAL for an order other than 1 or 2, H or W < order + 1, a negative or
 * non-finite alpha or non-positive dimensions, then LSI_ENULL, then
 * LSI_EWORKSPACE, all before any launch.  No atomics, no host synchronisation,
 * no allocation: the same inputs give the same bits, and both directions can be
 * captured in a HIP graph.
 */
typedef struct LsiEdgeSmoothDesc {
  int32_t L, B, H, W, order, normalise;
  int64_t d_sl, d_sb, d_sy, d_sx;
  int64_t g_sl, g_sb, g_sy, g_sx, g_sc;
  float alpha, eps;
} LsiEdgeSmoothDesc;

/* (3 L B bpp + L B) doubles with bpp = min(max(ceil(H W / 1024), 1), 256) blocks
 * per plane; 0 for a descriptor the entries below refuse. */
size_t lsi_edge_smooth_workspace_bytes(const LsiEdgeSmoothDesc* desc);
/* out_loss (one device float) = the loss; plane_sums (3 L B device doubles, the
 * caller's) = A_p, B_p, S_p at [3 p .. 3 p + 2], p = l B + b: written by the
 * finishing kernel, read by the backward.  The library keeps no state. */
int lsi_edge_smooth_loss_fwd(const LsiEdgeSmoothDesc* desc, const float* disp,
                             const float* guide, float* out_loss,
                             double* plane_sums, void* workspace,
                             size_t workspace_bytes, lsi_stream_t stream);
/* g_disp [L,B,H,W,1] contiguous, scaled by the device scalar g_loss; the
 * weights are recomputed from the guide.  Every element is written. */
int lsi_edge_smooth_loss_bwd(const LsiEdgeSmoothDesc* desc, const float* disp,
                             const float* guide, const double* plane_sums,
                             const float* g_loss, float* g_disp,
                             lsi_stream_t stream);

/*
 * Sparse depth-supervision loss (csrc/lsi_depth_sup.hip; no reference
 * counterpart, the definition is DESIGN.md section 4.20): the scale-invariant
 * log error of Eigen et al. 2014, or a plain L1, of predicted inverse depths
 * against a ground-truth map that is mostly holes.  pred [P,H,W] with the
 * element strides p_s*, gt [P,H,W] with the element strides g_s*, gt_scale P
 * device floats or NULL: g = gt * gt_scale[p] (one fp32 product; gt itself when
 * NULL) is the ground truth as inverse depth -- the convention of
 * lsi_eval_depth_metrics.  Pixel i of plane p is scored, a function of the
 * ground truth alone, when gt > valid_above and g_min <= g <= g_max (the caller
 * computes g_min = 1 / depth_max, g_max = 1 / depth_min once, in fp32); a NaN
 * ground truth fails every comparison.  n_p = scored pixels of plane p, S =
 * planes with n_p > 0.  q = fmaxf(pred, eps): a NaN prediction becomes eps.
 *   LSI_DEPTH_SUP_SILOG  d_i = logf(q_i) - logf(g_i) in fp32; in fp64
 *                        A_p = sum d_i, Q_p = sum d_i d_i (d_i widened, then
 *                        squared), D_p = Q_p / n_p - lambda (A_p / n_p)^2
 *                        loss = 1 / S sum_{n_p > 0} D_p
 *                        dloss/dpred_i = 1 / S (2 d_i / n_p - 2 lambda A_p /
 *                                        n_p^2) / q_i
 *   LSI_DEPTH_SUP_L1     e_i = q_i - g_i in fp32, A_p = sum |e_i| in fp64, Q_p = 0
 *                        loss = 1 / S sum_{n_p > 0} A_p / n_p
 *                        dloss/dpred_i = sign(e_i) / (n_p S), sign(0) = 0
 * The gradient is that where i is scored and pred_i > eps, 0 elsewhere; the
 * ground truth is data.  S = 0: loss 0, gradient all zeros.  No Inf or NaN
 * leaves either direction for finite or NaN inputs.  A pixel that is not scored
 * costs no read of pred, in either direction.
 * LSI_EINVAL for an unknown mode, non-positive dimensions (H W < 2^31),
 * g_min <= 0, g_max < g_min, valid_above < 0, eps <= 0, lambda outside [0, 1]
 * or a non-finite scalar; then LSI_ENULL (only gt_scale may be NULL); then
 * LSI_EWORKSPACE -- all before any launch.  No atomics, no host
 * synchronisation, no allocation: the same inputs give the same bits, and both
 * directions can be captured in a HIP graph.
 */
#define LSI_DEPTH_SUP_SILOG 0
#define LSI_DEPTH_SUP_L1 1
typedef struct LsiDepthSupDesc {
  int32_t P, H, W, mode;
  int64_t p_sp, p_sy, p_sx;
  int64_t g_sp, g_sy, g_sx;
  float valid_above, g_min, g_max, eps, lam; /* lam: lambda above */
  int32_t reserved;
} LsiDepthSupDesc;

/* (3 P bpp + P) doubles: a block covers r = max(ceil(1024 / W), ceil(H / 256))
 * rows of a plane, bpp = ceil(H / r) blocks per plane; 0 for a descriptor the
 * entries below refuse. */
size_t lsi_depth_sup_workspace_bytes(const LsiDepthSupDesc* desc);
/* 2 launches.  out_loss (one device float) = the loss; plane_sums (3 P device
 * doubles, the caller's) = n_p, A_p, Q_p at [3 p .. 3 p + 2]: written by the
 * finishing kernel, read by the backward.  The library keeps no state. */
int lsi_depth_sup_loss_fwd(const LsiDepthSupDesc* desc, const float* pred,
                           const float* gt, const float* gt_scale,
                           float* out_loss, double* plane_sums, void* workspace,
                           size_t workspace_bytes, lsi_stream_t stream);
/* 1 launch.  g_pred [P,H,W] contiguous, scaled by the device scalar g_loss;
 * validity and d_i are recomputed from the inputs, S from plane_sums.  Every
 * element is written. */
int lsi_depth_sup_loss_bwd(const LsiDepthSupDesc* desc, const float* pred,
                           const float* gt, const float* gt_scale,
                           const double* plane_sums, const float* g_loss,
                           float* g_pred, lsi_stream_t stream);

/*
 * Geometric-consistency loss between two views' inverse depths
 * (csrc/lsi_geo_cons.hip; no reference counterpart, the definition is DESIGN.md
 * section 4.21): the differentiable counterpart of lsi_disocclusion_mask.
 * disp [P,H,W] with the element strides d_s*, partner [P,H,W] with the element
 * strides e_s*, M [P,4,4] contiguous device floats.  Pixel (x, y) of plane p with
 * d = disp[p,y,x] is projected by M[p] under the renderer's floating-point
 * contract (every operation a separately rounded fp32 operation):
 *   q_j = ((px M[j][0] + py M[j][1]) + M[j][2]) + d M[j][3], px = x + .5, py = y + .5
 *   n = q_2, n' = n + 1e-8 [n == 0], u = q_0 / n', v = q_1 / n', dd = q_3 / n'
 *   s = c0 E00 + c1 E01 + c2 E10 + c3 E11 in that order: the bilinear sample of
 *       plane r = (p + shift) mod P of partner at (u, v), taps and weights as
 *       lsi_bilinear_fwd forms them (E01 is the tap at x0, y1)
 * The paired form is partner = disp with shift = P / 2; two tensors use shift 0.
 * The pixel is scored when d, u, v, dd are finite, n > 0, dd > 0,
 * 0.5 <= u <= W - 0.5, 0.5 <= v <= H - 0.5, s > 0 and, with occl_thresh > 0,
 * not s - dd > occl_thresh (s + dd) (the point would lie behind the partner's
 * visible surface).  With dd and s widened to fp64:
 *   LSI_GEO_CONS_RATIO   e = |dd - s| / (dd + s)
 *   LSI_GEO_CONS_L1      e = |dd - s|
 *   loss = 1 / S sum_{N_p > 0} (sum e over plane p) / N_p, N_p = scored pixels
 *   of plane p, S = planes with N_p > 0; 0 when S = 0.
 * Gradient w.r.t. disp and partner; the scored set and M are constants,
 * sign(dd - s) is that of the fp32 values, sign(0) = 0, g = g_loss / (S N_p):
 *   partner[r, tap k] += g de/ds c_k                      (c_k != 0)
 *   disp[p, y, x]     += g (de/ddd ddd/dd + de/ds (ds/du du/dd + ds/dv dv/dd))
 *   d(q_j / n')/dd = (M[j][3] n' - q_j M[2][3]) / n'^2; ds/du, ds/dv with the
 *   weights' derivatives those of x1 - x and x - x0 (floor has gradient 0)
 *   ratio: de/ddd = sign 2 s / (dd + s)^2, de/ds = -sign 2 dd / (dd + s)^2;
 *   l1: sign, -sign.
 * LSI_EINVAL for an unknown mode, non-positive dimensions, P > 65535,
 * H W >= 2^24, P H W > INT32_MAX, shift outside [0, P) or occl_thresh outside
 * [0, 1); then LSI_ENULL; then LSI_EWORKSPACE -- all before any launch.  No
 * host synchronisation, no allocation: both directions can be captured in a
 * HIP graph.  The forward has no atomics: the same inputs give the same loss,
 * plane sums and map bit for bit.  The backward adds with fp32 global atomics:
 * its last bits depend on the order the adds arrive in.
 */
#define LSI_GEO_CONS_RATIO 0
#define LSI_GEO_CONS_L1 1
typedef struct LsiGeoConsDesc {
  int32_t P, H, W, mode;
  int64_t d_sp, d_sy, d_sx;
  int64_t e_sp, e_sy, e_sx;
  int32_t shift;
  float occl_thresh;
} LsiGeoConsDesc;

/* (3 P bpp + P) doubles: a block covers r = max(ceil(1024 / W), ceil(H / 256))
 * rows of a plane, bpp = ceil(H / r) blocks per plane; 0 for a descriptor the
 * entries below refuse. */
size_t lsi_geo_cons_workspace_bytes(const LsiGeoConsDesc* desc);
/* 2 launches.  out_loss (one device float) = the loss; plane_sums (3 P device
 * doubles, the caller's) = sum e, N_p, 0 at [3 p .. 3 p + 2]: written by the
 * finishing kernel, read by the backward.  out_map [P,H,W] contiguous or NULL:
 * the per-pixel e as fp32, -1 where the pixel is not scored.  The library keeps
 * no state. */
int lsi_geo_cons_loss_fwd(const LsiGeoConsDesc* desc, const float* disp,
                          const float* partner, const float* M, float* out_loss,
                          double* plane_sums, float* out_map, void* workspace,
                          size_t workspace_bytes, lsi_stream_t stream);
/* 1 launch after the zero-fill of the outputs on the stream.  g_disp and
 * g_partner [P,H,W] contiguous, scaled by the device scalar g_loss.  g_partner
 * NULL (or g_disp itself) is the paired form: the taps' contributions land in
 * g_disp, at plane r, next to the pixels' own. */
int lsi_geo_cons_loss_bwd(const LsiGeoConsDesc* desc, const float* disp,
                          const float* partner, const float* M,
                          const double* plane_sums, const float* g_loss,
                          float* g_disp, float* g_partner, lsi_stream_t stream);

/*
 * Backward-warp photometric loss over the layers of an LDI
 * (csrc/lsi_photo_reproj.hip; no reference counterpart, the definition is
 * DESIGN.md section 4.23; Garg et al. 2016, Godard et al. 2017, Zhou et al. 2017).
 * tex [P,H,W,C] with C in 1 .. 4 and disp [P,H,W]; img [Q,H,W,C] with the element
 * strides i_s*, the images that are sampled; M [Q,4,4] contiguous; partner
 * [Q,H,W] with e_s* or NULL, the inverse depths of the sampled views' visible
 * surface.  Q divides P: plane p = l Q + q is layer l of view q = p mod Q, it
 * uses the matrix M[q] and the image and partner plane r = (q + shift) mod Q,
 * so L x B layers of B views are P = L B planes over Q = B images; a buffer of
 * 2 B views pairs each half with the other by shift = B.  Plane p of tex begins
 * at element l t_sl + q t_sq, of disp at l d_sl + q d_sq (a contiguous [P,...]
 * has t_sl = Q t_sq): the network's [L,Q,H,W,4] views of one [Q,H,W,L,4] buffer
 * are read in place.  Pixel (x, y) of plane p with
 * d = disp[p,y,x] is projected to (u, v, dd) by M[q] exactly as
 * lsi_geo_cons_loss_fwd projects it (q_j, n, n' above);
 *   s_c = the bilinear sample of img[r,:,:,c] at (u, v), taps, weights and order
 *         of lsi_bilinear_fwd.
 * The pixel is scored when d, u, v, dd are finite, n > 0, dd > 0,
 * 0.5 <= u <= W - 0.5, 0.5 <= v <= H - 0.5, every tex[p,y,x,c] and every s_c is
 * finite and, with occl_thresh > 0, the bilinear sample sd of partner[r] at
 * (u, v) is > 0 and not sd - dd > occl_thresh (sd + dd).  With tex_c and s_c
 * widened to fp64 and summed over c in order:
 *   LSI_PHOTO_L1      e = (1 / C) sum_c |tex_c - s_c|
 *   LSI_PHOTO_CHARB   e = (1 / C) sum_c sqrt((tex_c - s_c)^2 + eps^2)
 *   loss = 1 / S sum_{N_p > 0} (sum e over plane p) / N_p, N_p = scored pixels
 *   of plane p, S = planes with N_p > 0; 0 when S = 0.
 * Gradient w.r.t. tex and disp only; the scored set, M, img and partner are
 * constants, dd enters only the rule.  In fp32, x_c = tex_c - s_c, psi'(x) =
 * sign(x) (sign(0) = 0) or x / sqrt(x^2 + eps^2), g = g_loss / (S N_p):
 *   g_tex[p,y,x,c] = (g / C) psi'(x_c)
 *   g_disp[p,y,x]  = -(g / C) ((sum_c psi'(x_c) ds_c/du) du/dd +
 *                               (sum_c psi'(x_c) ds_c/dv) dv/dd)
 * with du/dd, dv/dd, ds/du, ds/dv the expressions of lsi_geo_cons_loss_bwd; 0
 * where the pixel is not scored.  Every cell of a requested gradient is stored
 * exactly once, by the thread of its pixel: no zero-fill, no atomics.
 * LSI_EINVAL for an unknown mode, non-positive dimensions, C outside 1 .. 4,
 * P > 65535, Q not a divisor of P, H W >= 2^24, P H W > INT32_MAX, shift
 * outside [0, Q), occl_thresh outside [0, 1) or eps not finite and > 0; then
 * LSI_ENULL (partner may be NULL only with occl_thresh == 0; it is not read
 * then); then LSI_EWORKSPACE -- all before any launch.  No host
 * synchronisation, no allocation: both directions can be captured in a HIP
 * graph, and in both the same inputs give the same bits.
 */
#define LSI_PHOTO_L1 0
#define LSI_PHOTO_CHARB 1
typedef struct LsiPhotoReprojDesc {
  int32_t P, Q, H, W, C, mode;
  int64_t t_sl, t_sq, t_sy, t_sx, t_sc;
  int64_t d_sl, d_sq, d_sy, d_sx;
  int64_t i_sq, i_sy, i_sx, i_sc;
  int64_t e_sq, e_sy, e_sx;
  int32_t shift;
  float occl_thresh, eps;
  int32_t reserved;
} LsiPhotoReprojDesc;

/* (3 P bpp + P) doubles: a block covers r = max(ceil(1024 / W), ceil(H / 256))
 * rows of a plane, bpp = ceil(H / r) blocks per plane; 0 for a descriptor the
 * entries below refuse. */
size_t lsi_photo_reproj_workspace_bytes(const LsiPhotoReprojDesc* desc);
/* 2 launches.  out_loss (one device float) = the loss; plane_sums (3 P device
 * doubles, the caller's) = sum e, N_p, 0 at [3 p .. 3 p + 2]: written by the
 * finishing kernel, read by the backward.  out_map [P,H,W] contiguous or NULL:
 * the per-pixel e as fp32, -1 where the pixel is not scored.  The library keeps
 * no state. */
int lsi_photo_reproj_loss_fwd(const LsiPhotoReprojDesc* desc, const float* tex,
                              const float* disp, const float* img, const float* M,
                              const float* partner, float* out_loss,
                              double* plane_sums, float* out_map, void* workspace,
                              size_t workspace_bytes, lsi_stream_t stream);
/* 1 launch.  g_tex [P,H,W,C] and g_disp [P,H,W] contiguous, scaled by the
 * device scalar g_loss; either may be NULL (not both): its work is skipped. */
int lsi_photo_reproj_loss_bwd(const LsiPhotoReprojDesc* desc, const float* tex,
                              const float* disp, const float* img, const float* M,
                              const float* partner, const double* plane_sums,
                              const float* g_loss, float* g_tex, float* g_disp,
                              lsi_stream_t stream);

/*
 * layers.compose, lsi/geometry/layers.py:29-70 with helpers.soft_z_buffering
 * (lsi/nnutils/helpers.py:140-160): white background layer at min_disp,
 * per-pixel softmax of log(mask + 1e-8) - depth / temp over the L + 1 layers,
 * hard (first arg-max of the probabilities) or soft blend.
 * imgs [L,N,C], masks [L,N], dmaps [L,N], out [N,C]; all contiguous.
 */
int lsi_compose_fwd(int32_t L, int64_t N, int32_t C, const float* imgs,
                    const float* masks, const float* dmaps, int32_t soft,
                    float min_disp, float depth_softmax_temp, float* out,
                    lsi_stream_t stream);
/* layers.compose_depth, layers.py:73-115.  dmax = max(relu(dmaps), min_disp)
 * over the whole tensor (used when bg_layer != 0).  out [N]. */
int lsi_compose_depth_fwd(int32_t L, int64_t N, const float* masks,
                          const float* dmaps, int32_t bg_layer, float dmax,
                          float min_disp, float depth_softmax_temp, float* out,
                          lsi_stream_t stream);
/*
 * Gradients of lsi_compose_fwd / lsi_compose_depth_fwd: TF autodiff of the same
 * op graph, per pixel, no atomics; the selected layer is the forward's.  The
 * forward's arguments, then g_out [N,C] (compose) or [N] (compose_depth).
 * g_imgs [L,N,C], g_masks [L,N], g_dmaps [L,N]: each may be NULL (its work is
 * skipped); every element of a requested one is written (no zeroing needed).
 * Hard composition passes g_out to the winning layer's image and nothing else;
 * compose_depth passes it to the winning layer's disparity where that is > 0
 * (the selection disparity dmax - d only chooses the layer).  The background
 * layer takes no gradient.
 */
int lsi_compose_bwd(int32_t L, int64_t N, int32_t C, const float* imgs,
                    const float* masks, const float* dmaps, int32_t soft,
                    float min_disp, float depth_softmax_temp, const float* g_out,
                    float* g_imgs, float* g_masks, float* g_dmaps,
                    lsi_stream_t stream);
int lsi_compose_depth_bwd(int32_t L, int64_t N, const float* masks,
                          const float* dmaps, int32_t bg_layer, float dmax,
                          float min_disp, float depth_softmax_temp,
                          const float* g_out, float* g_dmaps, lsi_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Evaluation metrics accumulated on the device (csrc/lsi_eval.hip): the     */
/* arithmetic of ldi_pred_eval.py:297-548 (define_metrics), one pass per     */
/* rendered view / pair of LDIs.  The running sums live in a caller-owned    */
/* device array `acc` of LSI_EVAL_SLOTS doubles, zeroed by the caller once;  */
/* every call ADDS to its slots in a one-block finishing kernel on the       */
/* caller's stream (stream order serialises the calls that share an          */
/* accumulator and a workspace).  No atomics: the same sequence of calls     */
/* gives the same 16 doubles bit for bit.  No host synchronisation.  A       */
/* metric whose optional inputs are absent leaves its slots untouched.       */
/* ------------------------------------------------------------------------ */
#define LSI_EVAL_COMPOSE_SUM 0         /* compose_splat_loss                  */
#define LSI_EVAL_COMPOSE_NORM 1
#define LSI_EVAL_COMPOSE_DISOCC_SUM 2  /* compose_splat_loss_disocc           */
#define LSI_EVAL_COMPOSE_DISOCC_NORM 3
#define LSI_EVAL_DEPTH_SUM 4           /* depth_splat_loss                    */
#define LSI_EVAL_DEPTH_NORM 5
#define LSI_EVAL_DEPTH_DISOCC_SUM 6    /* depth_splat_loss_disocc             */
#define LSI_EVAL_DEPTH_DISOCC_NORM 7
#define LSI_EVAL_PSNR_SUM 8            /* psnr: dB summed over the calls      */
#define LSI_EVAL_PSNR_COUNT 9
#define LSI_EVAL_FG_TEX_SUM 10         /* fg_tex_error                        */
#define LSI_EVAL_FG_DISP_SUM 11        /* fg_disp_error                       */
#define LSI_EVAL_FG_NORM 12
#define LSI_EVAL_BG_TEX_SUM 13         /* bg_tex_error                        */
#define LSI_EVAL_BG_DISP_SUM 14        /* bg_disp_error                       */
#define LSI_EVAL_BG_NORM 15
#define LSI_EVAL_SLOTS 16

#define LSI_EVAL_DISOCC_U8 1u  /* disocc holds one-byte bools, not floats     */
#define LSI_EVAL_VALID_GT 2u   /* valid holds a map to threshold: a pixel is  */
                               /* valid (1) where it exceeds valid_thresh     */

/* Bytes of device scratch (partial sums) the two metric calls need. */
size_t lsi_eval_workspace_bytes(void);

/*
 * The view-synthesis metrics of one rendered view (ldi_pred_eval.py:385-460),
 * one pass over the B x Ht x Wt cells:
 *   recons [nl,B,Ht,Wt,3], recons_disp [nl,B,Ht,Wt,1] (may be NULL): contiguous
 *   target [B,H,W,3] with element strides, H = fy Ht, W = fx Wt
 *   valid [B,H,W] (may be NULL: ones), disocc [B,H,W] fp32 or one-byte bool
 *   (LSI_EVAL_DISOCC_U8; may be NULL), gt_disp [B,H,W] (may be NULL): contiguous
 * Per cell every full-resolution input is box-averaged over its fy x fx block
 * (the AREA resize); valid = mean > 0.95; centre = [x_min <= x < Wt - x_min and
 * y_min <= y < Ht - y_min] * valid; pw = min_l mean_c |t - r_l| * centre;
 * se = mean_c (t - r_0)^2 * centre; dm = the un-thresholded mean of disocc;
 * pd = min_l |gt - rd_l| * centre.  Added to acc:
 *   slots 0, 1: sum pw, sum centre          2, 3: sum pw dm, sum centre dm
 *   slots 4, 5: sum pd, sum centre          6, 7: sum pd dm, sum centre dm
 *   slots 8, 9: 10 log10(1 / max(sum se / sum centre, 1e-20)), 1 -- only when
 *               sum centre > 0: a call without a scored cell adds nothing
 * Slots 4-7 need recons_disp and gt_disp, slots 2, 3, 6, 7 need disocc.  Cells
 * with centre = 0 are not read.
 */
int lsi_eval_view_metrics(int32_t nl, int32_t B, int32_t Ht, int32_t Wt,
                          int32_t H, int32_t W, int32_t x_min, int32_t y_min,
                          const float* recons, const float* recons_disp,
                          const float* target, int64_t t_sb, int64_t t_sy,
                          int64_t t_sx, int64_t t_sc, const float* valid,
                          const void* disocc, const float* gt_disp,
                          uint32_t flags, float valid_thresh, double* acc,
                          void* workspace, size_t workspace_bytes,
                          lsi_stream_t stream);

/*
 * The per-layer metrics of a pair of predicted LDIs (ldi_pred_eval.py:476-531),
 * one pass over B x H x W for both views.  Per view a descriptor gives L, B, H, W,
 * bg_layer_disp and the element strides of tex (img_s*) and disp (disp_s*), so
 * permuted convolution outputs and the packed RGBD head output are read in
 * place; only layers 0 and L - 1 are read.  img [B,H,W,3], gt_disp [B,H,W],
 * gt_disp_bg [B,H,W] and gt_tex_bg [B,H,W,3] are contiguous; the two *_bg inputs
 * are given for both views or for neither (else LSI_EINVAL).  The descriptors
 * must agree in L, B, H, W and bg_layer_disp.  With v = gt_disp > bg_layer_disp
 * and b = gt_disp > gt_disp_bg, added to acc:
 *   slots 10, 11, 12: sum_c |tex_0 - img| v / 3, sum |disp_0 - gt_disp| v, sum v
 *   slots 13, 14, 15: sum_c |tex_{L-1} - gt_tex_bg| b / 3,
 *                     sum |disp_{L-1} - gt_disp_bg| b, sum b    (with the *_bg)
 */
int lsi_eval_layer_metrics(const LsiLossDesc* src_desc, const float* src_tex,
                           const float* src_disp, const float* src_img,
                           const float* src_gt_disp, const float* src_gt_disp_bg,
                           const float* src_gt_tex_bg, const LsiLossDesc* trg_desc,
                           const float* trg_tex, const float* trg_disp,
                           const float* trg_img, const float* trg_gt_disp,
                           const float* trg_gt_disp_bg, const float* trg_gt_tex_bg,
                           double* acc, void* workspace, size_t workspace_bytes,
                           lsi_stream_t stream);

/*
 * Depth accuracy of a predicted inverse-depth map (csrc/lsi_depth_metrics.hip;
 * no reference counterpart, the definition is DESIGN.md section 4.16): the
 * seven figures of Eigen et al. 2014 per image, summed over the scored images
 * into an accumulator of its own, `acc` of LSI_DEPTH_SLOTS device doubles
 * (zeroed by the caller once; not part of the LSI_EVAL_SLOTS doubles).
 *   pred [B,H,W] predicted inverse depth, gt [B,H,W] a ground-truth map that
 *   gt_scale[b] (B device floats) turns into inverse depth, mask [B,H,W] fp32 or
 *   one-byte bool (LSI_DEPTH_MASK_U8; may be NULL): contiguous
 * Per pixel in fp32, dg = 1 / (gt gt_scale[b]).  It is scored -- the set V_b, a
 * function of the ground truth alone -- when gt > valid_above, y0 <= y < y1,
 * x0 <= x < x1, the mask is absent or non-zero and depth_min <= dg <= depth_max.
 * dp_raw = 1 / fmaxf(pred, FLT_MIN): a zero, negative or NaN prediction is a
 * huge finite depth, and no Inf or NaN reaches acc from such predictions.  (A
 * +Inf prediction is depth 0, clamped to depth_min; the caller keeps +Inf out
 * of a median-scaled call: were half an image's scored predictions +Inf, the
 * median depth would be 0 and s_b = Inf would be added to LSI_DEPTH_SCALE.)
 * s_b = 1, or with LSI_DEPTH_MEDIAN
 * (float)(med(dg over V_b) / med(dp_raw over V_b)): exact order statistics of
 * the fp32 values (a radix select on the device), the two middle values of an
 * even count averaged, mean and quotient in fp64.
 *   dp = fminf(fmaxf(s_b dp_raw, depth_min), depth_max), e = dg - dp
 *   terms |e| / dg, e e / dg, e e, (logf(dg) - logf(dp))^2
 *   r = fmaxf(dg / dp, dp / dg) < 1.25, 1.25^2, 1.25^3
 * Per image with n_b = |V_b| > 0, sums in fp64: abs_rel, sq_rel = sum / n_b;
 * rmse, rmse_log = sqrt(sum / n_b); a1..a3 = count / n_b.  Each is ADDED to its
 * slot, s_b to LSI_DEPTH_SCALE and 1 to LSI_DEPTH_IMAGES, images in index
 * order, by a one-block finishing kernel; an image without a scored pixel adds
 * nothing.  per_image (may be NULL): B x LSI_DEPTH_PER_IMAGE device doubles,
 * overwritten with the image's seven figures, s_b, n_b and 1 (all zeros for an
 * image that is not scored).  Pixels outside the crop are not read.
 * LSI_EINVAL for non-positive dimensions (B <= 65535), an empty or
 * out-of-range crop, depth_min <= 0, depth_max < depth_min, valid_above < 0 or
 * unknown flags; then LSI_ENULL for a NULL pred, gt, gt_scale, acc or
 * workspace; then LSI_EWORKSPACE -- all before any launch.  2 launches, 10
 * with LSI_DEPTH_MEDIAN, whatever the data; no floating-point atomics, no
 * host synchronisation: the same sequence of calls gives the same doubles bit
 * for bit.
 */
#define LSI_DEPTH_ABS_REL 0
#define LSI_DEPTH_SQ_REL 1
#define LSI_DEPTH_RMSE 2
#define LSI_DEPTH_RMSE_LOG 3
#define LSI_DEPTH_A1 4
#define LSI_DEPTH_A2 5
#define LSI_DEPTH_A3 6
#define LSI_DEPTH_SCALE 7      /* sum of s_b over the scored images            */
#define LSI_DEPTH_IMAGES 8     /* number of scored images                      */
#define LSI_DEPTH_SLOTS 9
#define LSI_DEPTH_PER_IMAGE 10 /* per_image row: slots 0-7 of the image, n_b,  */
                               /* scored (0 or 1)                              */

#define LSI_DEPTH_MASK_U8 1u   /* mask holds one-byte bools, not floats        */
#define LSI_DEPTH_MEDIAN 2u    /* per-image median scaling                     */

/* Bytes of device scratch lsi_eval_depth_metrics needs for B x H x W maps (any
 * crop), more with median != 0; 0 for dimensions the call refuses. */
size_t lsi_eval_depth_workspace_bytes(int32_t B, int32_t H, int32_t W,
                                      int32_t median);
int lsi_eval_depth_metrics(int32_t B, int32_t H, int32_t W, const float* pred,
                           const float* gt, const void* mask,
                           const float* gt_scale, int32_t y0, int32_t y1,
                           int32_t x0, int32_t x1, float valid_above,
                           float depth_min, float depth_max, uint32_t flags,
                           double* acc, double* per_image, void* workspace,
                           size_t workspace_bytes, lsi_stream_t stream);

/*
 * projection.disocclusion_mask (lsi/geometry/projection.py:109-150) for source
 * points on the pixel-centre grid: (x + .5, y + .5, 1, disps_src) through
 * M [B,4,4] under the floating-point contract of the renderer, divide_safe,
 * the four taps of disps_trg [B,Ht,Wt,1] as lsi_bilinear_fwd takes them;
 * mask [B,Hs,Ws,1] = [|d_src->trg - sampled| > thresh], 0 where the projected
 * point leaves the target (u > Wt, v > Ht, u < 0 or v < 0).
 */
int lsi_disocclusion_mask(int32_t B, int32_t Hs, int32_t Ws, int32_t Ht,
                          int32_t Wt, const float* disps_src,
                          const float* disps_trg, const float* M, float thresh,
                          float* mask, lsi_stream_t stream);

/*
 * Fused renderer of batches of planar scenes (lsi/data/synthetic_planes.py):
 * B worlds of P textured planes, V views each, in ONE launch.  Per view pixel
 * and plane: q = hom (x + .5, y + .5, 1), divide_safe, the four bilinear taps
 * of the RGBA texel (A = the plane's mask), the analytic disparity
 * dmat (x + .5, y + .5, 1); then layers.compose (hard: first maximum of the
 * soft z-buffer probabilities; or soft) and layers.compose_depth
 * (bg_layer = False) over the P planes + the white background layer at
 * min_disp.  The result is, bit for bit, what homography.transform_plane_imgs
 * -> trg_disp_maps -> lsi_compose_fwd / lsi_compose_depth_fwd give; the warped
 * layers are never written to memory.  The *_ROOM outputs are the same
 * composition with the masks of the planes [n_box, P) taken as 0 (the room
 * without its objects).
 *   tex_rgba [B,P,Hs,Ws,4] (16-byte aligned; Hs*Ws <= 2^24)
 *   hom      [B,V,P,9]  homography.inv_homography, row-major (view px -> texture px)
 *   dmat     [B,V,P,3]  homography.inv_homography_dmat
 *   img / img_room   [B,V,H,W,3]     disp / disp_room [B,V,H,W,1]
 * Only the outputs named in `outputs` are written; their pointers must not be
 * NULL (LSI_ENULL), the others may be.  1 <= P <= LSI_SCENE_MAX_PLANES,
 * 0 <= n_box <= P, positive sizes, at least one known output bit -- else
 * LSI_EINVAL, before any launch.  No workspace, no state.
 */
#define LSI_SCENE_MAX_PLANES 16
#define LSI_SCENE_IMG 1u
#define LSI_SCENE_DISP 2u
#define LSI_SCENE_IMG_ROOM 4u
#define LSI_SCENE_DISP_ROOM 8u
typedef struct LsiSceneDesc {
  int32_t B, V, P;        /* worlds, views per world, planes per world       */
  int32_t Hs, Ws;         /* plane texture size                              */
  int32_t H, W;           /* view size                                       */
  int32_t n_box;          /* planes [n_box, P) are objects (*_ROOM outputs)  */
  int32_t soft;           /* layers.compose(soft=...) for the images         */
  float min_disp, temp;   /* compose / compose_depth arguments               */
  uint32_t outputs;       /* LSI_SCENE_* bits                                */
} LsiSceneDesc;
int lsi_render_planes(const LsiSceneDesc* desc, const float* tex_rgba,
                      const float* hom, const float* dmat, float* img,
                      float* disp, float* img_room, float* disp_room,
                      lsi_stream_t stream);
/*
 * Gradients of lsi_render_planes' img and disp outputs (TF autodiff of the op
 * route's graph; the layer that wins here is the layer that won there).  The
 * descriptor is the forward's, without *_ROOM bits (LSI_EINVAL: the room
 * outputs are forward-only).
 *   g_img  [B,V,H,W,3], g_disp [B,V,H,W,1]: upstream gradients; either may be
 *          NULL (zero), not both (LSI_ENULL)
 *   g_tex  [B,P,Hs,Ws,4]: ACCUMULATED into with float atomics -- the caller
 *          zeroes it (as g_imgs of lsi_bilinear_bwd); its summation order, and
 *          so its last bits, vary from run to run
 *   g_hom  [B,V,P,9], g_dmat [B,V,P,3]: written fully, reproducible bit for bit
 * Any output may be NULL and its work is skipped.  g_hom / g_dmat need
 * lsi_render_planes_bwd_workspace_bytes(desc) bytes of workspace (one partial
 * sum per workgroup; LSI_ENULL / LSI_EWORKSPACE if missing / smaller; bytes
 * beyond that size are not touched); g_tex alone needs none.  A plane-pixel
 * whose texture coordinate is not finite samples 0 and sends no gradient.
 */
size_t lsi_render_planes_bwd_workspace_bytes(const LsiSceneDesc* desc);
int lsi_render_planes_bwd(const LsiSceneDesc* desc, const float* tex_rgba,
                          const float* hom, const float* dmat, const float* g_img,
                          const float* g_disp, float* g_tex, float* g_hom,
                          float* g_dmat, void* workspace, size_t workspace_bytes,
                          lsi_stream_t stream);

/*
 * Fused batch norm (batch statistics) + beta + ReLU of the reference's conv
 * layers: slim.batch_norm(center=True, scale=False, epsilon, is_training=True)
 * followed by tf.nn.relu (nets.py:44-67, 95-111, 265-347).  x, y, dy, dx:
 * npix x C values, C innermost (torch channels_last), fp32 (bf16 = 0) or
 * bfloat16 (bf16 = 1); C a multiple of 4 (fp32) / 8 (bf16) with C / that a
 * power of two <= 256, C <= 2048 -- else LSI_EINVAL.  Statistics in fp32
 * (shifted sums, fp32 device atomics across workgroups), biased variance
 * (tf.nn.moments).  relu = 0: batch norm only.
 *   groups: the npix x C arrays are `groups` such blocks stored one after the
 *   other (sub-batches along N), each normalised with its own statistics -- the
 *   reference runs its network once per view, so a batch holding both views
 *   keeps two sets (one launch per pass for all groups).
 *   workspace: lsi_bn_workspace_floats(npix, C, bf16, groups) floats,
 *   ZERO-FILLED ONCE by the caller and then reusable by any later call on the
 *   same stream (the library leaves its counters and accumulators zero).
 *   mean_rstd: [groups][2][C] out (forward), in (backward).  dbeta: [C] out
 *   (summed over the groups).
 */
size_t lsi_bn_workspace_floats(int64_t npix, int32_t C, int32_t bf16, int32_t groups);
/* Host only: the workgroups per group (grid.x; grid.y = groups) that every pass
 * of lsi_bn_relu_fwd / _norm / _bwd launches for these arguments, 0 for a shape
 * they refuse.  A workgroup of 256 threads covers rows = 256 / (C / vector)
 * pixels per step and advances by workgroups * rows. */
int32_t lsi_bn_launch_workgroups(int64_t npix, int32_t C, int32_t bf16, int32_t groups);
int lsi_bn_relu_fwd(const void* x, void* y, const float* beta, float* workspace,
                    float* mean_rstd, int64_t npix, int32_t C, int32_t bf16,
                    int32_t relu, float eps, int32_t groups, lsi_stream_t stream);
int lsi_bn_relu_bwd(const void* x, const void* dy, const float* mean_rstd,
                    const float* beta, void* dx, float* dbeta, float* workspace,
                    int64_t npix, int32_t C, int32_t bf16, int32_t relu,
                    int32_t groups, lsi_stream_t stream);
/* lsi_bn_relu_fwd behind a producer that left the sums of x and x * x in
 * `workspace` (lsi_conv2d_fwd_bnstats / lsi_conv2d_bwd_data_bnstats on the same
 * stream): one pass -- y = relu((x - mean) * rstd + beta), mean_rstd out as from
 * lsi_bn_relu_fwd --, accumulators cleared for the next producer.
 *   Numerical contract (tests/test_bn_stats_cpu.py derives it, test_bn_stats_gpu.py
 * holds every producer to it): the sums are plain fp32 and var = E[x^2] - mean^2
 * is formed in fp32, clamped at 0, so per channel, with m and v the exact mean
 * and biased variance of the stored tensor,
 *     |rstd / rsqrt(v + eps) - 1|  <=  2^-20 * (v + m^2) / (v + eps) + 2^-22,
 *     |mean - m|                   <=  1e-5 * max|x|.
 * At mean ~ 0 that is rstd to ~1e-6; at |m| = 100 sigma up to 1e-2 is allowed
 * (measured on the MI355X: ~1e-3, profiles/bn_stats/errors.txt) -- below the
 * bf16 rounding of y.  A constant channel gives var within rounding of 0 and
 * y = relu(beta).  lsi_bn_relu_fwd (sums around a per-channel shift -- the median
 * of the channel at three pixels of the group --, fp64 finish) keeps rstd to 2e-5
 * at every m / sigma, one of those pixels an outlier included.  Both normalise
 * as (x - mean) * rstd + beta, which a constant channel leaves as beta exactly. */
int lsi_bn_relu_norm(const void* x, void* y, const float* beta, float* workspace,
                     float* mean_rstd, int64_t npix, int32_t C, int32_t bf16, int32_t relu,
                     float eps, int32_t groups, lsi_stream_t stream);
/* The hand-over between a producer of statistics and lsi_bn_relu_norm is checked
 * on the device: the producer leaves a tag (C, groups) next to its sums, which
 * lsi_bn_relu_norm requires and clears, and which lsi_bn_relu_fwd / _bwd require
 * to be absent.  A call that finds the workspace in the other state writes NaN
 * (y, mean_rstd / dx, dbeta) instead of numbers computed from somebody else's
 * sums, and leaves the workspace clean.  lsi_bn_stats_discard drops statistics
 * whose consumer will not run (an error between the two calls): the first
 * 16 + 4096 floats of every group's block are zeroed on the stream. */
int lsi_bn_stats_discard(float* workspace, int32_t groups, lsi_stream_t stream);

/*
 * 3x3 stride-1 SAME convolution over 32 input channels on the matrix cores
 * (v_mfma_f32_16x16x32_bf16, fp32 accumulation): the full-resolution layers of
 * the LDI heads.
 *   mode 0  `upcnv1b` (nets.py:104-111): cout = 16 or 32, output bf16
 *           N x H x W x cout (before batch norm);
 *   mode 1  `pred_l` (nets.py:150-158): cout <= 4, bias, sigmoid, output fp32
 *           N x H x W x 4 -- RGBD pixels; scale3 must be 1 (LSI_EINVAL
 *           otherwise: lsi_conv3x3_pred_bwd reads sigmoid' off the stored
 *           output; the caller multiplies the disparities by max_disp);
 *   mode 2  the data gradient of mode 0 with cout = 32: the same convolution
 *           with the kernel transposed and flipped (x = the incoming gradient).
 *   x: bf16 N x H x W x 32, channels innermost (torch channels_last), 16-byte
 *   aligned; W % 16 == 0.  weight: the layer's fp32 parameter cout x 32 x 3 x 3
 *   (rounded to bf16 in the kernel, as torch.autocast does).  bias: [cout]
 *   fp32 or NULL (mode 1).
 */
int lsi_conv3x3_c32_fwd(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t mode,
                        const void* x, const float* weight, const float* bias,
                        float scale3, void* out, lsi_stream_t stream);

/*
 * Backward of the prediction head `pred_l` (nets.py:150-158; TF autodiff of
 * conv + bias + sigmoid): y = sigmoid(conv(x, W) + b), cout <= 4.
 *   g, y: fp32 N x H x W x 4 (the incoming gradient and the forward's output,
 *   RGBD pixels; channels >= cout ignored); x: bf16 N x H x W x 32 (needed for
 *   g_wb); weight: fp32 cout x 32 x 3 x 3.
 *   g_x (may be NULL): bf16 N x H x W x 32, the data gradient (MFMA, K = 9 taps
 *   x 4 channels).  g_wb (may be NULL): fp32 [cout * 288 + cout], weight
 *   gradient cout x 32 x 3 x 3 followed by the bias gradient (matrix cores, K =
 *   pixels, sigmoid'(z) * g as bf16 hi + lo); written (not added to).
 *   sigmoid'(z) * g is formed in fp32 registers and never written.
 *   workspace (needed with g_wb): lsi_conv3x3_pred_bwd_workspace_bytes(N, H, W)
 *   bytes, 16-byte aligned -- the pixel blocks' partial sums, folded by a second
 *   kernel (LSI_EWORKSPACE if smaller).
 */
size_t lsi_conv3x3_pred_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W);
int lsi_conv3x3_pred_bwd(int32_t N, int32_t H, int32_t W, int32_t cout, const float* g,
                         const float* y, const void* x, const float* weight, void* g_x,
                         float* g_wb, void* workspace, size_t workspace_bytes,
                         lsi_stream_t stream);

/*
 * Weight gradient of a 3x3 stride-1 SAME convolution on channels-last bf16
 * tensors (reference nets.py:104-111, the `upcnv*b` layers of the LDI heads; TF
 * autodiff of slim.conv2d):
 *   g_weight[co][ci][ky][kx] = sum over n, y, x of
 *       gy[n][y][x][co] * x[n][y + ky - 1][x + kx - 1][ci]        (zero outside)
 *   x: bf16 N x H x W x cin, gy: bf16 N x H x W x cout (16-byte aligned),
 *   g_weight: fp32 cout x cin x 3 x 3, written (not added to).  cin and cout
 *   multiples of 32 (LSI_EUNSUPPORTED otherwise).  MFMA with K = pixels,
 *   operands transposed by the LDS transpose read; fp32 accumulation.
 *   workspace: lsi_conv3x3_wgrad_workspace_bytes(...) bytes, 16-byte aligned
 *   (partial sums of the pixel blocks; LSI_EWORKSPACE if smaller).
 */
size_t lsi_conv3x3_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cin,
                                         int32_t cout);
int lsi_conv3x3_wgrad(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout,
                      const void* x, const void* gy, float* g_weight, void* workspace,
                      size_t workspace_bytes, lsi_stream_t stream);

/*
 * The compact STREAM kernel has two builds (12 waves x two items in flight, 16 x
 * one); which is faster depends on the disparity field, which the planner does
 * not see.  With LsiSplatDesc.adapt set, the kernel counts the items that took
 * its folded routes on a few probe launches (the first calls with the record,
 * then two of every 64); a later call reads the count -- asynchronously copied
 * to the record's pinned host memory, never waited for -- and picks the build.
 * All of that state is the caller's record; with adapt == NULL a call is a pure
 * function of its descriptor (the planner's choice: 12 x 2 for large launches).
 * tune_threads != 0, LSI_S2_WIDE and LSI_S2_ADAPT=0 switch the mechanism off;
 * launches under stream capture use the standing decision and probe nothing.
 * Both builds render the same pixels (both are parity-tested); only timing
 * depends on the record.
 * lsi_stream_adapt_state: the record's standing decision after looking for a
 * pending probe's counts: 0 undecided, 1 twelve waves, 2 sixteen waves, -1 NULL.
 */
int lsi_stream_adapt_state(LsiStreamAdapt* a);

/*
 * Convolutions of the encoder-decoder and the LDI heads on the matrix cores
 * (reference nets.py:29-70 encoder, 73-114 decoder_simple, 244-348 U-Net:
 * slim.conv2d k x k stride 1 | 2 with TF `SAME` padding, slim.conv2d_transpose
 * 4 x 4 stride 2; TF autodiff for the data gradients) as implicit GEMMs
 * (v_mfma_f32_16x16x32_bf16, fp32 accumulation) on bf16 channels-last tensors.
 * LsiConvDesc describes the FORWARD convolution
 *   out[n][oy][ox][co] = sum x[n][oy*stride + ky - pad_t][ox*stride + kx - pad_l][ci]
 *                            * weight[co][ci][ky][kx]            (zero outside)
 *   x: bf16 N x H x W x Cin, out: bf16 N x OH x OW x Cout (16-byte aligned),
 *   weight: the layer's fp32 parameter Cout x Cin x KH x KW (rounded to bf16 on
 *   the way into the kernel's operand order, as torch.autocast rounds it: see
 *   lsi_conv2d_pack below).
 *   Cin, Cout multiples of 32; KH, KW <= 7; stride 1 or 2; pad < kernel size
 *   (LSI_EUNSUPPORTED otherwise: lsi_conv2d_supported() tells beforehand).
 * lsi_conv2d_bwd_data: gx[n][iy][ix][ci] = the transpose of the above applied
 *   to gy (N x OH x OW x Cout) -- for stride 2 as four stride-1 sums over the
 *   sub-kernels of the input pixels' parity classes, no zero-stuffed tensor.
 * A transposed convolution (torch ConvTranspose2d(Cin_T, Cout_T, k, stride,
 * padding p), weight Cin_T x Cout_T x k x k, input N x h x w x Cin_T) IS the
 * data gradient of the forward convolution {H = stride h, W = stride w,
 * Cin = Cout_T, OH = h, OW = w, Cout = Cin_T, pad_t = pad_l = p} with the same
 * weight memory: its forward is lsi_conv2d_bwd_data of that descriptor, its
 * data gradient lsi_conv2d_fwd.
 * The weights enter in the kernels' operand order, bf16 [tap][out ch][in ch]:
 * lsi_conv2d_pack(d, mode, weight, packed, ...) writes it from the layer's fp32
 * parameter -- mode 0 for lsi_conv2d_fwd, mode 1 for lsi_conv2d_bwd_data (roles
 * of the channels swapped, taps in parity-class order) -- into
 * lsi_conv2d_packed_bytes(d) bytes (16-byte aligned; LSI_EWORKSPACE if
 * smaller).  mode | 2: the parameter is stored with torch's channels-last
 * strides (Cout x KH x KW x Cin in memory: what module.to(memory_format=
 * torch.channels_last) leaves) instead of contiguously.  A caller whose weights
 * have not changed may keep the packed form -- and one whose optimiser updates
 * them has to pack again after every update (torch's fused optimisers do not
 * move a parameter's version counter: a stale pack is silent).
 */
typedef struct LsiConvDesc {
  int32_t N, H, W, Cin;    /* input  N x H x W x Cin   */
  int32_t OH, OW, Cout;    /* output N x OH x OW x Cout */
  int32_t KH, KW, stride;  /* kernel size; 1 or 2       */
  int32_t pad_t, pad_l;    /* zero rows / columns before the input (TF SAME: total / 2) */
} LsiConvDesc;
int lsi_conv2d_supported(const LsiConvDesc* d);
size_t lsi_conv2d_packed_bytes(const LsiConvDesc* d);
int lsi_conv2d_pack(const LsiConvDesc* d, int32_t mode, const float* weight, void* packed,
                    size_t packed_bytes, lsi_stream_t stream);
/* Many layers packed by ONE launch (a training step re-packs every layer after
 * the optimiser's update: one launch instead of two per layer):
 * lsi_conv2d_pack_job fills a host-side job record for (d, mode, weight, packed)
 * and the number of workgroups it needs; the caller sets block0 of every record
 * to the running sum, copies the table to the device and passes it to
 * lsi_conv2d_pack_many with the total. */
typedef struct LsiPackJob {
  const float* w;     /* the layer's parameter Cout x Cin x KH x KW          */
  void* dst;          /* packed bf16 weights                                  */
  int32_t D0, D1, khw, tr, ntaps, block0;
  int8_t tap[56];     /* ky * KW + kx of every tap, in the kernel's order     */
} LsiPackJob;
int lsi_conv2d_pack_job(const LsiConvDesc* d, int32_t mode, const float* weight, void* packed,
                        size_t packed_bytes, LsiPackJob* job, int32_t* nblocks);
int lsi_conv2d_pack_many(const LsiPackJob jobs_device[], int32_t njobs, int32_t total_blocks,
                         lsi_stream_t stream);
int lsi_conv2d_fwd(const LsiConvDesc* d, const void* x, const void* packed, void* out,
                   lsi_stream_t stream);
int lsi_conv2d_bwd_data(const LsiConvDesc* d, const void* gy, const void* packed, void* gx,
                        lsi_stream_t stream);
/*
 * The same two calls for a layer that slim.batch_norm follows (every
 * slim.conv2d / conv2d_transpose of nets.py:44-67, 95-111, 265-347): the
 * kernel's epilogue also adds the sums of y and y * y of its (bf16-rounded)
 * output -- per channel and sub-batch group, what lsi_bn_relu_fwd's first pass
 * would read the tensor back for -- to the accumulators of `bn_workspace`
 * (lsi_bn_workspace_floats; zero-filled once).  The caller completes the layer
 * with lsi_bn_relu_norm(out, y, ...) as the NEXT call that uses this workspace
 * on the stream: it folds the sums, forms mean / rstd and clears the
 * accumulators.  groups must divide N.  (Plain sums, no shift: a layer whose
 * |mean| is 10^3 times its standard deviation loses the variance -- not a
 * convolution without bias behind a batch norm.)
 */
int lsi_conv2d_fwd_bnstats(const LsiConvDesc* d, const void* x, const void* packed, void* out,
                           float* bn_workspace, int32_t groups, lsi_stream_t stream);
int lsi_conv2d_bwd_data_bnstats(const LsiConvDesc* d, const void* gy, const void* packed,
                                void* gx, float* bn_workspace, int32_t groups,
                                lsi_stream_t stream);
/*
 * A convolution behind a skip connection (tf.concat([a, b], axis=3) in front of
 * slim.conv2d: nets.py:104-106 `upcnv{n}b`, :300-345 `icnv{n}`): the input as
 * TWO tensors -- channels [0, c1) of the descriptor's Cin from x1 (N x H x W x
 * c1), the rest from x2 (N x H x W x (Cin - c1)) -- so that the concatenated
 * tensor is never written, and its data gradient into two tensors likewise.
 * c1 a multiple of 32 (forward, weight gradient) / of 64 when Cin is one (data
 * gradient: the kernel's block of output channels), else LSI_EINVAL.
 * lsi_conv2d_fwd_cat: bn_workspace != NULL adds the batch-norm sums as
 * lsi_conv2d_fwd_bnstats does (groups is ignored otherwise).
 * lsi_conv2d_wgrad_cat: x2 may be NULL (one tensor, c1 ignored);
 * weight_layout 0 writes g_weight contiguously (Cout x Cin x KH x KW), 2 with
 * torch's channels-last strides (Cout x KH x KW x Cin in memory: the layout of
 * the parameter after module.to(memory_format=torch.channels_last) -- autograd
 * then takes the gradient as it is instead of copying it into that layout).
 */
int lsi_conv2d_fwd_cat(const LsiConvDesc* d, const void* x1, const void* x2, int32_t c1,
                       const void* packed, void* out, float* bn_workspace, int32_t groups,
                       lsi_stream_t stream);
int lsi_conv2d_bwd_data_cat(const LsiConvDesc* d, const void* gy, const void* packed,
                            void* gx1, void* gx2, int32_t c1, lsi_stream_t stream);
int lsi_conv2d_wgrad_cat(const LsiConvDesc* d, const void* x1, const void* x2, int32_t c1,
                         const void* gy, float* g_weight, int32_t weight_layout,
                         void* workspace, size_t workspace_bytes, lsi_stream_t stream);
/*
 * All of the above behind one entry, with a workspace: lsi_conv2d_run(d, mode,
 * io) is lsi_conv2d_fwd (mode 0) / lsi_conv2d_bwd_data (mode 1) with the
 * options of the _bnstats and _cat variants taken from `io` -- and, when
 * `workspace` holds lsi_conv2d_workspace_bytes(d, mode) bytes (16-byte
 * aligned), the contraction SPLIT OVER THE INPUT CHANNELS for the launches
 * whose tiles alone do not fill the chip: the bottleneck maps of the U-Net
 * (reference nets.py:281-305, `cnv5` ... `icnv6`: 2 x 6 ... 16 x 48 pixels with
 * 256 - 1024 channels) are 64 - 256 tiles, each a chain of 16 - 32 dependent
 * stages; ks splits each multiply Cin / ks channels into fp32 partial sums in
 * the workspace, a second kernel adds them in a fixed order, rounds to bf16,
 * stores (into the two tensors of a skip connection's gradient, too) and takes
 * the batch-norm sums.  lsi_conv2d_workspace_bytes returns 0 where the kernel
 * does not split; a smaller or absent workspace is not an error (no split).
 * The caller owns the workspace (no state in the library); calls that share one
 * must be ordered on one stream.  Results are deterministic for a given
 * geometry and differ from the unsplit kernel's only by the fp32 summation
 * order.
 *   x, x2, c1 (mode 0): the input as one (x2 NULL) or two tensors;
 *   out, out2, c1 (mode 1): the gradient into one (out2 NULL) or two tensors;
 *   bn_workspace (NULL: none), groups: as lsi_conv2d_fwd_bnstats.
 */
typedef struct LsiConvIO {
  const void* x;
  const void* x2;
  const void* packed;
  void* out;
  void* out2;
  float* bn_workspace;
  void* workspace;
  size_t workspace_bytes;
  int32_t c1, groups;
} LsiConvIO;
size_t lsi_conv2d_workspace_bytes(const LsiConvDesc* d, int32_t mode);
int lsi_conv2d_run(const LsiConvDesc* d, int32_t mode, const LsiConvIO* io,
                   lsi_stream_t stream);
/*
 * Weight gradient of the convolution LsiConvDesc describes (TF autodiff of
 * slim.conv2d, reference nets.py:29-114, 244-348):
 *   g_weight[co][ci][ky][kx] = sum over n, oy, ox of
 *       gy[n][oy][ox][co] * x[n][oy*stride + ky - pad_t][ox*stride + kx - pad_l][ci]
 *   x: bf16 N x H x W x Cin, gy: bf16 N x OH x OW x Cout (16-byte aligned);
 *   g_weight: fp32 Cout x Cin x KH x KW, written (not added to).  MFMA with K =
 *   output pixels, both operands transposed by the LDS transpose read; partial
 *   sums of the pixel blocks in the workspace, folded by a second kernel
 *   (deterministic).  lsi_conv2d_wgrad_workspace_bytes returns 0 for shapes it
 *   does not take (LSI_EUNSUPPORTED from the call: channel counts that are not
 *   multiples of 32, or small maps with so many channels that the partial sums
 *   would exceed 96 MB -- the bottleneck layers, which stay on the library).
 *   For a transposed convolution described as above (its forward = the data
 *   gradient of the descriptor's convolution), x is the transposed
 *   convolution's OUTPUT gradient and gy its INPUT.
 */
size_t lsi_conv2d_wgrad_workspace_bytes(const LsiConvDesc* d);
int lsi_conv2d_wgrad(const LsiConvDesc* d, const void* x, const void* gy, float* g_weight,
                     void* workspace, size_t workspace_bytes, lsi_stream_t stream);

/*
 * The networks' FIRST convolution (reference nets.py:273 `cnv1`, :53 in
 * encoder_simple: slim.conv2d(inp_img, 32, [7, 7], stride=2), TF `SAME`, batch
 * norm + ReLU behind it) on the matrix cores: d->Cin <= 4 (the image's 3
 * channels), Cout = 32, 7 x 7, stride 2 -- anything else LSI_EUNSUPPORTED
 * (lsi_conv2d_first_supported tells beforehand).  A pixel is padded to four
 * channels in LDS and the K of one MFMA is a whole kernel row (7 taps x 4
 * channels); no packed weights: the kernels read the fp32 parameter itself
 * (weight_layout 0: contiguous Cout x Cin x KH x KW; 2: torch's channels-last
 * strides) and round to bf16 as torch.autocast does.
 *   x: the image, N x H x W x Cin with the channels innermost, fp32 (x_bf16 =
 *   0: rounded to bf16 on the way in) or bf16 (1).  out: bf16 N x OH x OW x 32.
 *   bn_workspace != NULL: the epilogue leaves the batch-norm sums of the rounded
 *   outputs for lsi_bn_relu_norm (as lsi_conv2d_fwd_bnstats; groups | N).
 * lsi_conv2d_first_wgrad: g_weight[co][c][ky][kx] = sum over n, oy, ox of
 *   gy[n][oy][ox][co] * x[n][2 oy + ky - pad_t][2 ox + kx - pad_l][c]  (written,
 *   fp32, in weight_layout; K = output pixels on the matrix cores, partial sums
 *   per workgroup in the workspace folded in a fixed order: deterministic).
 *   gy: bf16 N x OH x OW x 32, 16-byte aligned.  The image has no data gradient.
 */
int lsi_conv2d_first_supported(const LsiConvDesc* d);
int lsi_conv2d_first_fwd(const LsiConvDesc* d, const void* x, int32_t x_bf16,
                         const float* weight, int32_t weight_layout, void* out,
                         float* bn_workspace, int32_t groups, lsi_stream_t stream);
size_t lsi_conv2d_first_wgrad_workspace_bytes(const LsiConvDesc* d);
int lsi_conv2d_first_wgrad(const LsiConvDesc* d, const void* x, int32_t x_bf16, const void* gy,
                           float* g_weight, int32_t weight_layout, void* workspace,
                           size_t workspace_bytes, lsi_stream_t stream);

/*
 * The same convolutions in EXACT fp32 (the reference network's own arithmetic,
 * nets.py:29-114, 244-348: slim.conv2d k x k stride 1 | 2 TF `SAME`,
 * slim.conv2d_transpose 4 x 4 stride 2, fp32 NHWC; TF autodiff for the
 * gradients) on the matrix cores: v_mfma_f32_16x16x4_f32, whose result is a
 * k-ordered chain of fp32 fmas -- no reduced-precision inputs.  Activations,
 * gradients and packed weights are fp32 channels-last, 16-byte aligned
 * (LSI_EUNSUPPORTED otherwise, before any launch).  The descriptor and the
 * roles are those of the bf16 entries above (a transposed convolution is the
 * data gradient of the descriptor's convolution).
 * lsi_conv2d_f32_supported(d): 1 if d is taken -- Cin a multiple of 32, Cout of
 *   16, KH, KW <= 7, stride 1 or 2, pad < kernel size; the data gradient (mode
 *   1) also needs Cout a multiple of 32 (it is the kernel's input there).
 * lsi_conv2d_f32_pack / _pack_job / _pack_many: as lsi_conv2d_pack / _pack_job
 *   / _pack_many (mode 0 | 1, | 2 for a channels-last parameter), writing fp32
 *   [tap][out ch][in ch] into lsi_conv2d_f32_packed_bytes(d) bytes; the jobs of
 *   lsi_conv2d_f32_pack_job go to lsi_conv2d_f32_pack_many only.
 * lsi_conv2d_f32_run(d, mode, io): lsi_conv2d_run in fp32 -- two input tensors
 *   (mode 0), two gradient tensors (mode 1; c1 a multiple of the kernel's block
 *   of output channels: 64 when Cin is a multiple of 64, else 32), the split over
 *   the input channels with a workspace of lsi_conv2d_f32_workspace_bytes(d,
 *   mode) bytes (0: no split), folded in a fixed order; io->bn_workspace must be
 *   NULL (the batch-norm statistics stay with the two-pass kernels).  out is
 *   written, fp32.
 * lsi_conv2d_wgrad_f32: lsi_conv2d_wgrad_cat in fp32 (x1, x2, gy fp32;
 *   g_weight written in weight_layout 0 | 2); K = output pixels on the matrix
 *   cores, partial sums of the pixel blocks in the workspace
 *   (lsi_conv2d_wgrad_f32_workspace_bytes(d): 0 for shapes it does not take --
 *   the bottleneck layers whose partial sums would exceed 96 MB), folded in a
 *   fixed order.  Every result is deterministic for a given geometry.
 */
int lsi_conv2d_f32_supported(const LsiConvDesc* d);
size_t lsi_conv2d_f32_packed_bytes(const LsiConvDesc* d);
int lsi_conv2d_f32_pack(const LsiConvDesc* d, int32_t mode, const float* weight, void* packed,
                        size_t packed_bytes, lsi_stream_t stream);
int lsi_conv2d_f32_pack_job(const LsiConvDesc* d, int32_t mode, const float* weight,
                            void* packed, size_t packed_bytes, LsiPackJob* job,
                            int32_t* nblocks);
int lsi_conv2d_f32_pack_many(const LsiPackJob jobs_device[], int32_t njobs, int32_t total_blocks,
                             lsi_stream_t stream);
size_t lsi_conv2d_f32_workspace_bytes(const LsiConvDesc* d, int32_t mode);
int lsi_conv2d_f32_run(const LsiConvDesc* d, int32_t mode, const LsiConvIO* io,
                       lsi_stream_t stream);
size_t lsi_conv2d_wgrad_f32_workspace_bytes(const LsiConvDesc* d);
int lsi_conv2d_wgrad_f32(const LsiConvDesc* d, const void* x1, const void* x2, int32_t c1,
                         const void* gy, float* g_weight, int32_t weight_layout,
                         void* workspace, size_t workspace_bytes, lsi_stream_t stream);

/* ---- skinny fully-connected layer (+ batch norm + ReLU) --------------------
 * The FC-bottleneck network's `fc` stack (slim.fully_connected + batch norm +
 * ReLU, nets.py:66-67) and `upcnv8`, its 4 x 4 stride-2 transposed convolution
 * on a 1 x 1 map (a fully-connected layer over the four centre taps), on
 * v_mfma_f32_16x16x32_bf16:  Z[M,N] = X[M,K] . W^T  with M <= 32 rows, K and N
 * multiples of 8.
 *
 * W is the fp32 PARAMETER, read in place and rounded to bf16 (nearest even) in
 * registers; nothing is packed, nothing is kept.  Element (n, k) lives at
 *     w[tap_off[n / (N / taps)] + (n % (N / taps)) * w_sn + k * w_sk]
 * (taps = 1, tap_off[0] = 0, w_sn = K, w_sk = 1: nn.Linear; taps = 4 with the
 * offsets of taps (ky, kx) in {1, 2}^2: ConvTranspose2d's (K, N / 4, 4, 4)
 * weight, contiguous or channels-last).  N / taps must be a multiple of 8.
 * X is [M][K] contiguous, bf16, or fp32 (LSI_FC_X_F32) rounded to bf16 on load;
 * products are exact in fp32 and accumulated in fp32; the reduction is split
 * over workgroups and folded in a fixed order (no float atomics): results are
 * bitwise reproducible.
 *
 * LSI_FC_BN: the M rows are `groups` groups of M / groups consecutive rows;
 * every column is normalised with the mean and the biased variance of its
 * group's rows (fp32), + beta[n], ReLU:  y = relu((z - mean) * rsqrt(var + eps)
 * + beta).  One row per group gives variance 0, as TF does.  mean_rstd
 * [groups][2][N] receives mean and 1 / sqrt(var + eps).  Without the flag
 * y = Z (beta, mean_rstd ignored, groups still must divide M).
 * y is [M][N] bf16 -- one rounding -- or fp32 (LSI_FC_OUT_F32).  z (may be
 * NULL) receives the fp32 Z [M][N]; the backward of LSI_FC_BN needs it.
 *
 * lsi_fc_bwd: dy [M][N] in y's type.  With LSI_FC_BN: dbeta[N] (written), the
 * ReLU mask from y, the batch-norm backward per (group, column) from z and
 * mean_rstd.  dZ is rounded once to bf16; then
 *   dw (may be NULL): dW[n][k] = sum_m dZ[m][n] X[m][k], fp32, WRITTEN through
 *     the weight's own strides and tap offsets (elements no (n, k) addresses --
 *     the outer taps -- are not touched);
 *   dx (may be NULL): dX[M][K] = dZ . W in x's type.
 *
 * workspace: lsi_fc_workspace_bytes(d) bytes (forward and backward; 0 for a
 * descriptor lsi_fc_supported(d) refuses; LSI_EWORKSPACE from either entry if
 * smaller, before any launch), 16-byte aligned, the caller's; no
 * state survives a call.  x, dy, workspace 16-byte aligned (LSI_EINVAL).
 * lsi_fc_desc_bytes(): sizeof(LsiFcDesc) as the library was built.
 */
#define LSI_FC_BN 1u
#define LSI_FC_X_F32 2u
#define LSI_FC_OUT_F32 4u
typedef struct LsiFcDesc {
  int32_t M, K, N;
  int32_t groups;
  int32_t taps;
  uint32_t flags;
  int64_t w_sn, w_sk;
  int64_t tap_off[4];
  float eps;
  int32_t reserved;
} LsiFcDesc;
size_t lsi_fc_desc_bytes(void);
int lsi_fc_supported(const LsiFcDesc* d);
size_t lsi_fc_workspace_bytes(const LsiFcDesc* d);
int lsi_fc_fwd(const LsiFcDesc* d, const void* x, const float* w, const float* beta, void* y,
               float* z, float* mean_rstd, void* workspace, size_t workspace_bytes,
               lsi_stream_t stream);
int lsi_fc_bwd(const LsiFcDesc* d, const void* x, const float* w, const void* dy,
               const void* y, const float* z, const float* mean_rstd, void* dx, float* dw,
               float* dbeta, void* workspace, size_t workspace_bytes, lsi_stream_t stream);

/*
 * Exact AREA resize of a ragged batch of decoded uint8 images, one launch
 * (lsi/data/kitti/data.py:area_resize of decode_png(path) * (1/255); reference
 * lsi/data/kitti/data.py:247-266): out[m, i, k, c] is the coverage-weighted
 * mean of image m over [i H/Ho, (i+1) H/Ho) x [k W/Wo, (k+1) W/Wo), divided by
 * 255; H, W are the image's own, the scale may be below or above 1 on either
 * axis.  Integer weights oy ox (in units of 1/Ho, 1/Wo) and a uint32 sum, then
 * one conversion and one fp32 multiply by fl(1 / (255 H W)): independent of
 * the summation order, bitwise reproducible, within 1.5 ulp of the exact
 * rational, exactly 0 where the covered input is 0.
 *   packed    device, uint8, 16-byte aligned, packed_bytes a multiple of 16
 *             (the producer pads); image m is H x W x C interleaved at
 *             packed + offset, rows W C bytes apart (any alignment).  No byte
 *             outside [0, packed_bytes) is read.
 *   desc_dev  the n descriptors on the device (8-byte aligned), read by the
 *             kernel; desc_host the same n descriptors in host memory, checked
 *             here before the launch (the two must agree)
 *   out       device, float32 [n, Ho, Wo, Co], written fully
 * LSI_ENULL for a NULL pointer; LSI_EINVAL for n outside [1, 65535], Co not 1
 * or 3, a descriptor with C != Co, H or W <= 0, H W > LSI_IMAGE_MAX_PIXELS
 * (255 H W must stay below 2^32), (Ho + 1)(H + 1) or (Wo + 1)(W + 1) >= 2^31,
 * an offset that is negative or not a multiple of 16, offset + H W C >
 * packed_bytes, or a misaligned pointer -- all before any launch.  No
 * workspace, no allocation, no synchronisation, no state.
 */
#define LSI_IMAGE_MAX_PIXELS 16843009
typedef struct LsiImageDesc {
  int64_t offset;         /* bytes from `packed`, a multiple of 16           */
  int32_t H, W, C;        /* the image's own size; C == Co                   */
  int32_t reserved;       /* 0                                               */
} LsiImageDesc;
int lsi_area_resize_u8(int32_t n, const LsiImageDesc desc_host[],
                       const LsiImageDesc desc_dev[], const uint8_t* packed,
                       size_t packed_bytes, int32_t Ho, int32_t Wo, int32_t Co,
                       float* out, lsi_stream_t stream);

/*
 * lsi_area_resize_u8 with a per-image crop window, horizontal flip, tone
 * table and channel gains, still one launch: with
 * win = img[y0 : y0 + ch, x0 : x0 + cw] and tone(v, c) = table[c][v] (or v),
 *   acc[i, k, c] = sum_yx oy ox tone(win[y, x, c], c)   (uint32, exact; the
 *                  integer overlaps of lsi_area_resize_u8 with ch, cw for H, W)
 *   val          = min(fl(fl((float)acc * fl(1 / (255 ch cw))) * gain[c]), 1)
 *   out[m, i, flip ? Wo - 1 - k : k, c] = val
 * A full window, no flip, table -1 and gains of 1 give the bits of
 * lsi_area_resize_u8 (wherever those do not exceed 1).
 *   packed    as for lsi_area_resize_u8; image rows stay W C bytes apart.  It
 *             also holds the tone tables: n_tables records of uint8[Co][256]
 *             from byte tables_offset (a multiple of 16), so descriptors,
 *             tables and pixels travel in one upload.  n_tables may be 0.
 *   desc_*    as for lsi_area_resize_u8, of LsiAugmentDesc
 * Refused like lsi_area_resize_u8 (with the int32 bounds on (Ho + 1)(ch + 1),
 * (Wo + 1)(cw + 1)); LSI_EINVAL as well for a window that is empty or leaves
 * the image, flags other than LSI_AUG_FLIP, a table outside [-1, n_tables),
 * n_tables outside [0, 65535], tables that are misaligned or leave the buffer,
 * a gain[c < Co] that is negative, infinite or NaN -- all before any launch.
 */
#define LSI_AUG_FLIP 1u
typedef struct LsiAugmentDesc {
  int64_t offset;         /* bytes from `packed`, a multiple of 16           */
  int32_t H, W, C;        /* the image's own size; C == Co                   */
  uint32_t flags;         /* LSI_AUG_FLIP or 0                               */
  int32_t y0, x0, ch, cw; /* the crop window, in source pixels               */
  int32_t table;          /* index of the image's tone table; -1 = identity  */
  int32_t reserved;       /* 0                                               */
  float gain[3];          /* per channel, finite and >= 0; gain[0] for C = 1 */
  int32_t reserved2;      /* 0                                               */
} LsiAugmentDesc;          /* 64 bytes                                        */
int lsi_augment_resize_u8(int32_t n, const LsiAugmentDesc desc_host[],
                          const LsiAugmentDesc desc_dev[], const uint8_t* packed,
                          size_t packed_bytes, int64_t tables_offset,
                          int32_t n_tables, int32_t Ho, int32_t Wo, int32_t Co,
                          float* out, lsi_stream_t stream);

/*
 * Nearest-neighbour samples of a ragged batch of 16-bit disparity maps (value
 * = disparity * 256, 0 = no match) through the crop window and flip of
 * lsi_augment_resize_u8's descriptors, one launch (DESIGN.md 4.12c;
 * lsi/data/kitti/augment.py:sample_disparity_px): with (y0, x0, ch, cw) the
 * window of map m,
 *   y   = y0 + min(((2 i + 1) ch) / (2 Ho), ch - 1)      (integer division:
 *   x   = x0 + min(((2 k + 1) cw) / (2 Wo), cw - 1)       the pixel under the
 *                                                         output pixel's centre)
 *   val = (float)(((double)map[y, x] / 256) * ((double)Wo / (double)cw))
 *   out[m, i, flip ? Wo - 1 - k : k, 0] = val
 * in pixels of the Ho x Wo image: one fp64 division, one fp64 product (the
 * division by 256 is exact) and one rounding to fp32, so the values are bit
 * for bit the host's.  Zeros stay zeros; a flip does not change the sign.  The
 * full window without flip gives the bits of data.load_disparity_px.
 *   packed    as for lsi_augment_resize_u8; map m is H x W host-order uint16
 *             at packed + offset, rows 2 W bytes apart
 *   desc_*    LsiAugmentDesc with C == 1 and table == -1; gain is not read
 *   out       device, float32 [n, Ho, Wo, 1], written fully
 * LSI_ENULL for a NULL pointer; LSI_EINVAL for n outside [1, 65535], C != 1,
 * H or W <= 0, a window that is empty or leaves the map, flags other than
 * LSI_AUG_FLIP, table != -1, an offset that is negative or not a multiple of
 * 16, offset + 2 H W > packed_bytes, (2 Ho + 1)(ch + 1) or (2 Wo + 1)(cw + 1)
 * >= 2^31, or a misaligned pointer -- all before any launch.  No workspace, no
 * allocation, no synchronisation, no state.
 */
int lsi_augment_sample_u16(int32_t n, const LsiAugmentDesc desc_host[],
                           const LsiAugmentDesc desc_dev[], const uint8_t* packed,
                           size_t packed_bytes, int32_t Ho, int32_t Wo,
                           float* out, lsi_stream_t stream);

/*
 * Contact sheet of visuals, one launch: n_items fp32 device
 * tensors, each with its own size, strides and value range, are quantised to
 * bytes and laid out on a grid of rows x cols cells of cell_h x cell_w pixels
 * with `gutter` >= 0 pixels between the cells and around the border.  The
 * sheet is rows cell_h + (rows + 1) gutter high and cols cell_w + (cols + 1)
 * gutter wide (lsi_visual_sheet_size), RGB interleaved, rows out_row_bytes
 * apart.  Item k sits in cell (k / cols, k % cols), at the cell's top-left;
 * cells without an item, gutters and what an item leaves of its cell take the
 * colour bg.  Every byte of a row below 3 width is written exactly once, no
 * byte beyond it.
 *   item      H x W x C through the element strides (s_y, s_x, s_c), none
 *             negative; sheet pixel (y, x) of the item shows source
 *             (y / zoom, x / zoom), zoom >= 1, H zoom <= cell_h, W zoom <=
 *             cell_w.  No element outside those H x W x C is read.
 *   kinds     RGB (C = 3, each channel quantised on its own), GRAY (C = 1, the
 *             byte in all three channels), LUT (C = 1, the byte indexes lut_dev),
 *             ABSDIFF (C = 1 or 3, a second tensor `ref` of the same size with
 *             the strides r_*: v = |a0 - b0|, or ((|a0 - b0| + |a1 - b1|) +
 *             |a2 - b2|) fl(1/3) added in that order in fp32; then as LUT),
 *             SKIP (no source: the cell stays bg)
 *   value     fp32, no contraction: a NaN (for RGB in any channel) gives the
 *             colour nan; else t = fl(fl(v - lo) inv), inv = fl(1 / fl(hi - lo))
 *             formed by the caller, t = min(max(t, 0), 1) and the byte is
 *             (int)floorf(fl(fl(t 255) + 0.5))
 *   lut_dev   256 x 3 bytes on the device, 4-byte aligned; may be NULL when no
 *             item is LUT or ABSDIFF
 *   items_dev the n_items descriptors on the device (8-byte aligned), read by
 *             the kernel; items_host the same in host memory, checked here
 *             before the launch (the two must agree)
 *   out       device, 4-byte aligned; out_row_bytes >= 3 width, a multiple of 4
 * LSI_ENULL for a NULL sheet, out, descriptor array (n_items > 0), src, ref of
 * an ABSDIFF item or lut_dev when an item needs it; LSI_EINVAL for a grid or
 * cell size < 1, a negative gutter, n_items outside [0, min(rows cols,
 * LSI_VIS_MAX_ITEMS)], an unknown kind, a C the kind does not take, zoom < 1,
 * H or W <= 0, an item larger than its cell, a negative stride, lo or inv not
 * finite or inv <= 0, a misaligned pointer, a bad out_row_bytes or a sheet of
 * more than 2^31 - 1 bytes -- all before any launch.  No workspace, no
 * allocation, no synchronisation, no state.
 */
#define LSI_VIS_SKIP 0
#define LSI_VIS_RGB 1
#define LSI_VIS_GRAY 2
#define LSI_VIS_LUT 3
#define LSI_VIS_ABSDIFF 4
#define LSI_VIS_MAX_ITEMS 256
typedef struct LsiVisSheet {
  int32_t rows, cols, cell_h, cell_w, gutter, n_items;
  uint8_t bg[3], nan[3];  /* background and NaN marker, R G B               */
  uint8_t reserved[2];    /* 0                                               */
} LsiVisSheet;
typedef struct LsiVisItem {
  const float* src;       /* device                                          */
  const float* ref;       /* device; ABSDIFF only, else NULL                 */
  int64_t s_y, s_x, s_c;  /* element strides of src                          */
  int64_t r_y, r_x, r_c;  /* ... and of ref                                  */
  int32_t kind, H, W, C, zoom;
  int32_t reserved;       /* 0                                               */
  float lo, inv;
} LsiVisItem;
int lsi_visual_sheet_size(const LsiVisSheet* sheet, int64_t* height, int64_t* width);
int lsi_visual_pack_u8(const LsiVisSheet* sheet, const LsiVisItem items_host[],
                       const LsiVisItem items_dev[], const uint8_t* lut_dev,
                       uint8_t* out, int64_t out_row_bytes, lsi_stream_t stream);

/*
 * Dense stereo disparities of a rectified pair by semi-global matching on a
 * census cost (csrc/lsi_sgm.hip): all integer, a function of
 * the input bytes alone.
 *   left, right  [B,H,W,C] uint8, C = 1 or 3, contiguous, device
 *   grey         C = 3: (77 R + 150 G + 29 B + 128) >> 8; C = 1: the byte
 *   census       9 wide x 7 high around the pixel without the centre (62 bits),
 *                a bit set where the neighbour's grey is < the centre's,
 *                neighbour coordinates clamped to the image
 *   cost         left view  popcount(cenL[y][x] ^ cenR[y][x - d]), 62 if x - d < 0
 *                right view popcount(cenR[y][x] ^ cenL[y][x + d]), 62 if x + d > W - 1
 *   paths        r in {(0, +-1), (+-1, 0)}, with paths = 8 also (+-1, +-1):
 *                L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + P1,
 *                L_r(p - r, d + 1) + P1, m + P2) - m, m = min_k L_r(p - r, k);
 *                terms with d +- 1 outside [0, D) are absent; L_r = C where p - r
 *                is outside the image.  L_r <= 62 + P2 <= 255; S = sum_r L_r
 *   winner       d0 the first argmin of S, s2 the minimum of S over |d - d0| > 1;
 *                acceptable iff 100 S[d0] <= uniq s2 and d0 > 0
 *   sub-pixel    0 < d0 < D - 1 and den = S[d0-1] - 2 S[d0] + S[d0+1] > 0:
 *                off = (S[d0-1] - S[d0+1]) 128 / den (C division), else 0;
 *                q = 256 d0 + off
 *   left-right   lr_max >= 0: a left pixel stays iff it is acceptable,
 *                x - dL >= 0, the right pixel (y, x - dL) is acceptable and
 *                |dR - dL| <= lr_max on the integer winners; a right pixel alike
 *                at (y, x + dR), x + dR <= W - 1.  lr_max < 0: every acceptable
 *                pixel stays
 *   disp_left, disp_right  [B,H,W] uint16, device: q where the pixel stays,
 *                else 0 (disparity * 256, 0 = no match)
 * D a multiple of 16 in [16, 256]; 0 <= P1 <= P2 <= 193; paths 4 or 8; uniq in
 * [0, 100]; B H W <= 2^27 -- else LSI_EINVAL; then LSI_ENULL for a NULL
 * pointer; then LSI_EWORKSPACE -- all before any launch.  The workspace
 * (16-byte aligned) holds both census planes twice, one 16-bit volume
 * S[2][B][H][W][D] that the path launches add into in place, and the winners:
 * about B H W (4 D + 42) bytes.  4 + paths launches on `stream`, no atomics,
 * no floating point, no host synchronisation, no state.
 */
/* Bytes of device scratch lsi_sgm_disparity_u8 needs; 0 for arguments the call
 * refuses. */
size_t lsi_sgm_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C,
                               int32_t D, int32_t paths);
int lsi_sgm_disparity_u8(int32_t B, int32_t H, int32_t W, int32_t C,
                         const uint8_t* left, const uint8_t* right, int32_t D,
                         int32_t P1, int32_t P2, int32_t paths, int32_t uniq,
                         int32_t lr_max, uint16_t* disp_left,
                         uint16_t* disp_right, void* workspace,
                         size_t workspace_bytes, lsi_stream_t stream);

/*
 * Post-filters for the 16-bit disparity maps above (csrc/lsi_disp_filter.hip;
 * DESIGN.md 4.18): all integer, a function of the input alone.
 *   in, out      [B,H,W] uint16, contiguous, device: disparity * 256, 0 = no
 *                match; out != in
 *   1. median    (median = 3; 0 skips the stage) a pixel that is 0 stays 0 --
 *                no hole filling; a valid pixel becomes the lower median of the
 *                valid values of its 3 x 3 neighbourhood, itself included:
 *                element (n - 1) / 2 of the n sorted values.  Neighbours
 *                outside the image are absent.  Reads the input, writes another
 *                buffer.
 *   2. speckle   (speckle_size > 0; 0 skips the stage) on the output of stage 1.
 *                Two 4-neighbours of one image (left/right, up/down) are linked
 *                iff both are non-zero and |a - b| <= speckle_range, the
 *                difference taken in a wider integer.  Components are the
 *                transitive closure of the links, never across the images of a
 *                batch nor from the end of a row to the start of the next.  A
 *                valid pixel whose component has <= speckle_size pixels becomes
 *                0; every other pixel is unchanged.
 *   Both stages off: out is a copy of in.
 * B, H, W >= 1 and B H W <= 2^27; median 0 or 3; 0 <= speckle_size <= 2^27;
 * 0 <= speckle_range <= 65535 (units of 1/256 px); out != in -- else
 * LSI_EINVAL; then LSI_ENULL for a NULL in or out, or a NULL workspace where
 * one is needed; then LSI_EWORKSPACE -- all before any launch.  Workspace
 * (16-byte aligned), only with speckle_size > 0: a 4-byte parent and a 4-byte
 * size per pixel, plus the 2-byte median plane (rounded up to 16 bytes) when
 * both stages run.  At most 5 launches on `stream`, their number independent
 * of the data; components are labelled by a lock-free union-find (LDS atomics
 * inside 32 x 32 tiles, agent-scope atomics across their edges).  No host
 * synchronisation, no allocation, no state.
 */
/* Bytes of device scratch lsi_disparity_filter_u16 needs; 0 for arguments the
 * call refuses (and where speckle_size = 0: no scratch is needed). */
size_t lsi_disparity_filter_workspace_bytes(int32_t B, int32_t H, int32_t W,
                                            int32_t median, int32_t speckle_size);
int lsi_disparity_filter_u16(int32_t B, int32_t H, int32_t W, const uint16_t* in,
                             uint16_t* out, int32_t median, int32_t speckle_size,
                             int32_t speckle_range, void* workspace,
                             size_t workspace_bytes, lsi_stream_t stream);

/*
 * LiDAR scans rasterised into depth maps (csrc/lsi_lidar.hip):
 * a scatter with a z-buffer, a function of its inputs alone.
 *   desc_host, desc_dev  the same B descriptors in host and in device memory:
 *                scan b is the points [first, first + n) of `pts`.  Padded
 *                batches (first = b Nmax) and packed ones use the same form.
 *   pts          [n_pts_total, 4] float x y z reflectance, device, 16-byte
 *                aligned; may be NULL only when every n is 0
 *   mats         [B, V, 12] float, device: a 3 x 4 row-major matrix per scan
 *                and view
 *   projection   all fp32, in this order, never contracted:
 *                X = ((m0 x + m1 y) + m2 z) + m3, Y and Z from rows 1 and 2;
 *                kept iff Z >= z_min && Z <= z_max (a NaN drops the point);
 *                u = X / Z, v = Y / Z, correctly rounded; kept iff
 *                u >= 0 && u < W && v >= 0 && v < H as floats; the pixel is
 *                (floorf(v), floorf(u))
 *   z-buffer     a pixel's depth is the smallest Z that lands on it (positive
 *                floats order as their bit patterns: an unsigned atomic
 *                minimum, independent of the order of points and threads)
 *   filter       on iff win_y > 0 || win_x > 0.  mn = the minimum of the
 *                unfiltered z-buffer over the non-empty pixels of
 *                [r - win_y, r + win_y] x [c - win_x, c + win_x] clipped to the
 *                image; a non-empty pixel of depth z becomes empty iff
 *                mn * occl_ratio < z (one fp32 multiply, one compare).  Not
 *                iterative, not in place.
 *   out          [B, V, H, W] float, device, written fully: the depth, with
 *                LSI_LIDAR_INVERSE 1.0f / depth (correctly rounded), 0 where
 *                the pixel is empty
 * LSI_EINVAL for B outside [1, 65535], V not 1 or 2, H or W < 1,
 * B V H W > 2^27, win_y or win_x outside [0, 8], n_pts_total outside
 * [0, 2^27], a descriptor with n < 0, first < 0, first + n > n_pts_total or a
 * non-zero reserved, !(0 < z_min <= z_max) or a non-finite bound,
 * !(occl_ratio >= 1) with a window on, unknown flags, a pts that is not
 * 16-byte aligned; then LSI_ENULL; then LSI_EWORKSPACE -- all before any
 * launch.  Workspace: the z-buffer, 4 bytes per pixel of out.  3 launches on
 * `stream` whatever the data (scans without points included: out is zeros);
 * the window minimum is taken per LSI_LIDAR_TILE_H x LSI_LIDAR_TILE_W tile in
 * LDS.  No host synchronisation, no allocation, no state.
 */
#define LSI_LIDAR_INVERSE 1u /* out holds 1 / depth                           */
#define LSI_LIDAR_TILE_H 16
#define LSI_LIDAR_TILE_W 64
typedef struct LsiScanDesc { /* one scan of a batch */
  int64_t first;             /* index of its first point in `pts` (points, not bytes) */
  int32_t n;                 /* number of points, >= 0 */
  int32_t reserved;          /* 0 */
} LsiScanDesc;
/* Bytes of device scratch lsi_lidar_rasterize needs; 0 for arguments the call
 * refuses. */
size_t lsi_lidar_workspace_bytes(int32_t B, int32_t V, int32_t H, int32_t W,
                                 int32_t win_y, int32_t win_x);
int lsi_lidar_rasterize(int32_t B, int32_t V, int32_t H, int32_t W,
                        const LsiScanDesc desc_host[], const LsiScanDesc desc_dev[],
                        const float* pts, int64_t n_pts_total, const float* mats,
                        float z_min, float z_max, int32_t win_y, int32_t win_x,
                        float occl_ratio, uint32_t flags, float* out,
                        void* workspace, size_t workspace_bytes, lsi_stream_t stream);

/*
 * Push-pull (pyramid) hole filling of a rendered image (csrc/lsi_fill.hip;
 * DESIGN.md 4.22).  Forward only.
 *   img          [N, H, W, C] float, device, contiguous, C in 1 .. 4
 *   w            [N, H, W] float, device: what `mode` says
 *   out          [N, H, W, C] float, device, written fully; may not alias img
 *   level 0      LSI_FILL_CONF:  c = (w > 0) ? min(w, 1) : 0 (NaN -> 0),
 *                                p = img c.
 *                LSI_FILL_SPLAT: img, w are forward_splat's normalised image
 *                and weights over a canvas of value bg_value and weight bg_wt:
 *                c = (w > bg_wt) ? (w - bg_wt) / w : 0, the share of the pixel
 *                that came from the layers; p = img - (1 - c) bg_value.
 *                Both: c < conf_min makes c = 0, and where c == 0, p is
 *                selected to be 0 (a NaN or Inf of a hole pixel does not leak).
 *   push         level l + 1 has ceil(H_l / 2) x ceil(W_l / 2) pixels, until
 *                1 x 1 (level Lmax).  For c and each channel of p:
 *                S = (v[2y, 2x] + v[2y, 2x+1]) + (v[2y+1, 2x] + v[2y+1, 2x+1]),
 *                children out of range count as 0; S_c > 1: p' = S_p / S_c,
 *                c' = 1; else p' = S_p, c' = S_c.
 *   pull         coarsest level: F = (c > 0) ? p / c : bg_value.  Below it
 *                F_l = p_l + (1 - c_l) U with U the 2 x bilinear up-sample of
 *                F_{l+1} with clamped borders: cy = y >> 1,
 *                ny = clamp(cy + ((y & 1) ? 1 : -1), 0, H_{l+1} - 1), the same
 *                in x, U = ((9 F[cy,cx] + 3 F[cy,nx]) + (3 F[ny,cx] + F[ny,nx]))
 *                * 0.0625.  out = F_0.
 * All fp32, in this order, never contracted, divisions correctly rounded: the
 * result is a function of the inputs alone, bit for bit.
 * LSI_EINVAL for N outside [1, 65535], H or W < 1, C outside [1, 4],
 * N H W > 2^28, a shape whose levels from 5 up hold more than
 * LSI_FILL_MID_MAX_PIXELS pixels together (they are kept in the LDS of one
 * workgroup; 1024 x 1024 holds 1365), an unknown mode, a non-finite bg_value,
 * a conf_min that is negative or not finite, with LSI_FILL_SPLAT a bg_wt that
 * is negative or not finite; then LSI_ENULL; then LSI_EWORKSPACE -- all before
 * any launch.  Workspace: the pushed levels 1 .. 5 and F of the topmost of
 * them.  3 launches on `stream` (1 for a 1 x 1 image) whatever the data: a
 * workgroup per LSI_FILL_TILE x LSI_FILL_TILE tile pushes 5 levels in LDS, a
 * workgroup per image pushes the rest to 1 x 1 and pulls back, a workgroup per
 * tile pulls with a halo of one pixel per level.  No atomics, no host
 * synchronisation, no allocation, no state.
 */
#define LSI_FILL_CONF 0  /* w is a confidence                                */
#define LSI_FILL_SPLAT 1 /* w is forward_splat's weight sum over a canvas    */
#define LSI_FILL_TILE 32
#define LSI_FILL_MID_MAX_PIXELS 2560
/* Bytes of device scratch lsi_fill_holes needs; 0 for a shape the call
 * refuses. */
size_t lsi_fill_holes_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);
int lsi_fill_holes(int32_t N, int32_t H, int32_t W, int32_t C, const float* img,
                   const float* w, int32_t mode, float bg_wt, float bg_value,
                   float conf_min, float* out, void* workspace, size_t workspace_bytes,
                   lsi_stream_t stream);

/*
 * A layered depth image as a textured triangle mesh: the packed vertex and face
 * records of a binary little-endian PLY file (csrc/lsi_ldi_mesh.hip; DESIGN.md
 * 4.24).  Forward only.  Per batch item b:
 *   tex  [l,b,y,x,c] c in 0..2, disp [l,b,y,x], mask [l,b,y,x] (may be NULL):
 *        float, device, read in place through the descriptor's ELEMENT strides
 *        (RGBD-packed and planar buffers alike)
 *   kinv_dev  B x 9 float, device: the inverse of the source intrinsics
 *   in range  disp finite and disp >= disp_min (a NaN fails)
 *   vertex (l, y, x) exists iff it is in range, mask is NULL or mask > mask_min
 *        (a NaN fails), and it is not merged; it is merged iff merge_ratio > 0,
 *        l > 0, layer l - 1 is in range at (y, x) and
 *        disp_l >= merge_ratio * disp_{l-1}
 *   position  u = x + 0.5, v = y + 0.5, z = 1 / disp,
 *        P_r = ((kinv[3r] u + kinv[3r+1] v) + kinv[3r+2]) z for r = 0, 1, 2;
 *        LSI_MESH_FLIP_YZ negates P_1 and P_2 (y up, looking down -z)
 *   colour    per channel t = min(max(v, 0), 1), (int)floorf(t * 255 + 0.5), a
 *        NaN gives 0 (lsi_visual_pack_u8's rule with lo = 0, inv = 1); alpha 255
 *   vertex record, LSI_MESH_VERTEX_BYTES: float x, y, z; uchar r, g, b, alpha
 *   faces     per layer the quad a = (y, x), b = (y, x+1), c = (y+1, x),
 *        d = (y+1, x+1), y < H - 1, x < W - 1, gives triangle 0 (a, c, b) and
 *        triangle 1 (b, c, d), counter-clockwise seen from the source camera; a
 *        triangle exists iff its three vertices exist and
 *        min(d_i) >= edge_ratio * max(d_i) over their disparities
 *   face record, LSI_MESH_FACE_BYTES: uchar 3; int32 i0, i1, i2
 *   order     vertices are numbered from 0 within an item in order (l, y, x),
 *        faces run in order (l, y, x, triangle) and hold their item's numbers
 *   capacity  item b's records start at b * capacity * record bytes; records
 *        numbered >= the capacity are not written, nor any byte beyond the
 *        item's region; counts[b] = {vertices, faces} are always the true totals
 * All fp32, every operation rounded on its own, divisions correctly rounded: the
 * bytes are a function of the inputs alone.
 * LSI_EINVAL for a NULL descriptor, L, H or W < 1, B outside [1, 65535],
 * L H W > 2^28 (vertex and face numbers and a workgroup's dword index into an
 * item's face bytes, < 2 L H W 13 / 4, then fit the kernels' int32), a negative
 * stride, disp_min that is not positive and finite, a mask_min that is not
 * finite, edge_ratio or merge_ratio outside [0, 1], unknown flag bits, a
 * non-zero reserved word, a capacity outside [0, 2^29], or a misaligned buffer
 * (vertices and workspace 16 bytes, everything else 4); then LSI_ENULL (mask may
 * be NULL; vertices and faces only with a capacity of 0); then LSI_EWORKSPACE
 * -- all before any launch.  Workspace: the index map (int32 per texel, -1
 * where no vertex) and two int32 per LSI_MESH_CHUNK texels.  4 launches on
 * `stream` whatever the data, 3 with a face capacity of 0: count per workgroup
 * of LSI_MESH_CHUNK texels, exclusive scan of the workgroup totals per item in
 * trips of LSI_MESH_SCAN_TRIP (writes counts), vertex records and index map,
 * face records.  No atomics, no host synchronisation, no allocation, no state.
 */
#define LSI_MESH_FLIP_YZ 1u
#define LSI_MESH_VERTEX_BYTES 16
#define LSI_MESH_FACE_BYTES 13
#define LSI_MESH_CHUNK 256
#define LSI_MESH_SCAN_TRIP 256
typedef struct LsiMeshDesc {
  int32_t L, B, H, W;
  int64_t tex_sl, tex_sb, tex_sy, tex_sx, tex_sc;
  int64_t disp_sl, disp_sb, disp_sy, disp_sx;
  int64_t mask_sl, mask_sb, mask_sy, mask_sx;
  float disp_min, mask_min, edge_ratio, merge_ratio;
  uint32_t flags;
  int32_t reserved;       /* 0 */
} LsiMeshDesc;
/* Bytes of device scratch lsi_ldi_mesh needs; 0 for a descriptor the call
 * refuses. */
size_t lsi_ldi_mesh_workspace_bytes(const LsiMeshDesc* desc);
int lsi_ldi_mesh(const LsiMeshDesc* desc, const float* tex, const float* mask,
                 const float* disp, const float* kinv_dev, void* vertices,
                 int64_t vertex_capacity, void* faces, int64_t face_capacity,
                 int32_t* counts, void* workspace, size_t workspace_bytes,
                 lsi_stream_t stream);

/*
 * The surface of lsi_ldi_mesh rasterised into V target views per item with a
 * z-buffer (csrc/lsi_ldi_raster.hip).  Forward only.
 *   tex, disp, mask  as lsi_ldi_mesh reads them, through the ELEMENT strides
 *   M        [B,V,4,4] float, device, contiguous: source pixel (u, v, 1, disp)
 *            to target frame (projection.forward_projection_matrix)
 *   img      [B,V,Ht,Wt,3] float, cov [B,V,Ht,Wt] float (1: a triangle won the
 *            pixel, 0: a hole), out_disp [B,V,Ht,Wt] float or NULL (the
 *            winner's target disparity, 0 at holes): device, written fully
 *   vertex   texel (l, y, x) of item b is a vertex iff lsi_ldi_mesh's rule holds
 *            (in range, mask, not merged).  Under view (b, v), with d its
 *            disparity, px = x + .5, py = y + .5 (the renderer's contract):
 *              q_j = ((px M[j][0] + py M[j][1]) + M[j][2]) + d M[j][3]
 *              n = q_2, u = q_0 / n, v = q_1 / n, dd = q_3 / n
 *            usable iff u, v, dd are finite, n > 0, dd > 0, |u| <= 16384 and
 *            |v| <= 16384 (LSI_RASTER_GUARD); snapped to LSI_RASTER_SUBPIXEL_BITS
 *            bits: X = (int)rintf(u * 256), Y = (int)rintf(v * 256), to nearest
 *            even
 *   triangle the export's (a, c, b) and (b, c, d) of the quad a = (y, x); it
 *            exists iff its vertices exist and are usable and
 *            min(d_i) >= edge_ratio * max(d_i).  No near-plane clipping.
 *            id = ((l H + y) W + x) 2 + t.  In int64
 *              A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0)
 *            A == 0 drops it.  The export's order gives A < 0 where the view
 *            keeps the source's orientation: vertices 1 and 2 are swapped
 *            (then A is -A > 0).  A > 0 before any swap: the view sees the
 *            back of the surface; LSI_RASTER_CULL_BACK drops the triangle,
 *            without the flag it is kept as it is (a two-sided surface).
 *            Pixel (i, j) has its centre at (256 i + 128, 256 j + 128).  The box
 *            i0 = (min X + 127) >> 8 .. i1 = (max X - 128) >> 8 (j likewise), the
 *            centres within the triangle's extent, is clipped to the frame; an
 *            empty box, or a clipped box wider or taller than max_extent
 *            pixels, drops the triangle.
 *   coverage for the edges k = 0, 1, 2 from vertex a to vertex b, (a, b) =
 *            (1, 2), (2, 0), (0, 1), with dx = Xb - Xa, dy = Yb - Ya, in int64
 *              E_k = dx (py - Ya) - dy (px - Xa)
 *            inside iff for every k: E_k > 0, or E_k == 0 and the edge is top-left
 *            (dy < 0, or dy == 0 and dx > 0): a shared edge has one owner.
 *   depth    b1 = (float)E_1 / (float)A, b2 = (float)E_2 / (float)A,
 *            b0 = (1 - b1) - b2, z = (b0 dd_0 + b1 dd_1) + b2 dd_2; a z that is
 *            not finite or not positive is no hit.
 *   z-test   key = bits(z) << 32 | (0xFFFFFFFF - id), combined per pixel by an
 *            unsigned 64-bit atomic maximum: the nearest wins, ties go to the
 *            lowest id, whatever the order of arrival.
 *   resolve  key 0: img = bg_value, cov = 0, out_disp = 0.  Otherwise the
 *            winner's vertices, E_k and b_k are formed again and per channel
 *            c = (b0 c_0 + b1 c_1) + b2 c_2 from tex; cov = 1, out_disp = z.
 * All fp32, every operation rounded on its own, divisions correctly rounded, the
 * int64 -> float conversions to nearest even: the outputs are a function of the
 * inputs alone, bit for bit.
 * LSI_EINVAL for what lsi_ldi_mesh refuses on the shared fields, V outside
 * [1, 1024], B V > 65535, Ht or Wt outside [1, 8192], max_extent outside
 * [1, 256], a bg_value that is not finite, unknown flag bits, a non-zero
 * reserved word or a misaligned buffer (workspace 16 bytes, everything else 4);
 * then LSI_ENULL (mask and out_disp may be NULL); then LSI_EWORKSPACE -- all
 * before any launch.  Workspace: the keys, 8 bytes per target pixel, then 16
 * bytes {X, Y, dd, d} per (b, v, l, y, x) (dd = 0: no usable vertex).  4
 * launches on `stream` whatever the data: clear the keys, project, rasterise
 * (a thread per texel and view: the corner a of its quad), resolve.  No host synchronisation, no
 * allocation, no state, plain vector stores and atomics only.
 */
#define LSI_RASTER_CULL_BACK 1u
#define LSI_RASTER_SUBPIXEL_BITS 8
#define LSI_RASTER_GUARD 16384
#define LSI_RASTER_MAX_VIEWS 1024
#define LSI_RASTER_MAX_SIZE 8192
#define LSI_RASTER_MAX_EXTENT 256
typedef struct LsiRasterDesc {
  int32_t L, B, H, W;
  int64_t tex_sl, tex_sb, tex_sy, tex_sx, tex_sc;
  int64_t disp_sl, disp_sb, disp_sy, disp_sx;
  int64_t mask_sl, mask_sb, mask_sy, mask_sx;
  int32_t V, Ht, Wt;
  int32_t max_extent;
  float disp_min, mask_min, edge_ratio, merge_ratio;
  float bg_value;
  uint32_t flags;
  int32_t reserved;       /* 0 */
} LsiRasterDesc;
/* Bytes of device scratch lsi_ldi_raster needs; 0 for a descriptor the call
 * refuses. */
size_t lsi_ldi_raster_workspace_bytes(const LsiRasterDesc* desc);
int lsi_ldi_raster(const LsiRasterDesc* desc, const float* tex, const float* mask,
                   const float* disp, const float* M, float* img, float* cov,
                   float* out_disp, void* workspace, size_t workspace_bytes,
                   lsi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSI_HIP_H_ */
