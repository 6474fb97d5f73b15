"""Layer composition and planar transforms (mirror of the reference's
lsi/geometry/layers.py)."""
import ctypes

import torch

from lsi.geometry import homography


def compose(imgs, masks, dmaps, soft=False, min_disp=1e-6,
            depth_softmax_temp=1, differentiable=False):
  """Composes layer images into one image with a white background layer at
  min_disp (reference layers.py:29-70).  imgs: L x [...] x C, masks/dmaps:
  L x [...] x 1.  Returns [...] x C.  One HIP pass (lsi_compose_fwd); CPU
  tensors raise.  With differentiable=True one more pass gives the gradients of
  imgs, masks and dmaps (lsi_compose_bwd; hard composition passes a gradient to
  the selected layer's image only); without it an input that requires a
  gradient raises, as it always did."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.compose(imgs, masks, dmaps, soft, min_disp, depth_softmax_temp,
                      differentiable)


def compose_depth(masks, dmaps, bg_layer=False, min_disp=1e-6,
                  depth_softmax_temp=1, differentiable=False):
  """Composes layer disparities into one map (reference layers.py:73-115):
  lsi_compose_depth_fwd; CPU tensors raise.  With differentiable=True the
  selected layer's disparity takes the gradient (lsi_compose_depth_bwd);
  without it an input that requires a gradient raises, as it always did."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.compose_depth(masks, dmaps, bg_layer, min_disp,
                            depth_softmax_temp, differentiable)


def planar_transform(imgs, masks, pixel_coords_trg, k_s, k_t, rot, t, n_hat, a):
  """Warps L planar layers (images + masks) into the target view and computes
  their target disparity maps (reference layers.py:118-162)."""
  n_layers = imgs.shape[0]

  def rep(x):
    return x.unsqueeze(0).expand((n_layers,) + tuple(x.shape))

  k_s, k_t, t, rot = rep(k_s), rep(k_t), rep(t), rep(rot)
  pixel_coords_trg = rep(pixel_coords_trg)
  imgs_masks = torch.cat([imgs, masks], dim=-1)
  imgs_masks_trg = homography.transform_plane_imgs(
      imgs_masks, pixel_coords_trg, k_s, k_t, rot, t, n_hat, a)
  imgs_trg, masks_trg = imgs_masks_trg[..., :3], imgs_masks_trg[..., 3:4]
  dmaps_trg = homography.trg_disp_maps(pixel_coords_trg, k_t, rot, t, n_hat, a)
  return imgs_trg, masks_trg, dmaps_trg


def plane_homographies(k_w, k_v, rot, t, n_hat, a):
  """(hom, dmat) of render_planes: homography.inv_homography (view pixel ->
  texture pixel, [...] x 3 x 3) and homography.inv_homography_dmat ([...] x 1 x
  3) in ONE batched call each over the broadcast leading dimensions (B x V x P
  for a batch of worlds).  Element-wise 3 x 3 algebra: every matrix has the bits
  the same functions give when they are called plane by plane."""
  lead = torch.broadcast_shapes(k_w.shape[:-2], k_v.shape[:-2], rot.shape[:-2],
                                t.shape[:-2], n_hat.shape[:-2], a.shape[:-2])
  ex = lambda x: x.expand(lead + tuple(x.shape[-2:]))
  k_w, k_v, rot, t, n_hat, a = [ex(x) for x in (k_w, k_v, rot, t, n_hat, a)]
  return (homography.inv_homography(k_w, k_v, rot, t, n_hat, a),
          homography.inv_homography_dmat(k_v, rot, t, n_hat, a))


class _RenderPlanes(torch.autograd.Function):
  """lsi_render_planes (img, disp) / lsi_render_planes_bwd on tex B x P x Hs x
  Ws x 4, hom B x V x P x 9, dmat B x V x P x 3 (contiguous fp32)."""

  @staticmethod
  def forward(ctx, tex, hom, dmat, desc):
    from lsi import _C  # pylint: disable=g-import-not-at-top
    dev = tex.device
    new = lambda c: torch.empty((desc.B, desc.V, desc.H, desc.W, c),
                                dtype=torch.float32, device=dev)
    img, disp = new(3), new(1)
    rc = _C.lib().lsi_render_planes(ctypes.byref(desc), _C.ptr(tex), _C.ptr(hom),
                                    _C.ptr(dmat), _C.ptr(img), _C.ptr(disp), None,
                                    None, _C.stream_ptr(dev))
    _C.check(rc, 'lsi_render_planes')
    ctx.save_for_backward(tex, hom, dmat)
    ctx.desc = desc
    ctx.set_materialize_grads(False)
    return img, disp

  @staticmethod
  def backward(ctx, g_img, g_disp):
    from lsi import _C  # pylint: disable=g-import-not-at-top
    tex, hom, dmat = ctx.saved_tensors
    need = ctx.needs_input_grad
    if (g_img is None and g_disp is None) or not any(need[:3]):
      return None, None, None, None
    dev = tex.device
    f32c = lambda g: None if g is None else g.float().contiguous()
    g_img, g_disp = f32c(g_img), f32c(g_disp)
    # the texture gradient is accumulated (float atomics), the others written
    g_tex = torch.zeros_like(tex) if need[0] else None
    g_hom = torch.empty_like(hom) if need[1] else None
    g_dmat = torch.empty_like(dmat) if need[2] else None
    ws, n = None, 0
    if need[1] or need[2]:
      n = int(_C.lib().lsi_render_planes_bwd_workspace_bytes(ctypes.byref(ctx.desc)))
      ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    rc = _C.lib().lsi_render_planes_bwd(
        ctypes.byref(ctx.desc), _C.ptr(tex), _C.ptr(hom), _C.ptr(dmat),
        _C.ptr(g_img), _C.ptr(g_disp), _C.ptr(g_tex), _C.ptr(g_hom),
        _C.ptr(g_dmat), _C.ptr(ws), n, _C.stream_ptr(dev))
    _C.check(rc, 'lsi_render_planes_bwd')
    return g_tex, g_hom, g_dmat, None


def render_planes(imgs, masks, k_w, k_v, rot, t, n_hat, a, view_hw, soft=False,
                  min_disp=1e-6, depth_softmax_temp=1, n_box=None):
  """B worlds of P textured planes rendered into V views each by ONE HIP launch
  (lsi_render_planes): the fused equivalent of
  `compose(*planar_transform(...), soft, min_disp, depth_softmax_temp)` and
  `compose_depth(masks_trg, dmaps_trg, False, min_disp, depth_softmax_temp)`
  per world and view, bit for bit, without the warped layers in memory.

  imgs: B x P x Hs x Ws x 3 with masks B x P x Hs x Ws x 1, or B x P x Hs x Ws x
  4 (RGBA, as the kernel reads it) with masks None.  k_w (the planes'
  intrinsics), k_v (the views'), rot, t (plane frame -> view), n_hat, a: the
  arguments of planar_transform, with leading dimensions that broadcast to
  B x V x P.  view_hw = (H, W).  Returns (img B x V x H x W x 3, disp B x V x H x
  W x 1); with n_box also (img_room, disp_room): the same with the masks of the
  planes [n_box, P) taken as 0.  CPU tensors raise.

  Without n_box the call is differentiable in imgs, masks (or the RGBA tensor)
  and, through plane_homographies, in k_w, k_v, rot, t, n_hat and a: one more
  launch (lsi_render_planes_bwd) gives the gradients the op route's autograd
  gives.  The room outputs are forward-only: n_box with an input that requires
  a gradient raises."""
  from lsi import _C  # pylint: disable=g-import-not-at-top
  tensors = [x for x in (imgs, masks, k_w, k_v, rot, t, n_hat, a) if x is not None]
  dev = _C.require_device(*tensors)
  wants_grad = torch.is_grad_enabled() and any(x.requires_grad for x in tensors)
  if wants_grad and n_box is not None:
    raise RuntimeError('layers.render_planes: the room outputs (n_box) are '
                       'forward-only; render without n_box for gradients')
  if masks is None:
    if imgs.shape[-1] != 4:
      raise ValueError('render_planes: masks=None needs RGBA textures (got %d '
                       'channels)' % imgs.shape[-1])
    tex = imgs.contiguous()
  else:
    if imgs.shape[-1] != 3 or masks.shape[-1] != 1:
      raise ValueError('render_planes: imgs ... x 3 and masks ... x 1')
    tex = torch.cat([imgs, masks], dim=-1)
  if tex.dim() != 5:
    raise ValueError('render_planes: textures are B x P x Hs x Ws x C')
  nb, npl, hs, ws, _ = tex.shape
  hom, dmat = plane_homographies(k_w, k_v, rot, t, n_hat, a)
  if hom.dim() != 5 or hom.shape[0] != nb or hom.shape[2] != npl:
    raise ValueError('render_planes: cameras / planes must broadcast to B x V x '
                     'P = %d x V x %d (got %s)' % (nb, npl, tuple(hom.shape[:-2])))
  nv = hom.shape[1]
  hom = hom.reshape(nb, nv, npl, 9).contiguous()
  dmat = dmat.reshape(nb, nv, npl, 3).contiguous()
  h, w = int(view_hw[0]), int(view_hw[1])
  d = _C.LsiSceneDesc()
  d.B, d.V, d.P, d.Hs, d.Ws, d.H, d.W = nb, nv, npl, hs, ws, h, w
  d.n_box = npl if n_box is None else int(n_box)
  d.soft = int(bool(soft))
  d.min_disp, d.temp = float(min_disp), float(depth_softmax_temp)
  d.outputs = _C.LSI_SCENE_IMG | _C.LSI_SCENE_DISP
  if n_box is None:
    return _RenderPlanes.apply(tex, hom, dmat, d)
  d.outputs |= _C.LSI_SCENE_IMG_ROOM | _C.LSI_SCENE_DISP_ROOM
  out = [torch.empty((nb, nv, h, w, c), dtype=torch.float32, device=dev)
         for c in (3, 1, 3, 1)]
  rc = _C.lib().lsi_render_planes(
      ctypes.byref(d), _C.ptr(tex), _C.ptr(hom), _C.ptr(dmat),
      *([_C.ptr(o) for o in out] + [_C.stream_ptr(dev)]))
  _C.check(rc, 'lsi_render_planes')
  return tuple(out)
