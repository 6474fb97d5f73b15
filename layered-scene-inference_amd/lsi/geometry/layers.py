"""Layer composition and planar transforms (mirror of the reference's
lsi/geometry/layers.py)."""
import torch

from lsi.geometry import homography


def compose(imgs, masks, dmaps, soft=False, min_disp=1e-6,
            depth_softmax_temp=1):
  """Composes layer images into one image with a white background layer at
  min_disp (reference layers.py:29-70).  imgs: L x [...] x C, masks/dmaps:
  L x [...] x 1.  Returns [...] x C.  One HIP pass (lsi_compose_fwd, forward
  only: data generation and evaluation); CPU tensors raise."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.compose(imgs, masks, dmaps, soft, min_disp, depth_softmax_temp)


def compose_depth(masks, dmaps, bg_layer=False, min_disp=1e-6,
                  depth_softmax_temp=1):
  """Composes layer disparities into one map (reference layers.py:73-115):
  lsi_compose_depth_fwd (forward only); CPU tensors raise."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.compose_depth(masks, dmaps, bg_layer, min_disp,
                            depth_softmax_temp)


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
  planes [n_box, P) taken as 0.  Forward only; CPU tensors raise."""
  from lsi import _C  # pylint: disable=g-import-not-at-top
  import ctypes  # pylint: disable=g-import-not-at-top
  tensors = [x for x in (imgs, masks, k_w, k_v, rot, t, n_hat, a) if x is not None]
  dev = _C.require_device(*tensors)
  if any(x.requires_grad for x in tensors):
    raise RuntimeError('layers.render_planes on the GPU is forward-only')
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
  new = lambda c: torch.empty((nb, nv, h, w, c), dtype=torch.float32, device=dev)
  out = [new(3), new(1)]
  if n_box is not None:
    d.outputs |= _C.LSI_SCENE_IMG_ROOM | _C.LSI_SCENE_DISP_ROOM
    out += [new(3), new(1)]
  rc = _C.lib().lsi_render_planes(
      ctypes.byref(d), _C.ptr(tex), _C.ptr(hom), _C.ptr(dmat),
      *([_C.ptr(o) for o in out] + [None] * (4 - len(out)) + [_C.stream_ptr(dev)]))
  _C.check(rc, 'lsi_render_planes')
  return tuple(out)
