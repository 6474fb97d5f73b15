"""A predicted LDI's triangle mesh rasterised into novel views on the device
(csrc/lsi_ldi_raster.hip).

    img, cov, disp = rasterize_ldi([tex, mask, disp], src2trg_mat, (ht, wt))
    img, cov, disp = render_views([tex, mask, disp], k_s, k_t, rot, t)

The surface is the one `lsi.geometry.mesh.ldi_mesh` exports: a vertex per valid
texel, two triangles per quad of neighbouring texels, cut where a triangle's
smallest disparity is below `edge_ratio` times its largest, hidden texels that
coincide with the layer in front merged away (`merge_ratio`).  Every view
projects the vertices under the renderer's floating-point contract, snaps them
to 1/256 pixel and rasterises the triangles with integer edge functions and a
top-left rule; the nearest surface wins a pixel through one 64-bit atomic
maximum, which commutes.  So the pictures have no cracks where the camera
magnifies a surface -- what stays uncovered (`cov` = 0, colour `bg_value`) is a
dis-occlusion, a cut, or the border -- and they are a function of the inputs
alone, bit for bit.  A triangle whose clipped box is wider or taller than
`max_extent` pixels is no surface and is dropped.  Forward only; there is no
CPU fallback.
"""
import ctypes

import torch

from lsi import _C
from lsi.geometry import mesh, projection

MAX_SIZE = _C.LSI_RASTER_MAX_SIZE


def _check(ldi, mat, trg_size):
  if not isinstance(ldi, (list, tuple)) or len(ldi) != 3:
    raise TypeError('ldi is [tex, mask or None, disp]')
  tex, mask, disp = ldi
  for name, t in (('tex', tex), ('mask', mask), ('disp', disp), ('src2trg_mat', mat)):
    if t is None and name == 'mask':
      continue
    if not isinstance(t, torch.Tensor):
      raise TypeError('%s must be a tensor' % name)
    if t.dtype != torch.float32:
      raise RuntimeError('rasterize_ldi is fp32 (got %s for %s)' % (t.dtype, name))
  if tex.dim() != 5 or tex.shape[4] != 3:
    raise RuntimeError('tex is L x B x H x W x 3, got %s' % (tuple(tex.shape),))
  for name, t in (('mask', mask), ('disp', disp)):
    if t is not None and tuple(t.shape) not in (tuple(tex.shape[:4]),
                                                tuple(tex.shape[:4]) + (1,)):
      raise RuntimeError('%s is L x B x H x W [x 1] = %s, got %s' %
                         (name, tuple(tex.shape[:4]), tuple(t.shape)))
  if mat.dim() != 4 or mat.shape[0] != tex.shape[1] or tuple(mat.shape[2:]) != (4, 4):
    raise RuntimeError('src2trg_mat is B x V x 4 x 4 with B = %d, got %s' %
                       (tex.shape[1], tuple(mat.shape)))
  if min(tex.shape) < 1 or mat.shape[1] < 1:
    raise RuntimeError('an empty LDI or no view: nothing to rasterise (%s, %s)' %
                       (tuple(tex.shape), tuple(mat.shape)))
  try:
    ht, wt = (int(v) for v in trg_size)
  except (TypeError, ValueError):
    raise TypeError('trg_size is (height, width)')
  if not (1 <= ht <= MAX_SIZE and 1 <= wt <= MAX_SIZE):
    raise RuntimeError('trg_size is (height, width) within 1 .. %d, got %s' %
                       (MAX_SIZE, (ht, wt)))
  for name, t in (('tex', tex), ('mask', mask), ('disp', disp)):
    if t is not None and any(s < 0 for s in t.stride()):
      raise RuntimeError('%s has a negative stride' % name)
  for name, t in (('tex', tex), ('mask', mask), ('disp', disp)):
    if t is not None and not t.is_cuda:
      raise RuntimeError('rasterize_ldi needs %s on a ROCm GPU (got device %s); there is no '
                         'CPU fallback' % (name, t.device))
  return ht, wt


def _check_out(name, t, shape, dev):
  if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or
      tuple(t.shape) != shape or not t.is_contiguous()):
    raise RuntimeError('out: %s must be a contiguous fp32 tensor of shape %s on %s' %
                       (name, shape, dev))


def rasterize_ldi(ldi, src2trg_mat, trg_size, disp_min=1e-3, mask_min=0.5,
                  edge_ratio=mesh.EDGE_RATIO, merge_ratio=0., max_extent=32, bg_value=1.,
                  cull_back=False, out=None, workspace=None):
  """(img B x V x Ht x Wt x 3, cov B x V x Ht x Wt, disp B x V x Ht x Wt) of
  ldi = [tex L x B x H x W x 3, mask or None, disp L x B x H x W [x 1]], read in
  place through their strides, under src2trg_mat B x V x 4 x 4 (any device:
  projection.forward_projection_matrix, rows 0 and 1 scaled to the target size).
  cov is 1 where a triangle won the pixel and 0 at a hole (img = bg_value, disp
  = 0 there).  `cull_back` drops triangles seen from behind; otherwise the
  surface is two-sided.  `out`: (img, cov, disp or None: not written) to write
  into, `workspace`: a uint8 device tensor of lsi_ldi_raster_workspace_bytes,
  both to reuse between calls.  4 launches whatever the data.  With
  src2trg_mat on the LDI's device nothing synchronises and the call can be
  captured in a graph; a host matrix is first copied to the device from
  pageable memory, which blocks the host until the copy is done."""
  ht, wt = _check(ldi, src2trg_mat, trg_size)
  tex, mask, disp = ldi
  dev = _C.require_device(tex, mask, disp)
  nl, nb, h, w = tex.shape[:4]
  nv = src2trg_mat.shape[1]
  d = _C.LsiRasterDesc()
  d.L, d.B, d.H, d.W = nl, nb, h, w
  (d.tex_sl, d.tex_sb, d.tex_sy, d.tex_sx, d.tex_sc) = tex.stride()
  (d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx) = disp.stride()[:4]
  if mask is not None:
    (d.mask_sl, d.mask_sb, d.mask_sy, d.mask_sx) = mask.stride()[:4]
  d.V, d.Ht, d.Wt, d.max_extent = nv, ht, wt, int(max_extent)
  d.disp_min, d.mask_min = disp_min, mask_min
  d.edge_ratio, d.merge_ratio = edge_ratio, merge_ratio
  d.bg_value = bg_value
  d.flags = _C.LSI_RASTER_CULL_BACK if cull_back else 0
  lib = _C.lib()
  with torch.cuda.device(dev):
    mat = src2trg_mat.detach().to(dev).contiguous()
    if out is None:
      img = torch.empty((nb, nv, ht, wt, 3), dtype=torch.float32, device=dev)
      cov = torch.empty((nb, nv, ht, wt), dtype=torch.float32, device=dev)
      od = torch.empty((nb, nv, ht, wt), dtype=torch.float32, device=dev)
    else:
      if not isinstance(out, (list, tuple)) or len(out) != 3:
        raise TypeError('out is (img, cov, disp or None)')
      img, cov, od = out
      _check_out('img', img, (nb, nv, ht, wt, 3), dev)
      _check_out('cov', cov, (nb, nv, ht, wt), dev)
      if od is not None:
        _check_out('disp', od, (nb, nv, ht, wt), dev)
    if workspace is None:
      # (for a descriptor the library refuses the size is 0: it reports it itself)
      need = int(lib.lsi_ldi_raster_workspace_bytes(ctypes.byref(d)))
      workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or
          workspace.device != dev or not workspace.is_contiguous()):
      raise RuntimeError('workspace must be a contiguous uint8 tensor on %s' % (dev,))
    _C.check(lib.lsi_ldi_raster(
        ctypes.byref(d), tex.data_ptr(), _C.ptr(mask), disp.data_ptr(), mat.data_ptr(),
        img.data_ptr(), cov.data_ptr(), _C.ptr(od), workspace.data_ptr(), workspace.numel(),
        _C.stream_ptr(dev)), 'lsi_ldi_raster')
  return img, cov, od


def view_matrices(n_items, k_s, k_t, rot, t, trg_downsampling=1):
  """B x V x 4 x 4 host matrices of B x V cameras (or V cameras for B = 1):
  forward_projection_matrix with rows 0 and 1 multiplied by trg_downsampling."""
  cams = [x.detach().cpu().float() for x in (k_s, k_t, rot, t)]
  if cams[1].dim() == 3:
    if n_items != 1:
      raise RuntimeError('V cameras without a batch dimension need an LDI of one item, got %d'
                         % n_items)
    cams = [x.unsqueeze(0) for x in cams]
  k_s, k_t, rot, t = cams
  if k_t.dim() != 4 or k_t.shape[0] != n_items or tuple(k_t.shape[2:]) != (3, 3):
    raise RuntimeError('k_t is [B x] V x 3 x 3 with B = %d, got %s' %
                       (n_items, tuple(k_t.shape)))
  nv = k_t.shape[1]
  for name, x, tail in (('k_s', k_s, (3, 3)), ('rot', rot, (3, 3)), ('t', t, (3, 1))):
    if tuple(x.shape) != (n_items, nv) + tail:
      raise RuntimeError('%s is [B x] V x %d x %d like k_t, got %s' %
                         (name, tail[0], tail[1], tuple(x.shape)))
  flat = lambda x: x.reshape((n_items * nv,) + tuple(x.shape[2:]))
  m = projection.forward_projection_matrix(flat(k_s), flat(k_t), flat(rot), flat(t))
  m = m.detach().cpu().float().reshape(n_items, nv, 4, 4).clone()
  m[:, :, :2] *= float(trg_downsampling)
  return m


def render_views(ldi, k_s, k_t, rot, t, trg_downsampling=1, trg_size=None, **kwargs):
  """`rasterize_ldi` for B x V cameras (k_s, k_t, rot B x V x 3 x 3, t B x V x 3
  x 1), or V cameras (V x ...) for an LDI of one item: all of them render from
  the one LDI, which is not repeated over the views.  The frames have
  int(H trg_downsampling) x int(W trg_downsampling) pixels unless `trg_size`
  says otherwise; further arguments are rasterize_ldi's.  The matrices are
  built on the host, so every call makes their blocking copy to the device."""
  if not isinstance(ldi, (list, tuple)) or len(ldi) != 3 or not isinstance(ldi[0], torch.Tensor):
    raise TypeError('ldi is [tex, mask or None, disp]')
  tex = ldi[0]
  if tex.dim() != 5:
    raise RuntimeError('tex is L x B x H x W x 3, got %s' % (tuple(tex.shape),))
  if trg_size is None:
    trg_size = (int(tex.shape[2] * trg_downsampling), int(tex.shape[3] * trg_downsampling))
  m = view_matrices(tex.shape[1], k_s, k_t, rot, t, trg_downsampling)
  return rasterize_ldi(ldi, m, trg_size, **kwargs)
