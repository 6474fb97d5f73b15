"""Dense stereo disparities of rectified pairs on the device: semi-global
matching on a census cost (csrc/lsi_sgm.hip).

    disp_left, disp_right = sgm_disparity(left, right, max_disp=128)

left, right: uint8 device tensors [B, H, W, C] (or [H, W, C]), C = 1 or 3.  The
results are uint16 [B, H, W] (or [H, W]): disparity * 256, 0 where the matcher
found no match -- the format of the KITTI ground-truth maps that
lsi.data.kitti.data.load_disparity_px reads.  All integer arithmetic: the result
is a function of the input bytes alone.  Not differentiable -- it produces data,
it is not a loss.  There is no CPU fallback.

    clean = filter_disparity(disp_u16, median=3, speckle_size=20)

post-filters such maps (csrc/lsi_disp_filter.hip): a
3 x 3 median over the valid values, then the removal of 4-connected components
of at most speckle_size pixels whose neighbours differ by at most speckle_range
(units of 1/256 px).  sgm_disparity takes the same three arguments and filters
both views in one call; all of them are off by default.
"""
import torch

from lsi import _C

# A call's workspace is dominated by the 16-bit cost volume, 4 D bytes per pixel
# of a pair; a batch whose workspace would exceed this many bytes is matched in
# slices (a single pair is never split, whatever it needs).
WORKSPACE_CAP = 1 << 30


def workspace_bytes(b, h, w, c, max_disp, paths):
  return int(_C.lib().lsi_sgm_workspace_bytes(b, h, w, c, max_disp, paths))


def _check(left, right):
  for name, t in (('left', left), ('right', right)):
    if not isinstance(t, torch.Tensor):
      raise TypeError('%s must be a tensor' % name)
    if not t.is_cuda:
      raise RuntimeError(
          'sgm_disparity needs tensors on a ROCm GPU (got device %s); there is no '
          'CPU fallback' % t.device)
    if t.dtype != torch.uint8:
      raise RuntimeError('sgm_disparity takes uint8 images (got %s)' % t.dtype)
  if left.shape != right.shape or left.device != right.device:
    raise RuntimeError('left %s on %s and right %s on %s differ' % (
        tuple(left.shape), left.device, tuple(right.shape), right.device))
  if left.dim() not in (3, 4):
    raise RuntimeError('images are [B, H, W, C] or [H, W, C], got %s' %
                       (tuple(left.shape),))


def filter_workspace_bytes(b, h, w, median, speckle_size):
  return int(_C.lib().lsi_disparity_filter_workspace_bytes(b, h, w, median, speckle_size))


def filter_disparity(disp_u16, median=0, speckle_size=0, speckle_range=256):
  """The filtered copy of uint16 maps [B, H, W] (or [H, W]); module doc.
  median 0 (off) or 3: the lower median of the valid 3 x 3 neighbours, holes
  stay holes; then, with speckle_size > 0, every 4-connected component of at
  most speckle_size pixels becomes 0, neighbours being linked when both are
  valid and differ by at most speckle_range (0 .. 65535, 1/256 px).  With both
  off the result is a copy."""
  if not isinstance(disp_u16, torch.Tensor):
    raise TypeError('disp_u16 must be a tensor')
  if not disp_u16.is_cuda:
    raise RuntimeError(
        'filter_disparity needs a tensor on a ROCm GPU (got device %s); there is no '
        'CPU fallback' % disp_u16.device)
  if disp_u16.dtype != torch.uint16:
    raise RuntimeError('filter_disparity takes the uint16 maps (got %s)' % disp_u16.dtype)
  if disp_u16.dim() not in (2, 3):
    raise RuntimeError('maps are [B, H, W] or [H, W], got %s' % (tuple(disp_u16.shape),))
  single = disp_u16.dim() == 2
  src = (disp_u16[None] if single else disp_u16).contiguous()
  b, h, w = src.shape
  median, speckle_size, speckle_range = int(median), int(speckle_size), int(speckle_range)
  out = torch.empty_like(src)
  with torch.cuda.device(src.device):
    # (for arguments the library refuses the size is 0: it reports them itself)
    need = filter_workspace_bytes(b, h, w, median, speckle_size)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=src.device)
    _C.check(_C.lib().lsi_disparity_filter_u16(
        b, h, w, src.data_ptr(), out.data_ptr(), median, speckle_size, speckle_range,
        ws.data_ptr(), ws.numel(), _C.stream_ptr(src.device)), 'lsi_disparity_filter_u16')
  return out[0] if single else out


def sgm_disparity(left, right, max_disp=128, p1=10, p2=120, paths=8, uniqueness=95,
                  lr_max=1, median=0, speckle_size=0, speckle_range=256):
  """(disp_left_u16, disp_right_u16) of the rectified pair(s); module doc.
  max_disp: the number of disparities, a multiple of 16 in [16, 256];
  0 <= p1 <= p2 <= 193; paths 4 or 8; uniqueness in [0, 100] (percent); lr_max
  the left-right tolerance in pixels, negative to disable the check.  median,
  speckle_size, speckle_range: filter_disparity's, applied to both views in one
  call; with the defaults nothing is filtered and nothing more is launched."""
  _check(left, right)
  single = left.dim() == 3
  if single:
    left, right = left[None], right[None]
  left, right = left.contiguous(), right.contiguous()
  b, h, w, c = left.shape
  lib = _C.lib()
  args = [int(v) for v in (max_disp, p1, p2, paths, uniqueness, lr_max)]
  per_pair = workspace_bytes(1, h, w, c, args[0], args[3])
  chunk = b if per_pair == 0 else max(1, min(b, WORKSPACE_CAP // per_pair))
  filtered = int(median) != 0 or int(speckle_size) != 0
  if filtered:   # both views in one buffer: one filter call on a batch of 2 B
    both = torch.empty((2, b, h, w), dtype=torch.uint16, device=left.device)
    out_l, out_r = both[0], both[1]
  else:
    out_l = torch.empty((b, h, w), dtype=torch.uint16, device=left.device)
    out_r = torch.empty((b, h, w), dtype=torch.uint16, device=left.device)
  with torch.cuda.device(left.device):
    # (for arguments the library refuses the size is 0: it reports them itself)
    need = workspace_bytes(chunk, h, w, c, args[0], args[3])
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=left.device)
    stream = _C.stream_ptr(left.device)
    for b0 in range(0, max(b, 1), chunk):
      n = min(chunk, b - b0)
      _C.check(lib.lsi_sgm_disparity_u8(
          n, h, w, c, left[b0:b0 + n].data_ptr(), right[b0:b0 + n].data_ptr(),
          args[0], args[1], args[2], args[3], args[4], args[5],
          out_l[b0:b0 + n].data_ptr(), out_r[b0:b0 + n].data_ptr(),
          ws.data_ptr(), ws.numel(), stream), 'lsi_sgm_disparity_u8')
  if filtered:
    both = filter_disparity(both.view(2 * b, h, w), median, speckle_size,
                            speckle_range).view(2, b, h, w)
    out_l, out_r = both[0], both[1]
  if single:
    return out_l[0], out_r[0]
  return out_l, out_r


def disparity_px(u16):
  """The 16-bit maps as float32 disparities in pixels (value / 256; 0 = no
  match)."""
  if u16.dtype != torch.uint16:
    raise RuntimeError('disparity_px takes the uint16 maps (got %s)' % u16.dtype)
  # (through int32: not every elementwise op takes uint16)
  wide = u16.view(torch.int16).to(torch.int32) & 0xFFFF
  return wide.to(torch.float32) / 256.0
