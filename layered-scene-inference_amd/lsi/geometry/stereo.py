"""Dense stereo disparities of rectified pairs on the device: semi-global
matching on a census cost (csrc/lsi_sgm.hip).

    disp_left, disp_right = sgm_disparity(left, right, max_disp=128)

left, right: uint8 device tensors [B, H, W, C] (or [H, W, C]), C = 1 or 3.  The
results are uint16 [B, H, W] (or [H, W]): disparity * 256, 0 where the matcher
found no match -- the format of the KITTI ground-truth maps that
lsi.data.kitti.data.load_disparity_px reads.  All integer arithmetic: the result
is a function of the input bytes alone.  Not differentiable -- it produces data,
it is not a loss.  There is no CPU fallback.
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


def sgm_disparity(left, right, max_disp=128, p1=10, p2=120, paths=8, uniqueness=95,
                  lr_max=1):
  """(disp_left_u16, disp_right_u16) of the rectified pair(s); module doc.
  max_disp: the number of disparities, a multiple of 16 in [16, 256];
  0 <= p1 <= p2 <= 193; paths 4 or 8; uniqueness in [0, 100] (percent); lr_max
  the left-right tolerance in pixels, negative to disable the check."""
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
