"""tools/splat_bwd_parity.py: sha256 of what the five splat backward entries write.

Calls lsi_splat_bwd, _bwd_m, _bwd_disp, _bwd_both and _bwd_both_m through the
C ABI on seeded inputs and prints one line `case tensor sha256` per output
tensor.  Two builds whose outputs agree line by line compute the same bits
(LSI_HIP_LIB=<name> selects liblsi_hip_<name>.so): what a change of the
entries' host code has to show.  Both backward routes add in a fixed order, so
a build also has to agree with itself from run to run.

The forward results handed to the backward are seeded random data, not a
forward's output (the kernels only read them, and the forwards do not add in a
fixed order); a few weights are exactly 0 (W' = 1e-8).  L = 3, B = 2, s = 0.5;
24 x 256, 20 x 260 (ragged in the rows per workgroup and the 256-pixel
segments) and 20 x 250 (W % 4 != 0: a STREAM descriptor falls to the gather);
the streamed route (rectified matrices), the gather with the same descriptor
(LSI_BWD_STREAM=0) and the gather with a general pose; composed or per layer,
with and without mask, RGBD pixels, with and without LSI_GRAD_M; both outputs
with and without the composed gradient.  lsi_splat_bwd_disp per layer only:
composed it renders the layers again in no fixed order.  Needs a GPU.
"""
import ctypes
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
from lsi import _C  # noqa: E402
from lsi.geometry import ldi  # noqa: E402

NL, B, S, MD, ZS = 3, 2, 0.5, 0.4, 50.0
DEV = torch.device('cuda', 0)


def rectified(w, g):
  m = torch.eye(4).repeat(B, 1, 1)
  m[:, 0, 0] = 1.0 + 0.05 * (torch.rand(B, generator=g) - 0.5)
  m[:, 0, 2] = 2.0 * (torch.rand(B, generator=g) - 0.5)
  m[:, 0, 3] = -0.3 * w
  m[:, 1, 2] = 0.5 * (torch.rand(B, generator=g) - 0.5)
  return m


def general(h, w, g):
  """K [R t] K^-1 with a small rotation and a 3-D translation."""
  f = 0.58 * w
  k = torch.tensor([[f, 0.0, w / 2, 0.0], [0.0, f, h / 2, 0.0], [0.0, 0.0, 1.0, 0.0],
                    [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
  mats = []
  for _ in range(B):
    a = 0.02 * (torch.rand(3, generator=g, dtype=torch.float64) - 0.5)
    e = torch.eye(4, dtype=torch.float64)
    e[:3, :3] = torch.linalg.matrix_exp(torch.tensor(
        [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64))
    e[:3, 3] = torch.tensor([-0.5, 0.02, 0.03], dtype=torch.float64)
    mats.append(k @ e @ torch.linalg.inv(k))
  return torch.stack(mats).to(torch.float32)


def canvases(nlo, ht, wt, g):
  """Stand-ins for a forward's (img, wts) and their incoming gradients."""
  img = torch.rand((nlo, B, ht, wt, 3), generator=g)
  wts = 0.05 + torch.rand((nlo, B, ht, wt, 1), generator=g)
  wts[torch.rand(wts.shape, generator=g) < 0.02] = 0.0
  return [t.to(DEV) for t in (img, wts, torch.rand(img.shape, generator=g) - 0.3,
                              torch.rand(wts.shape, generator=g) - 0.3)]


def run(case, name, desc, args, outs):
  """lib.<name>(desc, args..., workspace, bytes, stream); prints the hashes of
  `outs` ([(label, tensor)], filled with a constant before the call)."""
  lib = _C.lib()
  size = (lib.lsi_splat_bwd_disp_workspace_bytes if name == 'lsi_splat_bwd_disp'
          else lib.lsi_splat_bwd_workspace_bytes)
  nbytes = int(size(ctypes.byref(desc)))
  ws = torch.zeros((max(nbytes, 16),), dtype=torch.uint8, device=DEV)
  for _, t in outs:
    t.fill_(7.0)
  rc = getattr(lib, name)(ctypes.byref(desc), *[_C.ptr(t) for t in args], _C.ptr(ws),
                          nbytes, _C.stream_ptr(DEV))
  _C.check(rc, name)
  torch.cuda.synchronize()
  for label, t in outs:
    print('%s %s %s' % (case, label, hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()))


def geometry(h, w, route, seed):
  g = torch.Generator().manual_seed(seed)
  ht, wt = int(h * S), int(w * S)
  mat_host = general(h, w, g) if route == 'pose' else rectified(w, g)
  mat = mat_host.to(DEV)
  os.environ['LSI_BWD_STREAM'] = '1' if route == 'stream' else '0'
  rgbd = (MD * torch.rand((NL, B, h, w, 4), generator=g)).to(DEV)
  rgbd[..., :3] /= MD
  for inputs in ('plain', 'mask', 'rgbd'):
    if inputs == 'rgbd':
      tex, disp, mask = rgbd[..., :3], rgbd[..., 3:], None
    else:
      tex, disp = rgbd[..., :3].contiguous(), rgbd[..., 3:].contiguous()
      mask = None
      if inputs == 'mask':
        mask = 0.3 + 0.7 * torch.rand((NL, B, h, w, 1), generator=g)
        mask[torch.rand(mask.shape, generator=g) < 0.1] = 0.0
        mask = mask.to(DEV)
    g_tex = torch.empty((NL, B, h, w, 3), device=DEV)
    g_disp = torch.empty((NL, B, h, w, 1), device=DEV)
    g_mask = torch.empty((NL, B, h, w, 1), device=DEV) if mask is not None else None
    g_m = torch.empty((B, 4, 4), device=DEV)
    layers, composed = canvases(NL, ht, wt, g), canvases(1, ht, wt, g)
    out_disp = MD * torch.rand((NL, B, ht, wt, 1), generator=g).to(DEV)
    g_dsp = (torch.rand((NL, B, ht, wt, 1), generator=g) - 0.3).to(DEV)
    base = [('g_tex', g_tex), ('g_disp', g_disp)] + ([('g_mask', g_mask)] if mask is not None else [])
    for grad_m in (False, True):
      gm = [g_m] if grad_m else [None]
      outs = base + ([('g_M', g_m)] if grad_m else [])

      def desc(flags, later=0):
        d = ldi._desc(tex, mask, disp, ht, wt, S, MD, ZS, 1e-11, flags |
                      (_C.LSI_HAS_MASK if mask is not None else 0), 0)
        ldi.select_path(d, mat_host, 'auto')
        d.flags |= later | (_C.LSI_GRAD_M if grad_m else 0)
        return d

      def case(what):
        return '%dx%d/%s/%s/%s%s' % (h, w, route, inputs, what, '/grad_m' if grad_m else '')

      head = [tex, disp, mask, mat]
      tail = [g_tex, g_disp, g_mask]
      for compose in (True, False):
        if inputs == 'rgbd' and not compose:
          continue   # (RGBD pixels once: the composed call)
        img, wts, g_img, g_wts = composed if compose else layers
        args = head + [img, wts, g_img, g_wts] + tail
        what = 'composed' if compose else 'layers'
        d = desc(_C.LSI_COMPOSE if compose else 0)
        if grad_m:
          run(case(what), 'lsi_splat_bwd_m', d, args + gm, outs)
        else:
          run(case(what), 'lsi_splat_bwd', d, args, outs)
      if inputs == 'rgbd':
        continue
      img, wts, g_img, g_wts = layers
      # (the path chosen as for the call without the disparity output: a per-layer
      # STREAM descriptor, so that the streamed route is taken here too)
      run(case('disp'), 'lsi_splat_bwd_disp', desc(0, _C.LSI_WANT_DISP),
          head + [img, wts, out_disp, g_img, g_wts, g_dsp] + tail + gm, outs)
      img_c, wts_c, g_img_c, g_wts_c = composed
      for what, gc in (('both', [g_img_c, g_wts_c]), ('both_no_gc', [None, None])):
        args = head + [img, wts, img_c, wts_c, g_img, g_wts] + gc + tail
        if grad_m:
          run(case(what), 'lsi_splat_bwd_both_m', desc(0), args + gm, outs)
        else:
          run(case(what), 'lsi_splat_bwd_both', desc(0), args, outs)


if __name__ == '__main__':
  for seed, (h, w) in enumerate(((24, 256), (20, 260), (20, 250))):
    for route in ('stream', 'gather', 'pose'):   # (gather: the streamed call's inputs)
      geometry(h, w, route, seed + (10 if route == 'pose' else 0))
