"""A predicted LDI as a textured triangle mesh, packed on the device as the
records of a binary PLY file (csrc/lsi_ldi_mesh.hip).

    m = ldi_mesh([tex, mask, disp], k_s, edge_ratio=0.9)      # no synchronisation
    for vertices, faces in m.to_host():                       # the one sync
      write_ply('item.ply', vertices, faces)

Every texel whose disparity is finite and at least `disp_min` (and whose mask
exceeds `mask_min`) is a vertex at K^-1 (x + 0.5, y + 0.5, 1) / disp with its
colour as bytes; neighbouring texels of a layer are joined by two triangles per
quad, counter-clockwise seen from the source camera, unless the smallest of a
triangle's disparities is below `edge_ratio` times its largest (a depth
discontinuity: the surface is cut there).  With `merge_ratio` > 0 a hidden-layer
texel whose disparity is at least merge_ratio times that of the layer in front
coincides with the surface in front of it and is dropped.  Vertices are numbered
in order (l, y, x), faces in order (l, y, x, triangle): the bytes are a function
of the inputs alone.  The default `edge_ratio` is a starting value for viewing,
not a tuned one -- there is no KITTI data in this repository to tune it on.
There is no CPU fallback; `ldi_mesh_ops` states the same in torch ops on any
device (the second check and the context of the measurements).
"""
import ctypes

import numpy as np
import torch

from lsi import _C
from lsi.geometry import projection

VERTEX_BYTES = _C.LSI_MESH_VERTEX_BYTES
FACE_BYTES = _C.LSI_MESH_FACE_BYTES
VERTEX = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'),
                   ('blue', 'u1'), ('alpha', 'u1')])
FACE = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
EDGE_RATIO = 0.9      # a starting value, not tuned (module doc)
assert VERTEX.itemsize == VERTEX_BYTES and FACE.itemsize == FACE_BYTES


def full_capacity(nl, h, w):
  """(vertices, faces) per item that no LDI of this shape exceeds."""
  return nl * h * w, 2 * nl * (h - 1) * (w - 1)


def _check(ldi, k_s):
  if not isinstance(ldi, (list, tuple)) or len(ldi) != 3:
    raise TypeError('ldi is [tex, mask or None, disp]')
  tex, mask, disp = ldi
  for name, t in (('tex', tex), ('mask', mask), ('disp', disp), ('k_s', k_s)):
    if t is None and name == 'mask':
      continue
    if not isinstance(t, torch.Tensor):
      raise TypeError('%s must be a tensor' % name)
    if t.dtype != torch.float32:
      raise RuntimeError('ldi_mesh is fp32 (got %s for %s)' % (t.dtype, name))
  if tex.dim() != 5 or tex.shape[4] != 3:
    raise RuntimeError('tex is L x B x H x W x 3, got %s' % (tuple(tex.shape),))
  for name, t in (('mask', mask), ('disp', disp)):
    if t is not None and tuple(t.shape) not in (tuple(tex.shape[:4]),
                                                tuple(tex.shape[:4]) + (1,)):
      raise RuntimeError('%s is L x B x H x W [x 1] = %s, got %s' %
                         (name, tuple(tex.shape[:4]), tuple(t.shape)))
  if tuple(k_s.shape) != (tex.shape[1], 3, 3):
    raise RuntimeError('k_s is B x 3 x 3 = %s, got %s' %
                       ((tex.shape[1], 3, 3), tuple(k_s.shape)))
  if min(tex.shape) < 1:
    raise RuntimeError('an empty LDI has no mesh: %s' % (tuple(tex.shape),))
  for name, t in (('tex', tex), ('mask', mask), ('disp', disp)):
    if t is not None and any(s < 0 for s in t.stride()):
      raise RuntimeError('%s has a negative stride' % name)
  for name, t in (('tex', tex), ('mask', mask), ('disp', disp)):
    if t is not None and not t.is_cuda:
      raise RuntimeError('ldi_mesh needs %s on a ROCm GPU (got device %s); there is no '
                         'CPU fallback' % (name, t.device))


class LdiMesh(object):
  """What `ldi_mesh` returns: `vertices` and `faces`, uint8 device buffers of B x
  capacity records (item b's at b * capacity * record bytes), `counts`, B x 2
  int32 on the device: the true {vertices, faces} of every item, and the two
  capacities.  Nothing here has been waited for."""

  def __init__(self, vertices, faces, counts, vertex_capacity, face_capacity):
    self.vertices, self.faces, self.counts = vertices, faces, counts
    self.vertex_capacity, self.face_capacity = vertex_capacity, face_capacity

  def to_host(self):
    """Per item (vertices, faces): NumPy structured arrays (`VERTEX`, `FACE`).
    Reads `counts` (the one synchronisation), then copies the used prefixes
    only.  Raises if an item has more records than its capacity."""
    counts = self.counts.cpu().numpy()
    out = []
    for b, (nv, nf) in enumerate(counts):
      nv, nf = int(nv), int(nf)
      if nv > self.vertex_capacity or nf > self.face_capacity:
        raise RuntimeError('item %d has %d vertices and %d faces, the capacities are %d and '
                           '%d: the mesh is truncated' %
                           (b, nv, nf, self.vertex_capacity, self.face_capacity))
      v0, f0 = b * self.vertex_capacity * VERTEX_BYTES, b * self.face_capacity * FACE_BYTES
      v = self.vertices[v0:v0 + nv * VERTEX_BYTES].cpu().numpy()
      f = (self.faces[f0:f0 + nf * FACE_BYTES].cpu().numpy() if nf else
           np.zeros(0, np.uint8))
      out.append((v.view(VERTEX), f.view(FACE)))
    return out


def ldi_mesh(ldi, k_s, disp_min=1e-3, mask_min=0.5, edge_ratio=EDGE_RATIO, merge_ratio=0.0,
             flip_yz=False, capacity=None, out=None, workspace=None):
  """The mesh of ldi = [tex L x B x H x W x 3, mask or None, disp L x B x H x W
  [x 1]] under the source intrinsics k_s B x 3 x 3 (any device): an `LdiMesh`.
  The tensors are read in place through their strides -- views of the network's
  packed RGBD buffer, planar (permuted) tensors.  `capacity`: (vertices, faces)
  per item, None: `full_capacity`.  `out`: (vertex buffer, face buffer, counts)
  to write into, `workspace`: a uint8 device tensor of
  lsi_ldi_mesh_workspace_bytes, both to reuse between calls.  4 launches
  whatever the data (3 with a face capacity of 0), no synchronisation."""
  _check(ldi, k_s)
  tex, mask, disp = ldi
  dev = _C.require_device(tex, mask, disp)
  nl, nb, h, w = tex.shape[:4]
  vcap, fcap = full_capacity(nl, h, w) if capacity is None else (int(capacity[0]),
                                                                 int(capacity[1]))
  d = _C.LsiMeshDesc()
  d.L, d.B, d.H, d.W = nl, nb, h, w
  (d.tex_sl, d.tex_sb, d.tex_sy, d.tex_sx, d.tex_sc) = tex.stride()
  (d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx) = disp.stride()[:4]
  if mask is not None:
    (d.mask_sl, d.mask_sb, d.mask_sy, d.mask_sx) = mask.stride()[:4]
  d.disp_min, d.mask_min = disp_min, mask_min
  d.edge_ratio, d.merge_ratio = edge_ratio, merge_ratio
  d.flags = _C.LSI_MESH_FLIP_YZ if flip_yz else 0
  lib = _C.lib()
  with torch.cuda.device(dev):
    kinv = projection._inv3(k_s.detach()).reshape(nb, 9).to(dev).contiguous()
    if out is None:
      vbuf = torch.empty(max(nb * vcap * VERTEX_BYTES, 16), dtype=torch.uint8, device=dev)
      fbuf = (torch.empty(nb * fcap * FACE_BYTES, dtype=torch.uint8, device=dev)
              if fcap > 0 else None)
      counts = torch.empty((nb, 2), dtype=torch.int32, device=dev)
    else:
      vbuf, fbuf, counts = out
      for name, t, need in (('vertex buffer', vbuf, nb * vcap * VERTEX_BYTES),
                            ('face buffer', fbuf, nb * fcap * FACE_BYTES)):
        if t is None and need == 0:
          continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != dev or
            not t.is_contiguous() or t.numel() < need):
          raise RuntimeError('the %s must be a contiguous uint8 tensor of at least %d bytes '
                             'on %s' % (name, need, dev))
      if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or
          counts.device != dev or tuple(counts.shape) != (nb, 2) or
          not counts.is_contiguous()):
        raise RuntimeError('counts must be a contiguous B x 2 int32 tensor on %s' % (dev,))
    if workspace is None:
      # (for a descriptor the library refuses the size is 0: it reports it itself)
      need = int(lib.lsi_ldi_mesh_workspace_bytes(ctypes.byref(d)))
      workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _C.check(lib.lsi_ldi_mesh(
        ctypes.byref(d), tex.data_ptr(), _C.ptr(mask), disp.data_ptr(), kinv.data_ptr(),
        vbuf.data_ptr() if vcap > 0 else None, vcap, fbuf.data_ptr() if fcap > 0 else None,
        fcap, counts.data_ptr(), workspace.data_ptr(), workspace.numel(),
        _C.stream_ptr(dev)), 'lsi_ldi_mesh')
  if fbuf is None:
    fbuf = torch.empty(0, dtype=torch.uint8, device=dev)
  return LdiMesh(vbuf, fbuf, counts, vcap, fcap)


# --- PLY files ----------------------------------------------------------------------------
_HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\n'
           'property float x\nproperty float y\nproperty float z\n'
           'property uchar red\nproperty uchar green\nproperty uchar blue\n'
           'property uchar alpha\nelement face %d\n'
           'property list uchar int vertex_indices\nend_header\n')


def write_ply(path, vertices, faces):
  """A binary little-endian PLY file of `VERTEX` and `FACE` records (structured
  arrays, or their bytes as uint8 arrays)."""
  v = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
  f = np.ascontiguousarray(faces).view(np.uint8).reshape(-1)
  if v.size % VERTEX_BYTES or f.size % FACE_BYTES:
    raise ValueError('vertices are %d-byte records, faces %d-byte records' %
                     (VERTEX_BYTES, FACE_BYTES))
  with open(path, 'wb') as out:
    out.write((_HEADER % (v.size // VERTEX_BYTES, f.size // FACE_BYTES)).encode('ascii'))
    out.write(v.tobytes())
    out.write(f.tobytes())


def read_ply(path):
  """(vertices, faces) of a file `write_ply` wrote: structured arrays."""
  with open(path, 'rb') as f:
    data = f.read()
  end = data.find(b'end_header\n')
  if not data.startswith(b'ply\n') or end < 0:
    raise ValueError('%s is no PLY file' % path)
  header = data[:end].decode('ascii').split('\n')
  body = data[end + len(b'end_header\n'):]
  if header[1] != 'format binary_little_endian 1.0':
    raise ValueError('%s: only binary_little_endian 1.0 is read' % path)
  counts = {w[1]: int(w[2]) for w in (line.split() for line in header) if w and
            w[0] == 'element'}
  want = _HEADER % (counts.get('vertex', -1), counts.get('face', -1))
  if data[:len(data) - len(body)] != want.encode('ascii'):
    raise ValueError('%s: not the vertex and face layout write_ply writes' % path)
  nv, nf = counts['vertex'], counts['face']
  if len(body) != nv * VERTEX_BYTES + nf * FACE_BYTES:
    raise ValueError('%s: %d bytes of records, the header announces %d' %
                     (path, len(body), nv * VERTEX_BYTES + nf * FACE_BYTES))
  v = np.frombuffer(body, np.uint8, nv * VERTEX_BYTES).copy().view(VERTEX)
  f = np.frombuffer(body, np.uint8, nf * FACE_BYTES, nv * VERTEX_BYTES).copy().view(FACE)
  return v, f


# --- the op route -------------------------------------------------------------------------
def _in_range(d, disp_min):
  return torch.isfinite(d) & (d >= disp_min)


def ldi_mesh_ops(ldi, k_s, disp_min=1e-3, mask_min=0.5, edge_ratio=EDGE_RATIO,
                 merge_ratio=0.0, flip_yz=False):
  """`ldi_mesh` in torch ops on the tensors' device, in the definition's order
  of operations: per item (positions Nv x 3 float32, colours Nv x 4 uint8, faces
  Nf x 3 int32), of exactly the items' sizes (boolean indexing synchronises)."""
  tex, mask, disp = ldi
  tex = tex.float()
  sq = lambda t: t.float()[..., 0] if t.dim() == 5 else t.float()
  disp = sq(disp)
  mask = None if mask is None else sq(mask)
  nl, nb, h, w = disp.shape
  dev = disp.device
  kinv = projection._inv3(k_s.detach().float()).reshape(nb, 9).to(dev)
  f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
  u = (torch.arange(w, dtype=torch.float32, device=dev) + 0.5)[None, None, :]
  v = (torch.arange(h, dtype=torch.float32, device=dev) + 0.5)[None, :, None]
  out = []
  for b in range(nb):
    d = disp[:, b]
    e = _in_range(d, f32(disp_min))
    if mask is not None:
      e = e & (mask[:, b] > f32(mask_min))
    if merge_ratio > 0 and nl > 1:
      merged = _in_range(d[:-1], f32(disp_min)) & (d[1:] >= f32(merge_ratio) * d[:-1])
      e = torch.cat([e[:1], e[1:] & ~merged], 0)
    index = (torch.cumsum(e.reshape(-1).to(torch.int32), 0, dtype=torch.int32) - 1).reshape(
        e.shape)
    z = 1.0 / d
    k = kinv[b]
    p = [((k[3 * r] * u + k[3 * r + 1] * v) + k[3 * r + 2]) * z for r in range(3)]
    if flip_yz:
      p[1], p[2] = -p[1], -p[2]
    pos = torch.stack(p, -1)[e]
    t = tex[:, b]
    q = torch.floor(torch.clamp(t, 0.0, 1.0) * 255.0 + 0.5)
    q = torch.where(torch.isnan(t), torch.zeros_like(q), q).to(torch.uint8)
    col = torch.cat([q, torch.full_like(q[..., :1], 255)], -1)[e]
    A = (slice(None), slice(0, h - 1), slice(0, w - 1))
    B = (slice(None), slice(0, h - 1), slice(1, w))
    C = (slice(None), slice(1, h), slice(0, w - 1))
    D = (slice(None), slice(1, h), slice(1, w))

    def triangle(c0, c1, c2):
      lo = torch.minimum(torch.minimum(d[c0], d[c1]), d[c2])
      hi = torch.maximum(torch.maximum(d[c0], d[c1]), d[c2])
      ok = e[c0] & e[c1] & e[c2] & (lo >= f32(edge_ratio) * hi)
      return ok, torch.stack([index[c0], index[c1], index[c2]], -1)

    ok0, i0 = triangle(A, C, B)
    ok1, i1 = triangle(B, C, D)
    faces = torch.stack([i0, i1], -2)[torch.stack([ok0, ok1], -1)]
    out.append((pos, col, faces))
  return out
