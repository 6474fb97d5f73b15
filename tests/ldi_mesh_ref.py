"""float32 NumPy restatement of the LDI mesh export (DESIGN.md section 4.24,
the comment of lsi_ldi_mesh in include/lsi_hip.h): the exact vertex and face
records, the counts and the capacity rule.  Every operation is rounded to fp32
on its own, in the stated order; test_ldi_mesh_gpu.py holds the kernels to it
with np.array_equal.

  meshes = mesh(tex, mask, disp, kinv, ...)     # per item (vertices, faces)
  vbytes, fbytes, counts = pack(meshes, vcap, fcap, vbuf, fbuf)
"""
import numpy as np

F = np.float32
VERTEX = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'),
                   ('blue', 'u1'), ('alpha', 'u1')])
FACE = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
assert VERTEX.itemsize == 16 and FACE.itemsize == 13


def in_range(d, disp_min):
  with np.errstate(invalid='ignore'):
    return np.isfinite(d) & (d >= F(disp_min))


def exists(mask, disp, disp_min=1e-3, mask_min=0.5, merge_ratio=0.0):
  """L x H x W bools of one item: which texels are vertices."""
  e = in_range(disp, disp_min)
  with np.errstate(invalid='ignore'):
    if mask is not None:
      e &= mask > F(mask_min)
    if merge_ratio > 0:
      front = disp[:-1]
      with np.errstate(over='ignore'):
        merged = in_range(front, disp_min) & (disp[1:] >= (F(merge_ratio) * front).astype(F))
      e[1:] &= ~merged
  return e


def colour_bytes(tex):
  with np.errstate(invalid='ignore'):
    t = np.minimum(np.maximum(tex, F(0)), F(1))
    t = np.where(np.isnan(tex), F(0), t).astype(F)
  q = np.floor(((t * F(255)).astype(F) + F(0.5)).astype(F))
  return q.astype(np.int32).astype(np.uint8)


def positions(disp, kinv, flip_yz=False):
  """L x H x W x 3 float32 of one item (garbage where disp is out of range)."""
  _, h, w = disp.shape
  k = np.asarray(kinv, F).reshape(9)
  u = (np.arange(w, dtype=F) + F(0.5)).astype(F)[None, None, :]
  v = (np.arange(h, dtype=F) + F(0.5)).astype(F)[None, :, None]
  with np.errstate(all='ignore'):
    z = (F(1) / disp).astype(F)
    p = []
    for r in range(3):
      s = ((k[3 * r] * u).astype(F) + (k[3 * r + 1] * v).astype(F)).astype(F)
      s = (s + k[3 * r + 2]).astype(F)
      p.append((s * z).astype(F))
  if flip_yz:
    p[1], p[2] = -p[1], -p[2]
  return np.stack(p, -1)


def _sq(a):
  a = np.asarray(a, F)
  return a[..., 0] if a.ndim == 5 else a


def mesh(tex, mask, disp, kinv, disp_min=1e-3, mask_min=0.5, edge_ratio=0.0, merge_ratio=0.0,
         flip_yz=False):
  """tex L x B x H x W x 3, mask None or L x B x H x W [x 1], disp likewise,
  kinv B x 9 (or B x 3 x 3): per item (vertices, faces), structured arrays of
  all the records, in order."""
  tex, disp = np.asarray(tex, F), _sq(disp)
  mask = None if mask is None else _sq(mask)
  kinv = np.asarray(kinv, F).reshape(-1, 9)
  nl, nb, h, w = disp.shape
  out = []
  for b in range(nb):
    d = disp[:, b]
    e = exists(None if mask is None else mask[:, b], d, disp_min, mask_min, merge_ratio)
    index = np.full(e.shape, -1, np.int32)
    index[e] = np.arange(int(e.sum()), dtype=np.int32)      # C order: (l, y, x)
    vertices = np.zeros(int(e.sum()), VERTEX)
    p = positions(d, kinv[b], flip_yz)[e]
    vertices['x'], vertices['y'], vertices['z'] = p[:, 0], p[:, 1], p[:, 2]
    c = colour_bytes(tex[:, b])[e]
    vertices['red'], vertices['green'], vertices['blue'] = c[:, 0], c[:, 1], c[:, 2]
    vertices['alpha'] = 255
    # corners of every quad: L x (H - 1) x (W - 1)
    A, B, C, D = ((slice(None), slice(0, h - 1), slice(0, w - 1)),
                  (slice(None), slice(0, h - 1), slice(1, w)),
                  (slice(None), slice(1, h), slice(0, w - 1)),
                  (slice(None), slice(1, h), slice(1, w)))

    def triangle(c0, c1, c2):
      ok = e[c0] & e[c1] & e[c2]
      with np.errstate(invalid='ignore', over='ignore'):
        lo = np.minimum(np.minimum(d[c0], d[c1]), d[c2])
        hi = np.maximum(np.maximum(d[c0], d[c1]), d[c2])
        ok &= lo >= (F(edge_ratio) * hi).astype(F)
      return ok, np.stack([index[c0], index[c1], index[c2]], -1)

    ok0, i0 = triangle(A, C, B)
    ok1, i1 = triangle(B, C, D)
    ok = np.stack([ok0, ok1], -1)                            # (l, y, x, triangle)
    idx = np.stack([i0, i1], -2)[ok]
    faces = np.zeros(len(idx), FACE)
    faces['n'] = 3
    faces['i'] = idx
    out.append((vertices, faces))
  return out


def pack(meshes, vcap, fcap, vbuf=None, fbuf=None):
  """The capacity rule: the records numbered below the capacity written into
  copies of the byte buffers `vbuf` / `fbuf` (what they held before the call;
  None: zeros of B * capacity records), item b at b * capacity * record bytes.
  Returns (vertex bytes, face bytes, counts B x 2 int32: the true totals)."""
  nb = len(meshes)
  vb = np.zeros(nb * vcap * 16, np.uint8) if vbuf is None else np.array(vbuf, np.uint8)
  fb = np.zeros(nb * fcap * 13, np.uint8) if fbuf is None else np.array(fbuf, np.uint8)
  counts = np.zeros((nb, 2), np.int32)
  for b, (v, f) in enumerate(meshes):
    counts[b] = len(v), len(f)
    rv = v[:vcap].tobytes()
    vb[b * vcap * 16:b * vcap * 16 + len(rv)] = np.frombuffer(rv, np.uint8)
    rf = f[:fcap].tobytes()
    fb[b * fcap * 13:b * fcap * 13 + len(rf)] = np.frombuffer(rf, np.uint8)
  return vb, fb, counts
