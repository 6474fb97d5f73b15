"""The LDI mesh export's definition (tests/ldi_mesh_ref.py, the float32
restatement the kernels are held to in test_ldi_mesh_gpu.py) on cases with
known answers, the PLY reader and writer, the op route on the host, and what
`ldi_mesh` and the library refuse before they look for a device.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import ldi_mesh_ref as R

F = np.float32
K = np.array([[120.0, 0, 31.5], [0, 110.0, 17.25], [0, 0, 1]], F)


def kinv_of(k):
  from lsi.geometry import projection
  return projection._inv3(torch.from_numpy(np.asarray(k, F))).numpy().reshape(-1, 9)


def plane(nl, nb, h, w, value=0.25, seed=0):
  rs = np.random.RandomState(seed)
  return rs.rand(nl, nb, h, w, 3).astype(F), np.full((nl, nb, h, w), value, F)


# --- counts with known answers ----------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 2, 2), (2, 2, 5, 3), (1, 1, 33, 65)])
def test_fronto_parallel_plane(shape):
  nl, nb, h, w = shape
  tex, disp = plane(*shape)
  for v, f in R.mesh(tex, None, disp, kinv_of([K] * nb), edge_ratio=0.9):
    assert len(v) == nl * h * w and len(f) == 2 * nl * (h - 1) * (w - 1)
    assert (v['alpha'] == 255).all() and (f['n'] == 3).all()
    assert np.array_equal(v['z'], np.full(len(v), 4.0, F))


def test_vertical_step_is_cut():
  h, w = 6, 9
  tex, disp = plane(1, 1, h, w, 0.5)
  disp[..., 4:] = 0.25                    # ratio 0.5 between columns 3 and 4
  (v, f), = R.mesh(tex, None, disp, kinv_of([K]), edge_ratio=0.9)
  assert len(v) == h * w and len(f) == 2 * (h - 1) * (w - 2)
  (v, f), = R.mesh(tex, None, disp, kinv_of([K]), edge_ratio=0.0)
  assert len(f) == 2 * (h - 1) * (w - 1)
  # at the ratio exactly the triangle stays: min >= edge_ratio * max
  (v, f), = R.mesh(tex, None, disp, kinv_of([K]), edge_ratio=0.5)
  assert len(f) == 2 * (h - 1) * (w - 1)


def test_a_spike_takes_one_triangle_of_a_quad():
  tex, disp = plane(1, 1, 3, 3, 0.25)
  disp[0, 0, 0, 0] = 1.0                  # corner a of the first quad only
  (v, f), = R.mesh(tex, None, disp, kinv_of([K]), edge_ratio=0.9)
  assert len(v) == 9 and len(f) == 7
  assert np.array_equal(f['i'][0], [1, 3, 4])      # triangle 1 (b, c, d) of quad (0, 0)


def test_merge_ratio_drops_a_coinciding_layer():
  tex, disp = plane(2, 1, 5, 7, 0.25)
  (v, f), = R.mesh(tex, None, disp, kinv_of([K]), merge_ratio=0.98)
  assert len(v) == 35 and len(f) == 2 * 4 * 6
  (v2, f2), = R.mesh(tex, None, disp, kinv_of([K]), merge_ratio=0.0)
  assert len(v2) == 70 and len(f2) == 4 * 4 * 6
  # behind an out-of-range front layer nothing is merged
  disp[0] = np.nan
  (v3, _), = R.mesh(tex, None, disp, kinv_of([K]), merge_ratio=0.98)
  assert len(v3) == 35


def test_validity_rules():
  tex, disp = plane(1, 1, 1, 8, 0.25)
  disp[0, 0, 0] = [np.nan, np.inf, -np.inf, 0.0, -1.0, np.nextafter(F(1e-3), F(0)), 1e-3, 0.25]
  (v, _), = R.mesh(tex, None, disp, kinv_of([K]), disp_min=1e-3)
  assert len(v) == 2
  mask = np.array([0.5, np.nan, 1.0, 0.0, 1.0, 1.0, np.nextafter(F(0.5), F(1)), 0.5], F)
  disp[:] = 0.25
  (v, _), = R.mesh(tex, mask.reshape(1, 1, 1, 8), disp, kinv_of([K]), mask_min=0.5)
  assert len(v) == 4


def test_colour_bytes():
  t = np.array([-1.0, 0.0, 1.0, 2.0, np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255,
                0.4 / 255, 127.4999 / 255], F)
  got = R.colour_bytes(t)
  want = [0, 0, 255, 255, 0, 255, 0, None, None, 0, 127]
  for g, w_, x in zip(got, want, t):
    if w_ is not None:
      assert g == w_, x
  assert got[7] in (0, 1) and got[8] in (1, 2)


# --- structure -------------------------------------------------------------------------
def random_ldi(seed, nl, nb, h, w, holes=0.2):
  rs = np.random.RandomState(seed)
  tex = rs.rand(nl, nb, h, w, 3).astype(F)
  disp = (0.01 + 0.99 * rs.rand(nl, nb, h, w)).astype(F)
  disp[rs.rand(nl, nb, h, w) < holes] = 0
  return tex, disp


@pytest.mark.parametrize('flip', [False, True])
def test_faces_are_local_and_counter_clockwise(flip):
  nl, nb, h, w = 3, 2, 9, 11
  tex, disp = random_ldi(1, nl, nb, h, w)
  meshes = R.mesh(tex, None, disp, kinv_of([K] * nb), edge_ratio=0.3, flip_yz=flip)
  seen = 0
  for b, (v, f) in enumerate(meshes):
    e = R.exists(None, disp[:, b])
    where = np.argwhere(e)                        # vertex number -> (l, y, x)
    assert len(where) == len(v)
    idx = f['i']
    assert idx.min() >= 0 and idx.max() < len(v)
    lyx = where[idx]                              # Nf x 3 x 3
    assert (lyx[:, :, 0] == lyx[:, :1, 0]).all()  # one layer
    assert (np.ptp(lyx[:, :, 1], axis=1) == 1).all() and (np.ptp(lyx[:, :, 2], axis=1) == 1).all()
    # counter-clockwise seen from the camera: in the image (x right, y down)
    # that is a negative shoelace area; project the vertices to get there
    p = np.stack([v['x'], v['y'], v['z']], -1).astype(np.float64)
    if flip:
      p = p * [1, -1, -1]
    px = (K.astype(np.float64) @ p.T).T
    px = px[:, :2] / px[:, 2:]
    t = px[idx]
    area = ((t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) -
            (t[:, 2, 0] - t[:, 0, 0]) * (t[:, 1, 1] - t[:, 0, 1]))
    assert (area < 0).all()
    # seen from the camera at the origin the same holds in space: the normal of
    # (i0, i1, i2) points back at the camera
    q = np.stack([v['x'], v['y'], v['z']], -1).astype(np.float64)[idx]
    normal = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    assert ((normal * q[:, 0]).sum(-1) < 0).all()
    seen += len(f)
  assert seen > 100


def test_reprojection_returns_the_pixel_centre():
  h, w = 64, 96
  rs = np.random.RandomState(2)
  k = np.array([[0.58 * w, 0, w / 2], [0, 0.6 * w, h / 2], [0, 0, 1]], F)
  tex = rs.rand(1, 1, h, w, 3).astype(F)
  disp = (0.01 + 0.99 * rs.rand(1, 1, h, w)).astype(F)
  (v, _), = R.mesh(tex, None, disp, kinv_of([k]))
  p = np.stack([v['x'], v['y'], v['z']], -1).astype(np.float64)
  px = (k.astype(np.float64) @ p.T).T
  px = px[:, :2] / px[:, 2:]
  yy, xx = np.mgrid[0:h, 0:w]
  want = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], -1)
  assert np.abs(px - want).max() <= 1e-3


def test_scalar_restatement():
  """The vectorised restatement against the definition written texel by texel."""
  nl, nb, h, w = 2, 2, 5, 6
  rs = np.random.RandomState(3)
  tex, disp = random_ldi(3, nl, nb, h, w, holes=0.15)
  disp[1] = np.where(rs.rand(nb, h, w) < 0.5, disp[0], disp[1])
  mask = rs.rand(nl, nb, h, w).astype(F)
  kinv = kinv_of([K] * nb)
  par = dict(disp_min=0.05, mask_min=0.1, edge_ratio=0.4, merge_ratio=0.9)
  got = R.mesh(tex, mask, disp, kinv, flip_yz=True, **par)
  for b in range(nb):
    def rng(d):
      return bool(np.isfinite(d) and d >= F(par['disp_min']))

    def ex(l, y, x):
      d = disp[l, b, y, x]
      if not rng(d) or not mask[l, b, y, x] > F(par['mask_min']):
        return False
      if l > 0 and rng(disp[l - 1, b, y, x]) and d >= F(par['merge_ratio']) * disp[l - 1, b, y, x]:
        return False
      return True

    number, verts = {}, []
    for l in range(nl):
      for y in range(h):
        for x in range(w):
          if ex(l, y, x):
            number[(l, y, x)] = len(verts)
            u, v, z = F(x + 0.5), F(y + 0.5), F(1) / disp[l, b, y, x]
            k = kinv[b]
            p = [F(F(F(F(k[3 * r] * u) + F(k[3 * r + 1] * v)) + k[3 * r + 2]) * z)
                 for r in range(3)]
            c = [int(np.floor(F(F(min(max(t, F(0)), F(1)) * F(255)) + F(0.5))))
                 for t in tex[l, b, y, x]]
            verts.append((p[0], -p[1], -p[2], c[0], c[1], c[2], 255))
    faces = []
    for l in range(nl):
      for y in range(h - 1):
        for x in range(w - 1):
          a, bb, c, d = (l, y, x), (l, y, x + 1), (l, y + 1, x), (l, y + 1, x + 1)
          for tri in ((a, c, bb), (bb, c, d)):
            if all(t in number for t in tri):
              ds = [disp[t[0], b, t[1], t[2]] for t in tri]
              if min(ds) >= F(par['edge_ratio']) * max(ds):
                faces.append((3, [number[t] for t in tri]))
    assert got[b][0].tobytes() == np.array(verts, R.VERTEX).tobytes()
    assert got[b][1].tobytes() == np.array(faces, R.FACE).tobytes()
    assert len(faces) > 0


def test_capacity_rule():
  tex, disp = plane(1, 2, 3, 4)
  meshes = R.mesh(tex, None, disp, kinv_of([K] * 2))
  vb, fb, counts = R.pack(meshes, 12, 12)
  assert counts.tolist() == [[12, 12], [12, 12]]
  assert vb.tobytes() == meshes[0][0].tobytes() + meshes[1][0].tobytes()
  pre_v, pre_f = np.full(2 * 5 * 16 + 7, 0xA5, np.uint8), np.full(2 * 4 * 13 + 7, 0xA5, np.uint8)
  vb, fb, counts = R.pack(meshes, 5, 4, pre_v, pre_f)
  assert counts.tolist() == [[12, 12], [12, 12]]           # the true totals
  assert vb[:80].tobytes() == meshes[0][0][:5].tobytes()
  assert vb[80:160].tobytes() == meshes[1][0][:5].tobytes() and (vb[160:] == 0xA5).all()
  assert fb[52:104].tobytes() == meshes[1][1][:4].tobytes() and (fb[104:] == 0xA5).all()


# --- PLY files ---------------------------------------------------------------------------
def test_ply_round_trip(tmp_path, built_lib):
  from lsi.geometry import mesh
  assert mesh.VERTEX == R.VERTEX and mesh.FACE == R.FACE
  tex, disp = random_ldi(4, 2, 1, 7, 5)
  (v, f), = R.mesh(tex, None, disp, kinv_of([K]), edge_ratio=0.2)
  path = str(tmp_path / 'a.ply')
  mesh.write_ply(path, v, f)
  data = open(path, 'rb').read()
  head, body = data.split(b'end_header\n', 1)
  assert head.decode('ascii').split('\n')[:-1] == [
      'ply', 'format binary_little_endian 1.0', 'element vertex %d' % len(v),
      'property float x', 'property float y', 'property float z', 'property uchar red',
      'property uchar green', 'property uchar blue', 'property uchar alpha',
      'element face %d' % len(f), 'property list uchar int vertex_indices']
  assert body == v.tobytes() + f.tobytes()
  v2, f2 = mesh.read_ply(path)
  assert v2.dtype == R.VERTEX and f2.dtype == R.FACE
  assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
  # the bytes as uint8 arrays are accepted too
  mesh.write_ply(path, np.frombuffer(v.tobytes(), np.uint8), np.frombuffer(f.tobytes(), np.uint8))
  assert open(path, 'rb').read() == data
  # a header-only file
  empty = str(tmp_path / 'empty.ply')
  mesh.write_ply(empty, v[:0], f[:0])
  v0, f0 = mesh.read_ply(empty)
  assert len(v0) == 0 and len(f0) == 0 and v0.dtype == R.VERTEX and f0.dtype == R.FACE
  assert open(empty, 'rb').read().endswith(b'end_header\n')
  # what is no such file is refused
  bad = str(tmp_path / 'bad.ply')
  open(bad, 'wb').write(data[:-1])
  with pytest.raises(ValueError):
    mesh.read_ply(bad)
  open(bad, 'wb').write(b'not a ply file')
  with pytest.raises(ValueError):
    mesh.read_ply(bad)
  with pytest.raises(ValueError):
    mesh.write_ply(bad, np.zeros(15, np.uint8), f)


# --- the op route on the host -------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 1, 1, 7), (2, 2, 5, 3), (3, 1, 33, 65)])
def test_ops_statement_agrees_with_the_restatement(built_lib, shape):
  from lsi.geometry import mesh
  nl, nb, h, w = shape
  rs = np.random.RandomState(5)
  tex, disp = random_ldi(5, nl, nb, h, w)
  tex = (tex * 1.4 - 0.2).astype(F)
  tex[rs.rand(*tex.shape) < 0.05] = np.nan
  disp[rs.rand(*disp.shape) < 0.05] = np.nan
  if nl > 1:
    disp[1] = np.where(rs.rand(nb, h, w) < 0.5, disp[0], disp[1])
  mask = rs.rand(nl, nb, h, w).astype(F)
  k = np.stack([K] * nb)
  par = dict(disp_min=0.05, mask_min=0.1, edge_ratio=0.4, merge_ratio=0.9, flip_yz=True)
  want = R.mesh(tex, mask, disp, kinv_of(k), **par)
  got = mesh.ldi_mesh_ops([torch.from_numpy(tex), torch.from_numpy(mask),
                           torch.from_numpy(disp)[..., None]], torch.from_numpy(k), **par)
  for (v, f), (pos, col, faces) in zip(want, got):
    assert pos.dtype == torch.float32 and col.dtype == torch.uint8 and faces.dtype == torch.int32
    assert np.array_equal(faces.numpy().reshape(-1, 3), f['i'])
    p = np.stack([v['x'], v['y'], v['z']], -1)
    assert np.array_equal(pos.numpy().view(np.uint32), p.view(np.uint32))
    c = np.stack([v['red'], v['green'], v['blue'], v['alpha']], -1)
    assert np.array_equal(col.numpy(), c)


# --- refusals that need no device ---------------------------------------------------------
def test_ldi_mesh_refuses_before_it_looks_for_a_device(built_lib):
  from lsi.geometry import mesh
  tex, disp, k = torch.rand(2, 1, 8, 8, 3), torch.rand(2, 1, 8, 8, 1), torch.eye(3)[None]
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    mesh.ldi_mesh([tex, None, disp], k)
  with pytest.raises(RuntimeError, match='fp32'):
    mesh.ldi_mesh([tex.double(), None, disp], k)
  with pytest.raises(RuntimeError, match='fp32'):
    mesh.ldi_mesh([tex, None, disp], k.double())
  with pytest.raises(RuntimeError, match='L x B x H x W x 3'):
    mesh.ldi_mesh([torch.rand(2, 1, 8, 8, 4), None, disp], k)
  with pytest.raises(RuntimeError, match='L x B x H x W x 3'):
    mesh.ldi_mesh([tex[0], None, disp], k)
  with pytest.raises(RuntimeError, match='disp is'):
    mesh.ldi_mesh([tex, None, torch.rand(2, 1, 8, 7, 1)], k)
  with pytest.raises(RuntimeError, match='mask is'):
    mesh.ldi_mesh([tex, torch.rand(1, 1, 8, 8), disp], k)
  with pytest.raises(RuntimeError, match='k_s is'):
    mesh.ldi_mesh([tex, None, disp], torch.eye(3))
  with pytest.raises(RuntimeError, match='empty'):
    mesh.ldi_mesh([tex[:, :, :0], None, disp[:, :, :0]], k)
  with pytest.raises(TypeError):
    mesh.ldi_mesh([tex.numpy(), None, disp], k)
  with pytest.raises(TypeError):
    mesh.ldi_mesh([tex, disp], k)


def mesh_desc(_C, L=2, B=2, H=8, W=8, **kw):
  d = _C.LsiMeshDesc()
  d.L, d.B, d.H, d.W = L, B, H, W
  d.tex_sc, d.tex_sx, d.tex_sy, d.tex_sb, d.tex_sl = 1, 3, 3 * W, 3 * W * H, 3 * W * H * B
  d.disp_sx, d.disp_sy, d.disp_sb, d.disp_sl = 1, W, W * H, W * H * B
  d.mask_sx, d.mask_sy, d.mask_sb, d.mask_sl = 1, W, W * H, W * H * B
  d.disp_min, d.mask_min, d.edge_ratio, d.merge_ratio = 1e-3, 0.5, 0.9, 0.0
  for key, value in kw.items():
    setattr(d, key, value)
  return d


# what the library refuses with LSI_EINVAL: descriptor fields ...
BAD_DESCRIPTORS = [
    dict(L=0), dict(B=0), dict(B=65536), dict(H=0), dict(W=-1),
    dict(L=1, H=16384, W=16385),                     # L H W > 2^28
    dict(L=65536, H=65536, W=65536),
    dict(tex_sl=-1), dict(tex_sc=-1), dict(disp_sy=-8), dict(mask_sx=-1),
    dict(disp_min=0.0), dict(disp_min=-1.0), dict(disp_min=float('nan')),
    dict(disp_min=float('inf')), dict(mask_min=float('nan')), dict(mask_min=float('inf')),
    dict(edge_ratio=-0.1), dict(edge_ratio=1.5), dict(edge_ratio=float('nan')),
    dict(merge_ratio=-0.1), dict(merge_ratio=1.01), dict(merge_ratio=float('nan')),
    dict(flags=2), dict(flags=0x80000001), dict(reserved=1),
]
# ... and arguments: (name -> value) over a call that is otherwise taken
BAD_ARGUMENTS = [
    dict(vcap=-1), dict(fcap=-1), dict(vcap=(1 << 29) + 1), dict(fcap=(1 << 29) + 1),
    dict(tex=66), dict(mask=65), dict(disp=62), dict(kinv=63), dict(vertices=72),
    dict(faces=66), dict(counts=66), dict(workspace=72),
]


def test_library_refuses_before_any_launch(built_lib):
  """Host answers of the two entry points, in the header's order EINVAL ->
  ENULL -> EWORKSPACE: no pointer is touched."""
  from lsi import _C
  lib = _C.lib()
  size = lib.lsi_ldi_mesh_workspace_bytes
  names = ('tex', 'mask', 'disp', 'kinv', 'vertices', 'faces', 'counts', 'workspace')

  def call(d, vcap=128, fcap=196, nbytes=1 << 40, **ptrs):
    p = dict({n: 64 for n in names}, **ptrs)
    return lib.lsi_ldi_mesh(ctypes.byref(d), p['tex'], p['mask'], p['disp'], p['kinv'],
                            p['vertices'], vcap, p['faces'], fcap, p['counts'],
                            p['workspace'], nbytes, None)

  assert lib.lsi_ldi_mesh(None, 64, 64, 64, 64, 64, 1, 64, 1, 64, 64, 1 << 40, None) == -1
  assert size(None) == 0
  for kw in BAD_DESCRIPTORS:
    d = mesh_desc(_C, **kw)
    assert size(ctypes.byref(d)) == 0 and call(d) == -1, kw
    assert call(d, tex=None) == -1, kw               # EINVAL comes before ENULL
  good = mesh_desc(_C)
  for kw in BAD_ARGUMENTS:
    assert call(good, **kw) == -1, kw
    assert call(good, **dict(kw, disp=kw.get('disp') or None)) == -1, kw
  # what is taken: the limits themselves, and every required pointer on its own
  for kw in (dict(), dict(L=1, B=1, H=1, W=1), dict(L=1, B=65535, H=16384, W=16384),
             dict(edge_ratio=0.0, merge_ratio=1.0, flags=1), dict(edge_ratio=1.0)):
    d = mesh_desc(_C, **kw)
    need = size(ctypes.byref(d))
    n = d.L * d.H * d.W
    assert need == (d.B * n * 4 + 15) // 16 * 16 + d.B * ((n + 255) // 256) * 8, kw
    for miss in ('tex', 'disp', 'kinv', 'vertices', 'faces', 'counts', 'workspace'):
      assert call(d, **{miss: None}) == -2, (kw, miss)
    assert call(d, tex=None, nbytes=0) == -2, kw     # ENULL comes before EWORKSPACE
    assert call(d, nbytes=need - 1) == -3, kw
    assert call(d, mask=None, nbytes=need - 1) == -3, kw     # the mask may be NULL
    # a capacity of 0 needs no buffer
    assert call(d, vcap=0, fcap=0, vertices=None, faces=None, nbytes=need - 1) == -3, kw
    assert call(d, vcap=1 << 29, fcap=1 << 29, nbytes=need - 1) == -3, kw
