"""The LDI mesh rasteriser's definition (tests/ldi_raster_ref.py, the float32 /
int64 restatement the kernels are held to in test_ldi_raster_gpu.py) on cases
with known answers, the shared cases' preconditions, and what `rasterize_ldi`,
`render_views` and the library refuse before they look for a device.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import ldi_mesh_ref
import ldi_raster_cases as C
import ldi_raster_ref as R

F = np.float32
EYE = np.eye(4, dtype=F)[None, None]


def valid_ldi(nl, h, w, seed=0):
  rs = np.random.RandomState(seed)
  tex = rs.rand(nl, 1, h, w, 3).astype(F)
  disp = (0.2 + 0.5 * rs.rand(nl, 1, h, w)).astype(F)
  if nl > 1:
    disp[1:] = (disp[1:] * F(0.25)).astype(F)      # behind layer 0
  return tex, disp


# --- the three properties of the definition ---------------------------------------------
def test_identity_returns_the_texels_bit_for_bit():
  h, w = 9, 13
  tex, disp = valid_ldi(2, h, w)
  r = R.raster(tex, None, disp, EYE, h, w)
  cov = r['cov'][0, 0]
  # the surface spans texel centres; the fill rule gives away the right and bottom rims
  assert (cov[:-1, :-1] == 1).all() and (cov[-1] == 0).all() and (cov[:, -1] == 0).all()
  assert (r['img'][0, 0, -1] == 1).all() and (r['disp'][0, 0, -1] == 0).all()
  # layer 0 wins with weights exactly 1, 0, 0: triangle 0 of the quad of that texel
  ys, xs = np.mgrid[0:h - 1, 0:w - 1]
  assert np.array_equal(r['winner'][0, 0, :-1, :-1], (ys * w + xs) * 2)
  assert np.array_equal(r['img'][0, 0, :-1, :-1].view(np.uint32),
                        tex[0, 0, :-1, :-1].view(np.uint32))
  assert np.array_equal(r['disp'][0, 0, :-1, :-1].view(np.uint32),
                        disp[0, 0, :-1, :-1].view(np.uint32))
  # both layers cover every such pixel once
  assert (r['count'][0, 0, :-1, :-1] == 2).all() and r['count'][0, 0, -1].sum() == 0


def _affine_cover(m, h, w, ht, wt, eps=0.01):
  """Which pixel centres lie inside (1), outside (0) or within eps texels of the
  rim (-1) of the affine image of the texel-centre rectangle."""
  a = np.array([[m[0, 0], m[0, 1]], [m[1, 0], m[1, 1]]], np.float64)
  o = np.array([m[0, 2], m[1, 2]], np.float64)
  js, is_ = np.mgrid[0:ht, 0:wt]
  p = np.stack([is_ + 0.5, js + 0.5], -1) - o
  s = p @ np.linalg.inv(a).T
  def side(v, lo, hi):
    inside = (v > lo + eps) & (v < hi - eps)
    outside = (v < lo - eps) | (v > hi + eps)
    return inside, outside
  ix, ox = side(s[..., 0], 0.5, w - 0.5)
  iy, oy = side(s[..., 1], 0.5, h - 0.5)
  out = np.full((ht, wt), -1)
  out[ix & iy] = 1
  out[ox | oy] = 0
  return out


@pytest.mark.parametrize('view', ['magnifying', 'mirrored', 'mirrored-magnifying'])
def test_every_interior_pixel_is_covered_exactly_once(view):
  h, w, ht, wt = 9, 13, 30, 40
  m = C.magnifying_matrix()
  if view == 'mirrored':
    m = np.array([[-1, 0, w + 0.25, 0], [0, 1, 0.125, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F)
  elif view == 'mirrored-magnifying':
    m = (np.array([[-1, 0, 36, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F) @ m).astype(F)
  tex, disp = valid_ldi(1, h, w, seed=1)
  r = R.raster(tex, None, disp, m[None, None], ht, wt)
  want = _affine_cover(m, h, w, ht, wt)
  count = r['count'][0, 0]
  assert count.max() == 1                       # a shared edge has one owner
  assert (count[want == 1] == 1).all() and (count[want == 0] == 0).all()
  assert (want == 1).sum() > (80 if view == 'mirrored' else 400)
  assert np.array_equal(r['cov'][0, 0], (count > 0).astype(F))
  assert r['dropped_extent'] == 0 and r['max_coord'] < 64
  # culling: the mirrored views show the back of every triangle
  culled = R.raster(tex, None, disp, m[None, None], ht, wt, cull_back=True)
  if view == 'magnifying':
    assert np.array_equal(culled['count'], r['count'])
  else:
    assert culled['count'].sum() == 0 and (culled['img'] == 1).all()


def test_scalar_restatement():
  """The vectorised restatement against the definition written triangle by
  triangle and pixel by pixel in Python integers and float32 scalars."""
  nl, h, w, ht, wt = 2, 4, 5, 9, 11
  rs = np.random.RandomState(3)
  tex = rs.rand(nl, 1, h, w, 3).astype(F)
  disp = (0.25 + 0.35 * rs.rand(nl, 1, h, w)).astype(F)
  disp[1] = np.where(rs.rand(1, h, w) < 0.5, disp[0], disp[1] * F(0.5))
  disp[0, 0, 1, 2] = np.nan
  mask = rs.rand(nl, 1, h, w).astype(F)
  m = C.pose_matrix(h, w, ht, wt, C.rotation(0.05, -0.03, 0.08), [0.06, -0.04, -0.8])
  par = dict(disp_min=0.05, mask_min=0.1, edge_ratio=0.45, merge_ratio=0.0, max_extent=4,
             bg_value=0.5)
  got = R.raster(tex, mask, disp, m[None, None], ht, wt, **par)
  e = ldi_mesh_ref.exists(mask[:, 0], disp[:, 0], par['disp_min'], par['mask_min'], 0.0)
  f = lambda v: F(v)

  def vertex(l, y, x):
    if not e[l, y, x]:
      return None
    d, px, py = disp[l, 0, y, x], f(x + 0.5), f(y + 0.5)
    q = [f(f(f(f(px * m[j, 0]) + f(py * m[j, 1])) + m[j, 2]) + f(d * m[j, 3])) for j in range(4)]
    with np.errstate(all='ignore'):
      u, v, dd = f(q[0] / q[2]), f(q[1] / q[2]), f(q[3] / q[2])
    if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(dd) and q[2] > 0 and dd > 0 and
            abs(u) <= 16384 and abs(v) <= 16384):
      return None
    return int(np.rint(f(u * f(256)))), int(np.rint(f(v * f(256)))), dd, d, tex[l, 0, y, x]

  keys = {}
  count = np.zeros((ht, wt), np.int32)
  tris = {}
  for l in range(nl):
    for y in range(h - 1):
      for x in range(w - 1):
        a, b, c, d = (vertex(l, y, x), vertex(l, y, x + 1), vertex(l, y + 1, x),
                      vertex(l, y + 1, x + 1))
        for t, tri in enumerate(((a, c, b), (b, c, d))):
          if any(p is None for p in tri):
            continue
          ds = [p[3] for p in tri]
          if not min(ds) >= f(f(par['edge_ratio']) * max(ds)):
            continue
          p0, p1, p2 = tri
          area = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])
          if area == 0:
            continue
          if area < 0:
            p1, p2, area = p2, p1, -area
          xs_, ys_ = [p[0] for p in tri], [p[1] for p in tri]
          i0, i1 = max((min(xs_) + 127) >> 8, 0), min((max(xs_) - 128) >> 8, wt - 1)
          j0, j1 = max((min(ys_) + 127) >> 8, 0), min((max(ys_) - 128) >> 8, ht - 1)
          if i0 > i1 or j0 > j1 or i1 - i0 >= par['max_extent'] or j1 - j0 >= par['max_extent']:
            continue
          tid = ((l * h + y) * w + x) * 2 + t
          tris[tid] = (p0, p1, p2, area)
          for j in range(ht):                   # every pixel: the box only bounds the work
            for i in range(wt):
              hit = _pixel(p0, p1, p2, area, i, j)
              if hit is None:
                continue
              assert i0 <= i <= i1 and j0 <= j <= j1
              count[j, i] += 1
              z = hit[1]
              if np.isfinite(z) and z > 0:
                key = (int(np.array(z, F).view(np.uint32)) << 32) | (0xFFFFFFFF - tid)
                keys[(j, i)] = max(keys.get((j, i), 0), key)
  assert len(keys) > 20 and len(tris) > 10
  assert np.array_equal(got['count'][0, 0], count)
  for j in range(ht):
    for i in range(wt):
      key = keys.get((j, i), 0)
      if key == 0:
        assert got['cov'][0, 0, j, i] == 0 and (got['img'][0, 0, j, i] == F(0.5)).all()
        assert got['disp'][0, 0, j, i] == 0 and got['winner'][0, 0, j, i] == -1
        continue
      tid = 0xFFFFFFFF - (key & 0xFFFFFFFF)
      p0, p1, p2, area = tris[tid]
      b, z = _pixel(p0, p1, p2, area, i, j)
      col = [f(f(f(b[0] * p0[4][ch]) + f(b[1] * p1[4][ch])) + f(b[2] * p2[4][ch]))
             for ch in range(3)]
      assert got['winner'][0, 0, j, i] == tid and got['cov'][0, 0, j, i] == 1
      assert np.array_equal(got['img'][0, 0, j, i], np.array(col, F))
      assert got['disp'][0, 0, j, i] == z


def _pixel(p0, p1, p2, area, i, j):
  """None outside; else (weights, z)."""
  f = F
  px, py = 256 * i + 128, 256 * j + 128
  es = []
  for a, b in ((p1, p2), (p2, p0), (p0, p1)):
    dx, dy = b[0] - a[0], b[1] - a[1]
    ek = dx * (py - a[1]) - dy * (px - a[0])
    if not (ek > 0 or (ek == 0 and (dy < 0 or (dy == 0 and dx > 0)))):
      return None
    es.append(ek)
  b1, b2 = f(f(es[1]) / f(area)), f(f(es[2]) / f(area))
  b0 = f(f(f(1) - b1) - b2)
  z = f(f(f(b0 * p0[2]) + f(b1 * p1[2])) + f(b2 * p2[2]))
  return (b0, b1, b2), z


def test_nearest_wins_and_ties_go_to_the_lowest_id():
  h, w = 5, 6
  tex, disp = valid_ldi(2, h, w, seed=2)
  disp[1] = disp[0]                              # the two layers coincide
  r = R.raster(tex, None, disp, EYE, h, w)
  ys, xs = np.mgrid[0:h - 1, 0:w - 1]
  assert np.array_equal(r['winner'][0, 0, :-1, :-1], (ys * w + xs) * 2)     # layer 0
  disp[1, 0, 2, 3] = np.nextafter(disp[0, 0, 2, 3], F(1))                   # nearer by one ulp
  r = R.raster(tex, None, disp, EYE, h, w)
  assert r['winner'][0, 0, 2, 3] == ((h + 2) * w + 3) * 2
  assert np.array_equal(r['img'][0, 0, 2, 3], tex[1, 0, 2, 3])


def test_unusable_vertices_and_the_guard():
  h, w = 4, 4
  tex, disp = valid_ldi(1, h, w)
  m = np.eye(4, dtype=F)
  m[0, 0] = 20000.0                              # u beyond the guard from x = 1 on
  r = R.raster(tex, None, disp, m[None, None], 8, 8)
  assert r['triangles'] == 0 and r['cov'].sum() == 0 and r['max_coord'] > 16384
  m = np.eye(4, dtype=F)
  m[2, 2], m[2, 3] = 0.0, -1.0                   # n = -d: behind the camera
  r = R.raster(tex, None, disp, m[None, None], 8, 8)
  assert r['triangles'] == 0
  m = np.eye(4, dtype=F)
  m[3, 3] = -1.0                                 # dd < 0
  assert R.raster(tex, None, disp, m[None, None], 8, 8)['triangles'] == 0


# --- the shared cases are what the issue asks them to be ----------------------------------
@pytest.mark.parametrize('name', sorted(C.CASES))
def test_case_preconditions(name):
  c, r = C.inputs(name), C.reference(name)
  assert r['max_coord'] <= 16384 / 16           # far from the guard
  assert r['triangles'] > 50
  if c['par']['max_extent'] == 2:
    assert 0 < r['dropped_extent'] < r['triangles']
  else:
    assert r['dropped_extent'] == 0
  holes = 1 - r['cov'].mean(axis=(2, 3))
  mb, mv = C.MIRRORED
  if c['par']['cull_back']:
    assert r['cov'][mb, mv].sum() == 0 and (r['img'][mb, mv] == F(0.75)).all()
    holes[mb, mv] = 0.5
  assert (holes > 0.02).all() and (holes < 0.98).all()     # every view shows both
  assert np.array_equal(r['cov'], (r['winner'] >= 0).astype(F))
  assert ((r['disp'] > 0) == (r['cov'] == 1)).all()
  assert np.isnan(c['disp']).any() and np.isinf(c['disp']).any() and (c['disp'] == F(0.01)).any()


def test_cases_exercise_ties_cuts_and_merging():
  c, r = C.inputs('small-packed'), C.reference('small-packed')
  # each layer on its own: where both reach a pixel at bitwise the same depth, the
  # two together give it to layer 0, the lower id
  alone = [R.raster(c['tex'][l:l + 1], None, c['disp'][l:l + 1], c['M'], c['ht'], c['wt'],
                    **c['par']) for l in range(2)]
  tie = ((alone[0]['cov'] == 1) & (alone[1]['cov'] == 1) &
         (alone[0]['disp'].view(np.uint32) == alone[1]['disp'].view(np.uint32)))
  assert tie[C.IDENTITY].sum() > 10 and tie.sum() > tie[C.IDENTITY].sum()
  assert np.array_equal(r['winner'][tie], alone[0]['winner'][tie])
  assert np.array_equal(r['img'][tie], alone[0]['img'][tie])
  nearer = (alone[1]['cov'] == 1) & (alone[1]['disp'] > alone[0]['disp'])
  assert nearer.sum() > 0 and (r['winner'][nearer] >= 2 * 9 * 13).all()
  cut, merged = C.reference('big-packed-mask-cut'), C.reference('big-planar-merge')
  plain = R.raster(c['tex'], None, c['disp'], c['M'], c['ht'], c['wt'],
                   **dict(c['par'], edge_ratio=0.8))
  assert plain['triangles'] < r['triangles']
  assert cut['triangles'] > 0 and merged['triangles'] > 0
  # the general pose magnifies: some triangle covers more than one pixel
  assert (np.bincount(r['winner'][C.GENERAL][r['winner'][C.GENERAL] >= 0]) > 1).any()


# --- refusals that need no device ---------------------------------------------------------
def test_rasterize_ldi_refuses_before_it_looks_for_a_device(built_lib):
  from lsi.geometry import raster
  tex, disp = torch.rand(2, 1, 8, 8, 3), torch.rand(2, 1, 8, 8, 1)
  m = torch.eye(4)[None, None]
  size = (8, 8)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    raster.rasterize_ldi([tex, None, disp], m, size)
  with pytest.raises(RuntimeError, match='fp32'):
    raster.rasterize_ldi([tex.double(), None, disp], m, size)
  with pytest.raises(RuntimeError, match='fp32'):
    raster.rasterize_ldi([tex, None, disp], m.double(), size)
  with pytest.raises(RuntimeError, match='L x B x H x W x 3'):
    raster.rasterize_ldi([torch.rand(2, 1, 8, 8, 4), None, disp], m, size)
  with pytest.raises(RuntimeError, match='L x B x H x W x 3'):
    raster.rasterize_ldi([tex[0], None, disp], m, size)
  with pytest.raises(RuntimeError, match='disp is'):
    raster.rasterize_ldi([tex, None, torch.rand(2, 1, 8, 7, 1)], m, size)
  with pytest.raises(RuntimeError, match='mask is'):
    raster.rasterize_ldi([tex, torch.rand(1, 1, 8, 8), disp], m, size)
  with pytest.raises(RuntimeError, match='src2trg_mat is B x V x 4 x 4'):
    raster.rasterize_ldi([tex, None, disp], torch.eye(4)[None], size)
  with pytest.raises(RuntimeError, match='src2trg_mat is B x V x 4 x 4'):
    raster.rasterize_ldi([tex, None, disp], torch.eye(4).expand(2, 1, 4, 4), size)
  with pytest.raises(RuntimeError, match='nothing to rasterise'):
    raster.rasterize_ldi([tex[:, :, :0], None, disp[:, :, :0]], m, size)
  with pytest.raises(RuntimeError, match='nothing to rasterise'):
    raster.rasterize_ldi([tex, None, disp], m[:, :0], size)
  with pytest.raises(RuntimeError, match='trg_size'):
    raster.rasterize_ldi([tex, None, disp], m, (0, 8))
  with pytest.raises(RuntimeError, match='trg_size'):
    raster.rasterize_ldi([tex, None, disp], m, (8, 8193))
  with pytest.raises(TypeError, match='trg_size'):
    raster.rasterize_ldi([tex, None, disp], m, 8)
  with pytest.raises(TypeError):
    raster.rasterize_ldi([tex.numpy(), None, disp], m, size)
  with pytest.raises(TypeError):
    raster.rasterize_ldi([tex, disp], m, size)


def test_render_views_builds_the_matrices_on_the_host(built_lib):
  from lsi.geometry import projection, raster
  h, w, nv = 8, 12, 3
  k = torch.tensor(C.intrinsics(h, w), dtype=torch.float32)
  rot = torch.tensor(np.stack([C.rotation(0.01 * i, 0, 0) for i in range(nv)]),
                     dtype=torch.float32)
  t = torch.tensor([[[0.1 * i], [0.0], [0.0]] for i in range(nv)])
  ks = k.expand(nv, 3, 3)
  m = raster.view_matrices(1, ks, ks, rot, t, trg_downsampling=0.5)
  assert tuple(m.shape) == (1, nv, 4, 4) and m.dtype == torch.float32
  full = projection.forward_projection_matrix(ks, ks, rot, t).cpu().float()
  assert torch.equal(m[0, :, 2:], full[:, 2:]) and torch.equal(m[0, :, :2], full[:, :2] * 0.5)
  # B x V cameras
  m2 = raster.view_matrices(2, ks.expand(2, nv, 3, 3), ks.expand(2, nv, 3, 3),
                            rot.expand(2, nv, 3, 3), t.expand(2, nv, 3, 1))
  assert tuple(m2.shape) == (2, nv, 4, 4) and torch.equal(m2[1], full)
  with pytest.raises(RuntimeError, match='one item'):
    raster.view_matrices(2, ks, ks, rot, t)
  with pytest.raises(RuntimeError, match='rot is'):
    raster.view_matrices(1, ks, ks, rot[:2], t)
  tex, disp = torch.rand(2, 1, h, w, 3), torch.rand(2, 1, h, w, 1)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    raster.render_views([tex, None, disp], ks, ks, rot, t)
  with pytest.raises(TypeError):
    raster.render_views(tex, ks, ks, rot, t)


def raster_desc(_C, L=2, B=2, H=8, W=8, **kw):
  d = _C.LsiRasterDesc()
  d.L, d.B, d.H, d.W = L, B, H, W
  d.tex_sc, d.tex_sx, d.tex_sy, d.tex_sb, d.tex_sl = 1, 3, 3 * W, 3 * W * H, 3 * W * H * B
  d.disp_sx, d.disp_sy, d.disp_sb, d.disp_sl = 1, W, W * H, W * H * B
  d.mask_sx, d.mask_sy, d.mask_sb, d.mask_sl = 1, W, W * H, W * H * B
  d.V, d.Ht, d.Wt, d.max_extent = 3, 10, 12, 32
  d.disp_min, d.mask_min, d.edge_ratio, d.merge_ratio = 1e-3, 0.5, 0.9, 0.0
  d.bg_value = 1.0
  for key, value in kw.items():
    setattr(d, key, value)
  return d


# what the library refuses with LSI_EINVAL: lsi_ldi_mesh's shared fields ...
BAD_DESCRIPTORS = [
    dict(L=0), dict(B=0), dict(B=65536), dict(H=0), dict(W=-1),
    dict(L=1, H=16384, W=16385),                     # L H W > 2^28
    dict(L=65536, H=65536, W=65536),
    dict(tex_sl=-1), dict(tex_sc=-1), dict(disp_sy=-8), dict(mask_sx=-1),
    dict(disp_min=0.0), dict(disp_min=-1.0), dict(disp_min=float('nan')),
    dict(disp_min=float('inf')), dict(mask_min=float('nan')), dict(mask_min=float('inf')),
    dict(edge_ratio=-0.1), dict(edge_ratio=1.5), dict(edge_ratio=float('nan')),
    dict(merge_ratio=-0.1), dict(merge_ratio=1.01), dict(merge_ratio=float('nan')),
    # ... and the rasteriser's own
    dict(V=0), dict(V=-1), dict(V=1025), dict(B=64, V=1024), dict(B=21846, V=3),
    dict(Ht=0), dict(Ht=8193), dict(Wt=0), dict(Wt=8193), dict(Wt=-4),
    dict(max_extent=0), dict(max_extent=257), dict(max_extent=-1),
    dict(bg_value=float('nan')), dict(bg_value=float('inf')), dict(bg_value=float('-inf')),
    dict(flags=2), dict(flags=0x80000001), dict(reserved=1),
]
BAD_ARGUMENTS = [
    dict(tex=66), dict(mask=65), dict(disp=62), dict(M=63), dict(img=66), dict(cov=65),
    dict(out_disp=70), dict(workspace=72),
]


def test_library_refuses_before_any_launch(built_lib):
  """Host answers of the two entry points, in the header's order EINVAL ->
  ENULL -> EWORKSPACE: no pointer is touched."""
  from lsi import _C
  lib = _C.lib()
  size = lib.lsi_ldi_raster_workspace_bytes
  names = ('tex', 'mask', 'disp', 'M', 'img', 'cov', 'out_disp', 'workspace')

  def call(d, nbytes=1 << 50, **ptrs):
    p = dict({n: 64 for n in names}, **ptrs)
    return lib.lsi_ldi_raster(ctypes.byref(d), p['tex'], p['mask'], p['disp'], p['M'], p['img'],
                              p['cov'], p['out_disp'], p['workspace'], nbytes, None)

  assert lib.lsi_ldi_raster(None, 64, 64, 64, 64, 64, 64, 64, 64, 1 << 50, None) == -1
  assert size(None) == 0
  for kw in BAD_DESCRIPTORS:
    d = raster_desc(_C, **kw)
    assert size(ctypes.byref(d)) == 0 and call(d) == -1, kw
    assert call(d, tex=None) == -1, kw               # EINVAL comes before ENULL
  good = raster_desc(_C)
  for kw in BAD_ARGUMENTS:
    assert call(good, **kw) == -1, kw
    assert call(good, **dict(kw, disp=kw.get('disp') or None)) == -1, kw
  # what is taken: the limits themselves, and every required pointer on its own
  for kw in (dict(), dict(L=1, B=1, H=1, W=1, V=1, Ht=1, Wt=1, max_extent=1),
             dict(L=1, B=63, V=1024, H=16384, W=16384, Ht=8192, Wt=8192, max_extent=256),
             dict(B=65535, V=1), dict(B=21845, V=3),
             dict(edge_ratio=0.0, merge_ratio=1.0, flags=1, bg_value=-2.0), dict(edge_ratio=1.0)):
    d = raster_desc(_C, **kw)
    need = size(ctypes.byref(d))
    views, n = d.B * d.V, d.L * d.H * d.W
    assert need == (views * d.Ht * d.Wt * 8 + 15) // 16 * 16 + views * n * 16, kw
    for miss in ('tex', 'disp', 'M', 'img', 'cov', 'workspace'):
      assert call(d, **{miss: None}) == -2, (kw, miss)
    assert call(d, tex=None, nbytes=0) == -2, kw     # ENULL comes before EWORKSPACE
    assert call(d, nbytes=need - 1) == -3, kw
    # the mask and the disparity output may be NULL
    assert call(d, mask=None, out_disp=None, nbytes=need - 1) == -3, kw
