"""lsi_ldi_mesh (csrc/lsi_ldi_mesh.hip) against its float32 restatement
(tests/ldi_mesh_ref.py): np.array_equal on the vertex bytes, the face bytes and
the counts, no tolerance.  Every call writes into buffers pre-filled with 0xA5
that are three records per item and 64 bytes longer than the capacity needs, and
the WHOLE buffers are compared: an item's unused records, the bytes between the
items and the guard behind the last one must come back as they were.

Shapes (L, B, H, W): the smallest at which each mechanism can go wrong -- one
texel; a row and a column (no quads); one quad; a small batch; 33 x 65, ragged
against a 64-lane wave and a 256-texel workgroup in both directions; 64 x 96
with three items; and SCAN, whose items have CHUNK * TRIP + 254 texels, one
workgroup total more than scan_kernel takes in a trip."""
import numpy as np
import pytest
import torch

import ldi_mesh_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
GUARD, FILL, SLACK = 64, 0xA5, 3
CHUNK, TRIP = 256, 256                     # LSI_MESH_CHUNK, LSI_MESH_SCAN_TRIP (checked below)
SCAN = (2, 1, CHUNK * TRIP // (2 * 255) + 1, 255)
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 7), (1, 2, 7, 1), (1, 1, 2, 2), (2, 2, 5, 3), (3, 1, 33, 65),
          (2, 3, 64, 96), SCAN]
PATTERNS = ['valid', 'none', 'invalid', 'edges', 'merge', 'mask', 'colour']
PAR = dict(disp_min=0.05, mask_min=0.25, edge_ratio=0.3, merge_ratio=0.0, flip_yz=False)


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  from lsi import _C
  assert (_C.LSI_MESH_CHUNK, _C.LSI_MESH_SCAN_TRIP) == (CHUNK, TRIP)
  n = SCAN[0] * SCAN[2] * SCAN[3]
  assert (n + CHUNK - 1) // CHUNK == TRIP + 1
  return torch.device('cuda:0')


def intrinsics(nb, h, w):
  k = np.zeros((nb, 3, 3), F)
  for b in range(nb):
    k[b] = [[0.58 * w + 3 * b + 1, 0, 0.5 * w + 0.25 * b], [0, 0.61 * w + 2, 0.5 * h - 0.125 * b],
            [0, 0, 1]]
  return k


def kinv_of(k):
  from lsi.geometry import projection
  return projection._inv3(torch.from_numpy(k)).numpy().reshape(-1, 9)


def scene(pattern, shape, seed=0):
  """(tex, mask or None, disp, parameters) of a pattern: float32 arrays
  L x B x H x W [x 3]."""
  nl, nb, h, w = shape
  rs = np.random.RandomState(seed + 17 * PATTERNS.index(pattern))
  par = dict(PAR)
  tex = rs.rand(nl, nb, h, w, 3).astype(F)
  disp = (0.06 + 0.9 * rs.rand(nl, nb, h, w)).astype(F)
  mask = None
  if pattern == 'none':
    disp = rs.choice(np.array([0, np.nan, -1, 0.01], F), size=disp.shape)
  elif pattern == 'invalid':
    below = np.nextafter(F(par['disp_min']), F(0))
    bad = np.array([np.nan, np.inf, -np.inf, 0, -0.5, below], F)
    hit = rs.rand(*disp.shape) < 0.3
    disp[hit] = rs.choice(bad, size=int(hit.sum()))
    disp.reshape(-1)[0] = par['disp_min']                   # at the limit exactly: in range
  elif pattern == 'edges':
    disp[:] = 0.5
    disp[..., w // 2:] = 0.4                                # a step in x: ratio 0.8 < 0.9
    disp[..., h // 2:, :] *= F(0.5)                         # and one in y
    disp[:, :, h // 3, w // 3] = 1.0                        # a one-texel spike
    disp[:, :, h - 1, w - 1] = 0.9                          # corner d of the last quad only
    par['edge_ratio'] = 0.9
  elif pattern == 'merge':
    par['merge_ratio'] = 0.9
    if nl > 1:
      front = disp[0].copy()
      at = (F(0.9) * front).astype(F)
      pick = rs.randint(0, 5, size=front.shape)
      back = np.where(pick == 0, at, disp[1])
      back = np.where(pick == 1, np.nextafter(at, F(2)), back)
      back = np.where(pick == 2, np.nextafter(at, F(0)), back)
      back = np.where(pick == 3, front, back)
      gone = rs.rand(*front.shape) < 0.25                   # behind an out-of-range layer 0
      disp[0][gone] = rs.choice(np.array([np.nan, 0, 0.01], F), size=int(gone.sum()))
      disp[1] = back.astype(F)
  elif pattern == 'mask':
    at = F(par['mask_min'])
    values = np.array([np.nan, at, np.nextafter(at, F(1)), np.nextafter(at, F(0)), 0, 1, -1,
                       np.inf], F)
    mask = rs.choice(values, size=disp.shape)
  elif pattern == 'colour':
    k = rs.randint(0, 256, size=tex.shape).astype(F)
    centre = ((k + F(0.5)) / F(255)).astype(F)              # around the rounding boundary
    pick = rs.randint(0, 8, size=tex.shape)
    tex = np.where(pick == 0, centre, tex)
    tex = np.where(pick == 1, np.nextafter(centre, F(2)), tex)
    tex = np.where(pick == 2, np.nextafter(centre, F(-1)), tex)
    tex = np.where(pick == 3, -tex, tex)
    tex = np.where(pick == 4, F(1) + tex, tex)
    tex = np.where(pick == 5, F(np.nan), tex)
    tex = np.where(pick == 6, (k / F(255)).astype(F), tex).astype(F)
    tex.reshape(-1)[:3] = [np.inf, -np.inf, 1.0]
  return tex, mask, disp, par


def on_device(dev, tex, mask, disp, layout):
  """The LDI as device tensors L x B x H x W x C in one of the three layouts."""
  t, d = torch.from_numpy(tex), torch.from_numpy(disp)[..., None]
  m = None if mask is None else torch.from_numpy(mask)[..., None]
  if layout == 'contiguous':
    out = [t.to(dev), None if m is None else m.to(dev), d.to(dev)]
    assert out[0].is_contiguous() and out[2].is_contiguous()
  elif layout == 'packed':                     # views of one RGBD buffer
    buf = torch.cat([t, d], -1).to(dev).contiguous()
    out = [buf[..., :3], None if m is None else m.to(dev), buf[..., 3:]]
    assert out[2].data_ptr() == out[0].data_ptr() + 12 and out[0].stride() == out[2].stride()
  else:                                        # planar: permuted N C H W
    planar = lambda x: x.permute(0, 1, 4, 2, 3).contiguous().to(dev).permute(0, 1, 3, 4, 2)
    out = [planar(t), None if m is None else planar(m), planar(d)]
    assert out[0].stride(4) == tex.shape[2] * tex.shape[3] and not out[0].is_contiguous()
  return out


def capacities(shape):
  nl, _, h, w = shape
  return nl * h * w + SLACK, 2 * nl * (h - 1) * (w - 1) + SLACK


def export(dev, tex, mask, disp, k, par, layout='contiguous', capacity=None):
  """One call into fresh pre-filled buffers: (LdiMesh, vertex bytes, face bytes,
  counts) with the bytes and counts on the host."""
  from lsi.geometry import mesh
  nb = tex.shape[1]
  vcap, fcap = capacity or capacities(tex.shape[:4])
  vbuf = torch.full((nb * vcap * 16 + GUARD,), FILL, dtype=torch.uint8, device=dev)
  fbuf = torch.full((nb * fcap * 13 + GUARD,), FILL, dtype=torch.uint8, device=dev)
  counts = torch.full((nb, 2), -7, dtype=torch.int32, device=dev)
  m = mesh.ldi_mesh(on_device(dev, tex, mask, disp, layout), torch.from_numpy(k),
                    capacity=(vcap, fcap), out=(vbuf, fbuf, counts), **par)
  return m, vbuf.cpu().numpy(), fbuf.cpu().numpy(), counts.cpu().numpy()


def expected(tex, mask, disp, k, par, capacity=None):
  nb = tex.shape[1]
  vcap, fcap = capacity or capacities(tex.shape[:4])
  meshes = R.mesh(tex, mask, disp, kinv_of(k), **par)
  return meshes, R.pack(meshes, vcap, fcap,
                        np.full(nb * vcap * 16 + GUARD, FILL, np.uint8),
                        np.full(nb * fcap * 13 + GUARD, FILL, np.uint8))


def same(got, want, what):
  _, vb, fb, counts = got
  wv, wf, wc = want
  assert np.array_equal(counts, wc), (what, counts.tolist(), wc.tolist())
  assert np.array_equal(vb, wv), (what, 'vertex bytes', int(np.argmax(vb != wv)))
  assert np.array_equal(fb, wf), (what, 'face bytes', int(np.argmax(fb != wf)))


# every pattern on every shape where it makes sense: merging needs a second layer
CASES = [(s, p) for s in SHAPES for p in PATTERNS if p != 'merge' or s[0] > 1]


@pytest.mark.parametrize('shape,pattern', CASES,
                         ids=['%s-%s' % ('x'.join(map(str, s)), p) for s, p in CASES])
def test_bytes_and_counts_are_the_restatements(dev, shape, pattern):
  tex, mask, disp, par = scene(pattern, shape)
  k = intrinsics(shape[1], shape[2], shape[3])
  meshes, want = expected(tex, mask, disp, k, par)
  got = export(dev, tex, mask, disp, k, par)
  same(got, want, (shape, pattern))
  nv, nf = want[2].sum(0)
  if pattern == 'none':
    assert nv == 0 and nf == 0 and (got[1] == FILL).all() and (got[2] == FILL).all()
  elif pattern == 'valid':
    assert nv == np.prod(shape)
  elif shape[2] > 1 and shape[3] > 1 and np.prod(shape) > 100:
    # the pattern cut something and left something
    full = 2 * shape[0] * shape[1] * (shape[2] - 1) * (shape[3] - 1)
    assert 0 < nf < full, (nf, full)


def test_a_quad_loses_one_triangle_and_keeps_the_other(dev):
  shape = (1, 1, 5, 6)
  tex, mask, disp, par = scene('edges', shape)
  k = intrinsics(1, 5, 6)
  (v, f), = R.mesh(tex, mask, disp, kinv_of(k), **par)
  # the last quad: only its corner d differs, triangle 0 stays and triangle 1 goes
  a = 3 * 6 + 4
  assert (f['i'] == [a, a + 6, a + 1]).all(1).any() and not (f['i'][:, 0] == a + 1).any()
  same(export(dev, tex, mask, disp, k, par), expected(tex, mask, disp, k, par)[1], shape)


def test_no_face_buffer(dev):
  """H or W = 1: the default capacity for faces is 0 and no face buffer is
  given (3 launches); the counts are still written."""
  from lsi.geometry import mesh
  for shape in ((1, 1, 1, 1), (2, 1, 1, 7), (1, 2, 7, 1)):
    tex, mask, disp, par = scene('invalid', shape, seed=3)
    k = intrinsics(shape[1], shape[2], shape[3])
    m = mesh.ldi_mesh(on_device(dev, tex, mask, disp, 'contiguous'), torch.from_numpy(k), **par)
    assert m.face_capacity == 0 and m.faces.numel() == 0
    want = R.mesh(tex, mask, disp, kinv_of(k), **par)
    assert m.counts.cpu().numpy().tolist() == [[len(v), 0] for v, _ in want]
    for (v, f), (wv, wf) in zip(m.to_host(), want):
      assert v.tobytes() == wv.tobytes() and len(f) == 0 and f.dtype == R.FACE


@pytest.mark.parametrize('shape', [(2, 2, 5, 3), (3, 1, 33, 65), (2, 3, 64, 96)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_layouts_give_the_same_bytes(dev, shape):
  tex, _, disp, par = scene('invalid', shape, seed=1)
  _, mask, _, _ = scene('mask', shape, seed=1)
  par['merge_ratio'] = 0.9
  k = intrinsics(shape[1], shape[2], shape[3])
  _, want = expected(tex, mask, disp, k, par)
  for layout in ('contiguous', 'packed', 'planar'):
    same(export(dev, tex, mask, disp, k, par, layout), want, (shape, layout))
    same(export(dev, tex, None, disp, k, par, layout), expected(tex, None, disp, k, par)[1],
         (shape, layout, 'no mask'))


@pytest.mark.parametrize('shape', [(2, 2, 5, 3), (3, 1, 33, 65)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_flip_yz(dev, shape):
  tex, mask, disp, par = scene('invalid', shape, seed=2)
  par['flip_yz'] = True
  k = intrinsics(shape[1], shape[2], shape[3])
  meshes, want = expected(tex, mask, disp, k, par)
  same(export(dev, tex, mask, disp, k, par), want, shape)
  par['flip_yz'] = False
  plain = R.mesh(tex, mask, disp, kinv_of(k), **par)
  for (v, _), (p, _) in zip(meshes, plain):
    assert np.array_equal(v['y'], -p['y']) and np.array_equal(v['z'], -p['z'])
    assert np.array_equal(v['x'], p['x'])


@pytest.mark.parametrize('short', ['vertices', 'faces'])
def test_capacity_below_the_count(dev, short):
  shape = (2, 3, 64, 96)
  tex, mask, disp, par = scene('invalid', shape, seed=4)
  k = intrinsics(shape[1], shape[2], shape[3])
  counts = np.array([[len(v), len(f)] for v, f in R.mesh(tex, mask, disp, kinv_of(k), **par)])
  vcap, fcap = capacities(shape)
  if short == 'vertices':
    vcap = int(counts[:, 0].min()) // 2 + 1
  else:
    fcap = (int(counts[:, 1].min()) // 2) | 1        # odd: the items' byte phases differ
  assert (counts[:, 0] > vcap).all() or (counts[:, 1] > fcap).all()
  meshes, want = expected(tex, mask, disp, k, par, (vcap, fcap))
  got = export(dev, tex, mask, disp, k, par, capacity=(vcap, fcap))
  assert np.array_equal(want[2], counts)             # the true totals
  same(got, want, short)                             # prefixes, guards, the next item's region
  with pytest.raises(RuntimeError, match='truncated'):
    got[0].to_host()


def test_capacities_at_every_byte_phase(dev):
  """Face capacities 1 .. 9 on a small batch: every phase of an item's first
  byte and of a workgroup's first and last byte against the dwords."""
  shape = (2, 3, 5, 3)
  tex, mask, disp, par = scene('valid', shape, seed=5)
  par['edge_ratio'] = 0.0
  k = intrinsics(3, 5, 3)
  for fcap in range(1, 10):
    cap = (7, fcap)
    same(export(dev, tex, mask, disp, k, par, capacity=cap),
         expected(tex, mask, disp, k, par, cap)[1], cap)


def test_two_calls_are_byte_equal(dev):
  shape = (3, 1, 33, 65)
  tex, mask, disp, par = scene('invalid', shape, seed=6)
  k = intrinsics(1, 33, 65)
  a, b = (export(dev, tex, mask, disp, k, par) for _ in range(2))
  for x, y in zip(a[1:], b[1:]):
    assert np.array_equal(x, y)


def test_to_host_and_files(dev, tmp_path):
  from lsi.geometry import mesh
  shape = (2, 2, 5, 3)
  tex, mask, disp, par = scene('invalid', shape, seed=7)
  k = intrinsics(2, 5, 3)
  m = mesh.ldi_mesh(on_device(dev, tex, mask, disp, 'packed'), torch.from_numpy(k).to(dev), **par)
  assert (m.vertex_capacity, m.face_capacity) == mesh.full_capacity(2, 5, 3)
  want = R.mesh(tex, mask, disp, kinv_of(k), **par)
  for b, ((v, f), (wv, wf)) in enumerate(zip(m.to_host(), want)):
    assert v.dtype == R.VERTEX and f.dtype == R.FACE
    assert v.tobytes() == wv.tobytes() and f.tobytes() == wf.tobytes()
    path = str(tmp_path / ('%d.ply' % b))
    mesh.write_ply(path, v, f)
    v2, f2 = mesh.read_ply(path)
    assert v2.tobytes() == wv.tobytes() and f2.tobytes() == wf.tobytes()


@pytest.mark.parametrize('shape', [(3, 1, 33, 65), (2, 3, 64, 96)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_op_route(dev, shape):
  """ldi_mesh_ops on the device states section 4.24 in its order of operations,
  one rounded torch op per operation of the definition (no op of it fuses a
  multiply with an add, and torch's fp32 division is correctly rounded): counts,
  faces, colours AND positions are equal bit for bit."""
  from lsi.geometry import mesh
  tex, _, disp, par = scene('invalid', shape, seed=8)
  _, mask, _, _ = scene('mask', shape, seed=8)
  par.update(merge_ratio=0.9, flip_yz=True)
  k = intrinsics(shape[1], shape[2], shape[3])
  want = R.mesh(tex, mask, disp, kinv_of(k), **par)
  got = mesh.ldi_mesh_ops(on_device(dev, tex, mask, disp, 'packed'), torch.from_numpy(k), **par)
  for (v, f), (pos, col, faces) in zip(want, got):
    assert pos.is_cuda
    assert (len(pos), len(faces)) == (len(v), len(f))
    assert np.array_equal(faces.cpu().numpy().reshape(-1, 3), f['i'])
    assert np.array_equal(col.cpu().numpy(),
                          np.stack([v['red'], v['green'], v['blue'], v['alpha']], -1))
    p = np.stack([v['x'], v['y'], v['z']], -1)
    q = pos.cpu().numpy()
    print('positions: max |difference| %g' % (np.abs(q - p).max() if len(p) else 0.0))
    assert np.array_equal(q.view(np.uint32), p.view(np.uint32))
