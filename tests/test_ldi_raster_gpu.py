"""lsi_ldi_raster against its float32 / int64 restatement (tests/ldi_raster_ref.py)
with np.array_equal: the definition leaves nothing to tolerance.  The cases are
tests/ldi_raster_cases.py (their preconditions are asserted on the restatement in
test_ldi_raster_cpu.py); their references are computed once and read only."""
import numpy as np
import pytest
import torch

import ldi_raster_cases as C
import ldi_raster_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def device_ldi(c, dev):
  """[tex, mask, disp] on the device in the case's layout: views of one packed
  RGBD buffer, or planar (permuted) tensors."""
  tex, disp = torch.from_numpy(c['tex']).to(dev), torch.from_numpy(c['disp']).to(dev)
  if c['layout'] == 'packed':
    buf = torch.cat([tex, disp[..., None]], -1).contiguous()
    tex, disp = buf[..., :3], buf[..., 3:4]
    assert tex.stride(3) == 4 and disp.stride(3) == 4
  else:
    tex = tex.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
    assert tex.stride(4) == tex.shape[2] * tex.shape[3]
  mask = None if c['mask'] is None else torch.from_numpy(c['mask']).to(dev)
  return [tex, mask, disp]


def bits(a):
  a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
  return np.ascontiguousarray(a, F).view(np.uint32)


def assert_equals_reference(got, want):
  img, cov, disp = got
  assert np.array_equal(bits(cov), bits(want['cov']))
  if disp is not None:
    assert np.array_equal(bits(disp), bits(want['disp']))
  assert np.array_equal(bits(img), bits(want['img']))


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_equals_the_restatement(dev, name):
  from lsi.geometry import raster
  c, want = C.inputs(name), C.reference(name)
  got = raster.rasterize_ldi(device_ldi(c, dev), torch.from_numpy(c['M']), (c['ht'], c['wt']),
                             **c['par'])
  assert_equals_reference(got, want)
  assert want['triangles'] > 0 and want['cov'].sum() > 0
  if c['par']['cull_back']:
    assert float(got[1][C.MIRRORED].sum()) == 0           # the mirrored view covers nothing


def test_reuse_with_stale_contents_and_without_the_disparity(dev):
  """out= and workspace= that hold another call's results and keys; then a NULL
  out_disp, which leaves the other two outputs what they were."""
  from lsi.geometry import raster
  a, b = 'big-packed-mask-cut', 'big-planar-merge'        # one shape, different pictures
  ca, cb = C.inputs(a), C.inputs(b)
  size = (ca['ht'], ca['wt'])
  first = raster.rasterize_ldi(device_ldi(cb, dev), torch.from_numpy(cb['M']), size, **cb['par'])
  assert_equals_reference(first, C.reference(b))
  nb, nv = ca['M'].shape[:2]
  work = torch.full((int(1.5 * (nb * nv * (size[0] * size[1] * 8 + ca['disp'][:, 0].size * 16))),),
                    0xA5, dtype=torch.uint8, device=dev)
  out = tuple(torch.full_like(t, float('nan')) for t in first)
  for cx, name in ((cb, b), (ca, a), (ca, a)):            # stale keys of b, then of a itself
    got = raster.rasterize_ldi(device_ldi(cx, dev), torch.from_numpy(cx['M']), size, out=out,
                               workspace=work, **cx['par'])
    assert all(g is o for g, o in zip(got, out))
    assert_equals_reference(got, C.reference(name))
  keep = out[2].clone()
  out[0].fill_(7.0), out[1].fill_(7.0)
  got = raster.rasterize_ldi(device_ldi(cb, dev), torch.from_numpy(cb['M']), size,
                             out=(out[0], out[1], None), workspace=work, **cb['par'])
  assert got[2] is None and torch.equal(out[2], keep)
  assert_equals_reference(got, C.reference(b))
  with pytest.raises(RuntimeError, match='out: cov'):
    raster.rasterize_ldi(device_ldi(cb, dev), torch.from_numpy(cb['M']), size,
                         out=(out[0], out[1][:, :2], None), **cb['par'])
  with pytest.raises(RuntimeError, match='workspace'):
    raster.rasterize_ldi(device_ldi(cb, dev), torch.from_numpy(cb['M']), size,
                         workspace=work[:64], **cb['par'])


def test_two_calls_are_bitwise_equal(dev):
  from lsi.geometry import raster
  c = C.inputs('big-packed-mask-cut')
  ldi, m = device_ldi(c, dev), torch.from_numpy(c['M'])
  one = raster.rasterize_ldi(ldi, m, (c['ht'], c['wt']), **c['par'])
  two = raster.rasterize_ldi(ldi, m, (c['ht'], c['wt']), **c['par'])
  for x, y in zip(one, two):
    assert x.data_ptr() != y.data_ptr() and np.array_equal(bits(x), bits(y))


def test_identity_returns_the_texels(dev):
  from lsi.geometry import raster
  h, w = 20, 37
  rs = np.random.RandomState(5)
  tex = torch.from_numpy(rs.rand(2, 1, h, w, 3).astype(F)).to(dev)
  disp = torch.from_numpy((0.2 + 0.5 * rs.rand(2, 1, h, w, 1)).astype(F)).to(dev)
  disp[1] *= 0.25
  img, cov, od = raster.rasterize_ldi([tex, None, disp], torch.eye(4)[None, None], (h, w),
                                      edge_ratio=0.0)
  assert torch.equal(cov[0, 0, :-1, :-1], torch.ones_like(cov[0, 0, :-1, :-1]))
  assert float(cov[0, 0, -1].sum()) == 0 and float(cov[0, 0, :, -1].sum()) == 0
  assert torch.equal(img[0, 0, :-1, :-1], tex[0, 0, :-1, :-1])
  assert torch.equal(od[0, 0, :-1, :-1], disp[0, 0, :-1, :-1, 0])
  assert torch.equal(img[0, 0, -1], torch.ones_like(img[0, 0, -1]))
  assert float(od[0, 0, -1].abs().sum()) == 0


def test_magnified_single_layer_has_no_cracks(dev):
  from lsi.geometry import raster
  h, w, ht, wt = 20, 37, 56, 100
  rs = np.random.RandomState(6)
  tex = rs.rand(1, 1, h, w, 3).astype(F)
  disp = (0.2 + 0.5 * rs.rand(1, 1, h, w)).astype(F)
  m = C.magnifying_matrix()[None, None]
  want = R.raster(tex, None, disp, m, ht, wt)
  assert want['count'].max() == 1 and want['dropped_extent'] == 0 and want['max_coord'] < 128
  y0, y1, x0, x1 = C.interior(want['count'][0, 0])
  assert (y1 - y0 + 1) * (x1 - x0 + 1) > 0.5 * ht * wt       # most of the frame
  img, cov, od = raster.rasterize_ldi(
      [torch.from_numpy(tex).to(dev), None, torch.from_numpy(disp).to(dev)],
      torch.from_numpy(m), (ht, wt), edge_ratio=0.0)
  inner = cov[0, 0, y0:y1 + 1, x0:x1 + 1]
  assert torch.equal(inner, torch.ones_like(inner))
  assert_equals_reference((img, cov, od), want)


def test_render_views_equals_rasterize_ldi(dev):
  """V cameras for an LDI of one item: the matrices are built on the host."""
  from lsi.geometry import raster
  c = C.inputs('small-packed')
  h, w = c['disp'].shape[2:]
  ldi = [t if t is None else t[:, :1] for t in device_ldi(c, dev)]
  k = torch.tensor(C.intrinsics(h, w), dtype=torch.float32).expand(2, 3, 3)
  rot = torch.tensor(np.stack([np.eye(3), C.rotation(0.05, -0.03, 0.08)]), dtype=torch.float32)
  t = torch.tensor([[[-0.3], [0.0], [0.0]], [[0.06], [-0.04], [-0.5]]])
  got = raster.render_views(ldi, k, k, rot, t, trg_downsampling=1.5, **c['par'])
  m = raster.view_matrices(1, k, k, rot, t, 1.5)
  assert tuple(got[0].shape) == (1, 2, int(h * 1.5), int(w * 1.5), 3)
  want = R.raster(c['tex'][:, :1], None, c['disp'][:, :1], m.numpy(), int(h * 1.5), int(w * 1.5),
                  **c['par'])
  assert want['cov'].sum() > 50 and want['max_coord'] < 1024
  assert_equals_reference(got, want)
