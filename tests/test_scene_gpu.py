"""lsi_render_planes / layers.render_planes / BatchedDataLoader on the GPU:
against the reference's planar_transform outputs, against the op route
(transform_plane_imgs -> trg_disp_maps -> compose / compose_depth) exactly,
under hostile homographies, and the loader against DataLoader."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import lsi_oracle as O
from conftest import PKG, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def T(a, dev):
  return torch.tensor(np.asarray(a, dtype=np.float32), device=dev)


# ---------------------------------------------------------------------------
# 1. against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('soft,min_disp,temp', [(False, 0.2, 0.4), (False, 1e-6, 1),
                                                (True, 1e-3, 0.4)])
def test_against_the_reference_planar_transform(dev, soft, min_disp, temp):
  """Expected: the oracle's compose / compose_depth on the REFERENCE's
  planar_transform outputs (layers.npz).  Hard composition: a pixel is left out
  only where the oracle's two largest layer probabilities differ by < 1e-4, and
  at most 1 % of the 640 pixels may be (computed before the kernel runs; on the
  stored arrays the share is 0)."""
  from lsi.geometry import layers
  g = golden('layers.npz')
  ti, tm, td = g['p_out_imgs'], g['p_out_masks'], g['p_out_dmaps']
  want_img = O.compose(ti, tm, td, soft=soft, min_disp=min_disp,
                       depth_softmax_temp=temp)
  want_disp = O.compose_depth(tm, td, bg_layer=False, min_disp=min_disp,
                              depth_softmax_temp=temp)
  masks = np.concatenate([tm, np.ones_like(tm[:1])], 0)
  dmaps = np.concatenate([np.maximum(td, 0), np.full_like(td[:1], min_disp)], 0)
  p = np.sort(O.soft_z_buffering(masks, dmaps, temp), axis=0)
  keep = ((p[-1] - p[-2]) >= 1e-4)[..., 0]
  if soft:                       # (a blend has no discrete choice)
    keep[:] = True
  print('left out: %d of %d pixels' % ((~keep).sum(), keep.size))
  assert keep.size == 640 and 1.0 - keep.mean() <= 0.01
  # L x B x ... -> B x (V = 1) x P = L
  bl = lambda x: T(x, dev).transpose(0, 1)
  per_b = lambda x: T(x, dev)[:, None, None]
  got = layers.render_planes(
      bl(g['p_imgs']).contiguous(), bl(g['p_masks']).contiguous(),
      per_b(g['p_k_s']), per_b(g['p_k_t']), per_b(g['p_rot']), per_b(g['p_t']),
      bl(g['p_n_hat'])[:, None], bl(g['p_a'])[:, None], (16, 20), soft=soft,
      min_disp=min_disp, depth_softmax_temp=temp)
  img, disp = [x[:, 0].cpu().numpy() for x in got]
  print('max |img err| %.3g  max |disp err| %.3g' %
        (np.abs(img - want_img)[keep].max(), np.abs(disp - want_disp)[keep].max()))
  np.testing.assert_allclose(img[keep], want_img[keep], rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(disp[keep], want_disp[keep], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# 2. against the op route, exactly
# ---------------------------------------------------------------------------
def _worlds(seed, n_obj_max, h, w, nb):
  from lsi.data import synthetic_planes as sp
  gen = sp.WorldGenerator(h=h, w=w, n_obj_max=n_obj_max,
                          n_obj_min=min(1, n_obj_max), seed=seed)
  rs = np.random.RandomState(seed + 100)
  worlds = [gen.forward() for _ in range(nb)]
  views = [[(np.eye(3), np.zeros((3, 1))), sp.sample_views(1, rs)[0]]
           for _ in range(nb)]
  return gen, worlds, views


def _op_route(dev, gen, worlds, views, h, w, nbox):
  """Renderer.render_planes / render_disps (fg) per world and view, and again
  with the object masks zeroed: four lists of B x V tensors."""
  from lsi.data import synthetic_planes as sp
  ren = sp.Renderer(gen.bs, h=h, w=w, device=dev)
  k = np.array([[w, 0, w / 2.0], [0, h, h / 2.0], [0, 0, 1.0]])
  ren.set_cameras(k, k)
  out = [[], [], [], []]
  for wd, vs in zip(worlds, views):
    room = np.copy(wd[6])
    room[nbox:] = 0
    for j, masks in ((0, wd[6]), (2, room)):
      ren.set_world(*(list(wd[:6]) + [masks]))
      out[j].append(torch.stack([ren.render_planes(r, t) for r, t in vs]))
      out[j + 1].append(torch.stack([ren.render_disps(r, t)[0] for r, t in vs]))
  return [torch.stack(o) for o in out]


def _fused(dev, gen, worlds, views, h, w, nbox, **kw):
  from lsi.geometry import layers
  from lsi.nnutils import helpers
  t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
  st = lambda i: t32(np.stack([wd[i] for wd in worlds]))
  rot_w2s, t_w2s, k_w, n_hat_w, a_w, imgs, masks = [st(i) for i in range(7)]
  rv = t32(np.stack([np.stack([v[0] for v in vs]) for vs in views]))[:, :, None]
  tv = t32(np.stack([np.stack([v[1] for v in vs]) for vs in views]))[:, :, None]
  k = t32(np.array([[w, 0, w / 2.0], [0, h, h / 2.0], [0, 0, 1.0]]))
  rot_w2t = helpers.seq_matmul(rv, rot_w2s[:, None])
  t_w2t = tv + helpers.seq_matmul(rv, t_w2s[:, None])
  kw.setdefault('min_disp', 0.2)
  kw.setdefault('depth_softmax_temp', 0.4)
  return layers.render_planes(imgs, masks, k_w[:, None], k[None, None, None],
                              rot_w2t, t_w2t, n_hat_w[:, None], a_w[:, None],
                              (h, w), n_box=nbox, **kw)


@pytest.mark.parametrize('seed,n_obj_max,hw,nb', [
    (0, 0, (128, 128), 1), (1, 2, (128, 128), 3), (2, 4, (256, 256), 1),
    (3, 4, (128, 256), 3), (0, 2, (128, 256), 1), (1, 4, (128, 128), 3),
    (2, 0, (256, 256), 3), (3, 2, (256, 256), 1)])
def test_equals_the_op_route(dev, seed, n_obj_max, hw, nb):
  """Both sides execute the same fp32 operation sequence on the same device:
  torch.equal on all four outputs."""
  h, w = hw
  gen, worlds, views = _worlds(seed, n_obj_max, h, w, nb)
  want = _op_route(dev, gen, worlds, views, h, w, gen.n_box_planes)
  got = _fused(dev, gen, worlds, views, h, w, gen.n_box_planes)
  for name, a, b in zip(('img', 'disp', 'img_room', 'disp_room'), got, want):
    assert a.shape == b.shape, name
    ndiff = int((a != b).sum())
    print('%s: %d of %d elements differ, max |diff| %.3g' %
          (name, ndiff, a.numel(), float((a - b).abs().max())))
    assert torch.equal(a, b), name
  assert float(got[0].min()) >= 0 and float(got[1].min()) >= 0.2


def test_soft_composition_equals_the_op_route(dev):
  from lsi.data import synthetic_planes as sp
  from lsi.geometry import layers
  h = w = 128
  gen, worlds, views = _worlds(4, 2, h, w, 2)
  got = _fused(dev, gen, worlds, views, h, w, gen.n_box_planes, soft=True,
               min_disp=1e-3, depth_softmax_temp=0.4)
  ren = sp.Renderer(gen.bs, h=h, w=w, device=dev)
  k = np.array([[w, 0, w / 2.0], [0, h, h / 2.0], [0, 0, 1.0]])
  ren.set_cameras(k, k)
  for b, (wd, vs) in enumerate(zip(worlds, views)):
    ren.set_world(*wd)
    for v, (r, t) in enumerate(vs):
      imgs, masks, dmaps, _, _ = ren._warp(r, t, ren.k_t)
      want = layers.compose(imgs, masks, dmaps, soft=True, min_disp=1e-3,
                            depth_softmax_temp=0.4)
      want_d = layers.compose_depth(masks, dmaps, bg_layer=False, min_disp=1e-3,
                                    depth_softmax_temp=0.4)
      assert torch.equal(got[0][b, v], want)
      assert torch.equal(got[1][b, v], want_d)


# ---------------------------------------------------------------------------
# 3. hostile homographies
# ---------------------------------------------------------------------------
def test_hostile_homographies(dev):
  """Planes behind the camera, q2 == 0, coordinates far outside the texture,
  NaN / Inf matrix entries: lsi_render_planes on explicit hom / dmat equals the
  op route (transform_pts -> divide_safe -> bilinear -> compose) on the same
  matrices; where nothing is hit the view is white at min_disp."""
  import ctypes
  from lsi import _C
  from lsi.geometry import homography, layers, sampling
  from lsi.nnutils import helpers
  rs = np.random.RandomState(17)
  nb, nv, npl, hs, ws, h, w = 2, 2, 6, 24, 40, 32, 64
  tex = T(rs.rand(nb, npl, hs, ws, 4), dev)
  tex[..., 3] = (tex[..., 3] > 0.3).float()
  hom = np.tile(np.array([ws / w, 0, 0, 0, hs / h, 0, 0, 0, 1], np.float32),
                (nb, nv, npl, 1))
  hom += 0.05 * rs.randn(*hom.shape).astype(np.float32) * (hom != 0)
  dmat = np.tile(np.array([0, 0, 0.4], np.float32), (nb, nv, npl, 1))
  dmat[..., 2] += 0.1 * rs.rand(nb, nv, npl).astype(np.float32)
  hom[0, 0, 0, 6:] = [0, 0, -1]                 # behind the camera
  dmat[0, 0, 0] = [0, 0, -0.5]
  hom[0, 0, 1, 6:] = [0, 0, 0]                  # q2 == 0 everywhere
  hom[0, 1, 0, 6:] = [1, 0, -32.5]              # q2 == 0 on the column x = 32.5
  hom[0, 1, 1, :3] = [1e6, 0, 1e9]              # far outside
  hom[0, 1, 2, 2] = np.nan
  hom[1, 0, 0, 0] = np.inf
  hom[1, 0, 1, 8] = -np.inf
  hom[1, 0, 2, 4] = 1e38                        # overflows to Inf
  dmat[1, 0, 3] = [np.nan, 0, 0.3]
  dmat[1, 0, 4] = [0, np.inf, 0.3]
  hom[1, 1, :, :] = 0                           # a view that sees nothing
  hom[1, 1, :, 2] = -1e4
  hom[1, 1, :, 8] = 1
  hom_t, dmat_t = T(hom, dev), T(dmat, dev)
  min_disp, temp = 0.2, 0.4
  d = _C.LsiSceneDesc()
  d.B, d.V, d.P, d.Hs, d.Ws, d.H, d.W = nb, nv, npl, hs, ws, h, w
  d.n_box, d.soft, d.min_disp, d.temp, d.outputs = 3, 0, min_disp, temp, 15
  outs = [torch.empty((nb, nv, h, w, c), device=dev) for c in (3, 1, 3, 1)]
  rc = _C.lib().lsi_render_planes(ctypes.byref(d), _C.ptr(tex), _C.ptr(hom_t),
                                  _C.ptr(dmat_t), *([_C.ptr(o) for o in outs] +
                                                    [_C.stream_ptr(dev)]))
  assert rc == 0
  pc = helpers.pixel_coords(1, h, w, device=dev)[0]
  for b in range(nb):
    for v in range(nv):
      pcs = pc[None].expand(npl, h, w, 3)
      q = helpers.transform_pts(pcs, hom_t[b, v].reshape(npl, 3, 3))
      uv = homography.normalize_homogeneous(q)
      both = sampling.bilinear_wrapper(tex[b], uv)
      prod = dmat_t[b, v].reshape(npl, 1, 1, 3) * pcs
      dm = (prod[..., 0:1] + prod[..., 1:2]) + prod[..., 2:3]
      for j, zero_from in ((0, npl), (2, 3)):
        masks = both[..., 3:4].clone()
        masks[zero_from:] = 0
        want = layers.compose(both[..., :3], masks, dm, soft=False,
                              min_disp=min_disp, depth_softmax_temp=temp)
        want_d = layers.compose_depth(masks, dm, bg_layer=False, min_disp=min_disp,
                                      depth_softmax_temp=temp)
        # (NaN == NaN for this comparison: a NaN disparity is the op route's too)
        assert torch.equal(torch.nan_to_num(outs[j][b, v], nan=-7.0),
                           torch.nan_to_num(want, nan=-7.0)), (b, v, j)
        assert torch.equal(torch.nan_to_num(outs[j + 1][b, v], nan=-7.0),
                           torch.nan_to_num(want_d, nan=-7.0)), (b, v, j)
  # the view whose planes are all sampled far outside their textures
  assert bool((outs[0][1, 1] == 1).all()) and bool((outs[1][1, 1] == min_disp).all())
  assert bool((outs[2][1, 1] == 1).all()) and bool((outs[3][1, 1] == min_disp).all())


# ---------------------------------------------------------------------------
# 4. / 5. the batched loader
# ---------------------------------------------------------------------------
def _opts(h=128, w=128, gt=False, ds=1, n_obj_max=4):
  return types.SimpleNamespace(img_height=h, img_width=w, n_obj_max=n_obj_max,
                               n_obj_min=1, n_box_planes=5, synth_ds_factor=ds,
                               synth_dl_eval_data=gt)


@pytest.mark.parametrize('gt', [False, True])
@pytest.mark.parametrize('ds', [1, 2])
def test_loader_parity_with_host_textures(dev, gt, ds):
  from lsi.data import synthetic_planes as sp
  seed = 11 + ds
  want = sp.DataLoader(_opts(gt=gt, ds=ds), device=dev, seed=seed).forward(3)
  got = sp.BatchedDataLoader(_opts(gt=gt, ds=ds), device=dev, seed=seed,
                             textures='host').forward(3)
  assert len(got) == len(want) == (14 if gt else 6)
  for i, (a, b) in enumerate(zip(got, want)):
    assert a.shape == b.shape and a.device == b.device and a.dtype == b.dtype, i
    diff = float((a - b).abs().max())
    print('output %d: max |diff| %.3g' % (i, diff))
    if ds == 1 or i in (2, 3, 4, 5, 6, 7):
      assert torch.equal(a, b), i
    else:
      assert diff <= 1e-6, (i, diff)


def test_device_textures(dev):
  from lsi.data import synthetic_planes as sp
  from lsi.geometry import ldi
  from lsi.nnutils import helpers
  ld = sp.BatchedDataLoader(_opts(gt=True), device=dev, seed=3)
  worlds = [ld.generator.forward(raster=False) for _ in range(4)]
  tex = ld._device_textures([wd[5] for wd in worlds], [wd[6] for wd in worlds])
  assert tex.shape == (4, 9, 128, 128, 4)
  assert float(tex[..., :3].min()) >= 0 and float(tex[..., :3].max()) <= 1
  assert bool((tex[:, :5, :, :, 3] == 1).all())            # box planes: opaque
  for b, wd in enumerate(worlds):
    n_obj = wd[5]
    assert 1 <= n_obj <= 4
    assert bool((tex[b, 5 + n_obj:, :, :, 3] == 0).all())  # unused slots
    sil = tex[b, 5:5 + n_obj, :, :, 3]
    assert bool(((sil == 0) | (sil == 1)).all())
    frac = sil.mean(dim=(1, 2))
    assert float(frac.min()) > 0.1 and float(frac.max()) < 0.95
  # same seed -> same batch, another seed -> another batch
  a = sp.BatchedDataLoader(_opts(gt=True, n_obj_max=2), device=dev, seed=5).forward(2)
  b = sp.BatchedDataLoader(_opts(gt=True, n_obj_max=2), device=dev, seed=5).forward(2)
  c = sp.BatchedDataLoader(_opts(gt=True, n_obj_max=2), device=dev, seed=6).forward(2)
  assert len(a) == 14
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  assert not torch.equal(a[0], c[0]) and not torch.equal(a[4], c[4])
  # the geometric check of test_scene_generator_views_are_geometrically_consistent
  src, trg, k_s, k_t, rot, t = a[:6]
  d_src = a[8]
  assert src.shape == (2, 128, 128, 3) and d_src.shape == (2, 128, 128, 1)
  assert float(src.min()) >= 0 and float(src.max()) <= 1 + 1e-5
  assert float(d_src.min()) >= 0.2 - 1e-6 and float(d_src.max()) < 0.6
  img, wts = ldi.forward_splat([src[None], None, d_src[None]],
                               helpers.pixel_coords(2, 128, 128), k_s, k_t, rot,
                               t, trg_downsampling=1, bg_layer_disp=1e-3,
                               max_disp=1.0, zbuf_scale=50)
  covered = (wts[0, ..., 0] > 1e-6).float()
  err = ((img[0] - trg).abs().mean(dim=3) * covered).sum() / covered.sum()
  print('coverage %.3f, mean error %.4f' % (float(covered.mean()), float(err)))
  assert float(covered.mean()) > 0.25
  assert float(err) < 0.06, float(err)


# ---------------------------------------------------------------------------
# 6. the scripts
# ---------------------------------------------------------------------------
def test_train_step_on_batched_planes(tmp_path, dev):
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  argv = ['--dataset', 'synthetic', '--synth_scene', 'planes_batched',
          '--debug_synth_texture', 'true', '--batch_size', '2', '--n_layers', '2',
          '--img_height', '128', '--img_width', '128', '--n_obj_max', '2',
          '--checkpoint_dir', str(tmp_path), '--log_freq', '1000000',
          '--save_latest_freq', '1000000', '--checkpoint_freq', '1000000']
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(argv))
  tr = script.Trainer(opts)
  tr.setup()
  from lsi.data import synthetic_planes
  assert isinstance(tr.data_loader, synthetic_planes.BatchedDataLoader)
  total, scalars = tr.train_step()
  assert tr.gt_disps is not None and tr.gt_disps[0].shape == (2, 2, 128, 128, 1)
  assert np.isfinite(float(total))
  assert len(scalars) == 6
  for k, v in scalars.items():
    assert np.isfinite(float(v)), k


def test_eval_script_on_batched_planes(tmp_path, dev):
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  argv = ['--dataset', 'synthetic', '--synth_scene', 'planes_batched',
          '--batch_size', '1', '--n_layers', '2', '--img_height', '128',
          '--img_width', '128', '--n_obj_max', '2', '--num_eval_iter', '2',
          '--random_weights', 'true', '--checkpoint_dir', str(tmp_path)]
  opts = script.apply_dataset_overrides(ev.build_parser().parse_args(argv))
  opts.debug_synth_texture = False
  opts.synth_dl_eval_data = True
  tester = ev.Tester(opts)
  results = tester.test()
  for k in ('compose_splat_loss', 'compose_splat_loss_disocc', 'depth_splat_loss',
            'fg_tex_error', 'fg_disp_error', 'bg_tex_error', 'bg_disp_error', 'psnr'):
    assert k in results and np.isfinite(results[k]), k
  assert 0 <= results['compose_splat_loss'] <= 1
  text = open(os.path.join(opts.checkpoint_dir, 'results', 'results.txt')).read()
  assert 'fg_disp_error' in text
