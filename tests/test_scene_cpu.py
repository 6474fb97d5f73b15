"""The fused scene renderer's boundary, without a GPU: lsi_render_planes is
exported, bound and refuses bad arguments before any launch; the Python layer
has no CPU path; the batched plane homographies are the per-instance ones bit
for bit; the scripts know --synth_scene planes_batched."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

from conftest import PKG


def test_render_planes_is_exported_and_bound(built_lib):
  from lsi import _C
  assert hasattr(ctypes.CDLL(built_lib), 'lsi_render_planes')
  assert 'lsi_render_planes' in _C.SIGNATURES
  # 9 int32 + 2 float + uint32, as include/lsi_hip.h lays LsiSceneDesc out
  assert ctypes.sizeof(_C.LsiSceneDesc) == 48
  assert _C.LsiSceneDesc.n_box.offset == 28
  assert _C.LsiSceneDesc.min_disp.offset == 36
  assert _C.LsiSceneDesc.outputs.offset == 44
  assert (_C.LSI_SCENE_IMG, _C.LSI_SCENE_DISP, _C.LSI_SCENE_IMG_ROOM,
          _C.LSI_SCENE_DISP_ROOM) == (1, 2, 4, 8)


def _desc(_C, **kw):
  d = _C.LsiSceneDesc()
  d.B, d.V, d.P, d.Hs, d.Ws, d.H, d.W = 2, 2, 3, 8, 8, 8, 8
  d.n_box, d.soft, d.min_disp, d.temp, d.outputs = 2, 0, 0.2, 0.4, 1 | 2
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_render_planes_argument_errors_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  null = None
  some = 256           # a non-NULL, 16-byte aligned address that is never read:
  # every call below is refused by the argument checks
  call = lambda d, tex=some, hom=some, dmat=some, img=some, disp=some, ir=null, dr=null: \
      lib.lsi_render_planes(ctypes.byref(d) if d is not None else None, tex, hom,
                            dmat, img, disp, ir, dr, None)
  assert call(None) == -2                                   # LSI_ENULL
  for bad in (dict(P=0), dict(P=17), dict(B=0), dict(V=-1), dict(Hs=0), dict(W=0),
              dict(n_box=4), dict(n_box=-1), dict(outputs=0), dict(outputs=16),
              dict(Hs=8192, Ws=8192)):
    assert call(_desc(_C, **bad)) == -1, bad                # LSI_EINVAL
  d = _desc(_C)
  assert call(d, tex=null) == -2
  assert call(d, hom=null) == -2
  assert call(d, dmat=null) == -2
  assert call(d, img=null) == -2                            # wanted, not given
  assert call(d, disp=null) == -2
  assert call(_desc(_C, outputs=1 | 4), disp=null) == -2    # img_room wanted
  assert call(_desc(_C, outputs=8), img=null, disp=null) == -2
  assert call(d, tex=260) == -1                             # RGBA texel alignment


def test_no_cpu_path(built_lib):
  from lsi.data import synthetic_planes
  from lsi.geometry import layers
  b, p = 1, 2
  eye = torch.eye(3).expand(b, 1, p, 3, 3)
  args = [torch.rand(b, p, 8, 8, 3), torch.rand(b, p, 8, 8, 1), eye, eye, eye,
          torch.zeros(b, 1, p, 3, 1), torch.tensor([0., 0., 1.]).expand(b, 1, p, 1, 3),
          -torch.ones(b, 1, p, 1, 1), (8, 8)]
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    layers.render_planes(*args)
  opts = types.SimpleNamespace(img_height=32, img_width=32)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    synthetic_planes.BatchedDataLoader(opts, device='cpu')
  with pytest.raises(ValueError, match='textures'):
    synthetic_planes.BatchedDataLoader(opts, device='cpu', textures='disk')


def test_batched_homographies_equal_the_per_instance_ones():
  """layers.plane_homographies over B x V x P planes at once against the
  matrices Renderer._warp computes view by view (its own lines, CPU torch on
  both sides): the same bits."""
  from lsi.data import synthetic_planes as sp
  from lsi.geometry import homography, layers
  from lsi.nnutils import helpers
  h = w = 64
  gen = sp.WorldGenerator(h=h, w=w, n_obj_max=3, seed=5)
  rs = np.random.RandomState(6)
  t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
  k_np = np.array([[w, 0, w / 2.0], [0, h, h / 2.0], [0, 0, 1.0]])
  worlds = [gen.forward(raster=False) for _ in range(3)]
  views = [[(np.eye(3), np.zeros((3, 1))), sp.sample_views(1, rs)[0]]
           for _ in worlds]
  n = gen.bs
  want_h, want_d = [], []
  for wd, vs in zip(worlds, views):
    rot_w2s, t_w2s, k_w, n_hat_w, a_w = [t32(x) for x in wd[:5]]
    for rot_v, trans_v in vs:                      # Renderer._warp
      rv = t32(rot_v)[None].expand(n, 3, 3)
      tv = t32(trans_v)[None].expand(n, 3, 1)
      rot_w2t = helpers.seq_matmul(rv, rot_w2s)
      t_w2t = tv + helpers.seq_matmul(rv, t_w2s)
      k_vv = t32(k_np)[None].expand(n, 3, 3)
      want_h.append(homography.inv_homography(k_w, k_vv, rot_w2t, t_w2t, n_hat_w,
                                              a_w))
      want_d.append(homography.inv_homography_dmat(k_vv, rot_w2t, t_w2t, n_hat_w,
                                                   a_w))
  st = lambda i: t32(np.stack([wd[i] for wd in worlds]))
  rot_w2s, t_w2s, k_w, n_hat_w, a_w = [st(i) for i in range(5)]
  rv = t32(np.stack([np.stack([v[0] for v in vs]) for vs in views]))[:, :, None]
  tv = t32(np.stack([np.stack([v[1] for v in vs]) for vs in views]))[:, :, None]
  rot_w2t = helpers.seq_matmul(rv, rot_w2s[:, None])
  t_w2t = tv + helpers.seq_matmul(rv, t_w2s[:, None])
  hom, dmat = layers.plane_homographies(
      k_w[:, None], t32(k_np)[None, None, None], rot_w2t, t_w2t, n_hat_w[:, None],
      a_w[:, None])
  assert hom.shape == (3, 2, n, 3, 3) and dmat.shape == (3, 2, n, 1, 3)
  assert torch.equal(hom.reshape(6, n, 3, 3), torch.stack(want_h))
  assert torch.equal(dmat.reshape(6, n, 1, 3), torch.stack(want_d))
  assert bool(torch.isfinite(hom).all())


def test_world_geometry_without_textures_is_the_same_geometry():
  from lsi.data import synthetic_planes as sp
  g1 = sp.WorldGenerator(h=32, w=48, seed=9)
  g2 = sp.WorldGenerator(h=32, w=48, seed=9)
  for _ in range(4):
    full, geo = g1.forward(), g2.forward(raster=False)
    assert all(np.array_equal(x, y) for x, y in zip(full[:5], geo[:5]))
    n_obj, sil = geo[5], geo[6]
    assert len(sil) == n_obj
    # objects: the slots whose mask is not empty
    assert int((full[6][5:].reshape(4, -1).max(axis=1) > 0).sum()) == n_obj


def test_scripts_know_planes_batched():
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  p = script.build_parser()
  assert p.parse_args([]).synth_scene == 'pairs'
  assert p.parse_args(['--synth_scene', 'planes_batched']).synth_scene == 'planes_batched'
  assert p.parse_args(['--synth_scene', 'planes']).synth_scene == 'planes'
  assert ev.build_parser().parse_args(
      ['--synth_scene', 'planes_batched']).synth_scene == 'planes_batched'
