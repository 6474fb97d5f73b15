"""The SSIM view-synthesis loss and metric, the parts that need no GPU: the two
restatements of tests/ssim_ref.py agree, the host entry lsi_ssim_window gives
the weights of the definition, the device entries refuse bad arguments before
any launch, header / binding / exports agree, and the Python surface exists
(no CPU path, three trainer flags)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import ssim_ref

NEW = ('lsi_ssim_window', 'lsi_ssim_loss_fwd', 'lsi_ssim_loss_bwd', 'lsi_eval_ssim')
EINVAL, ENULL, EWORKSPACE = -1, -2, -3     # include/lsi_hip.h


@pytest.mark.parametrize('win', [3, 5])
def test_the_two_restatements_agree(win):
  g = torch.Generator().manual_seed(3)
  recons = torch.rand((2, 1, 9, 11, 3), dtype=torch.float64, generator=g)
  target = torch.rand((1, 18, 22, 3), dtype=torch.float64, generator=g)
  for sigma in (1.5, 0.0):
    ops = ssim_ref.dssim_maps(recons, target, 1, 1, win, sigma).numpy()
    direct = ssim_ref.dssim_direct(recons.numpy(), target.numpy(), 1, 1, win, sigma)
    assert ops.shape == direct.shape == (2, 1, 9 - 2 - win + 1, 11 - 2 - win + 1)
    assert np.abs(ops - direct).max() <= 1e-12


def _window(lib, win, sigma):
  out = (ctypes.c_float * 16)(*([7.0] * 16))
  rc = lib.lsi_ssim_window(win, sigma, ctypes.cast(out, ctypes.c_void_p))
  return rc, np.array(out[:], np.float32)


def test_window_weights(built_lib):
  from lsi import _C
  lib = _C.lib()
  for win in (3, 5, 7, 9, 11):
    for sigma in (1.5, 0.8, 4.0):
      rc, w = _window(lib, win, sigma)
      assert rc == 0
      assert np.all(w[win:] == 7.0)                 # win weights, no more
      w = w[:win]
      assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 1e-6
      assert np.array_equal(w, w[::-1])
      assert np.array_equal(w, ssim_ref.window64(win, sigma).astype(np.float32))
    for sigma in (0.0, -1.0):                       # the box
      rc, w = _window(lib, win, sigma)
      assert rc == 0
      assert np.array_equal(w[:win], np.full(win, np.float32(1.0 / win)))
  for win in (2, 4, 13, 0, -3, 1):
    assert _window(lib, win, 1.5)[0] == EINVAL
  assert lib.lsi_ssim_window(7, 1.5, None) == ENULL
  # the Python accessor
  from lsi.loss import _hip
  assert _hip.ssim_window(7, 1.5) == [float(v) for v in _window(lib, 7, 1.5)[1][:7]]
  with pytest.raises(ValueError, match='odd'):
    _hip.ssim_window(4, 1.5)


def _desc(_C, **kw):
  d = _C.LsiSsimDesc()
  d.nl, d.B, d.Ht, d.Wt, d.H, d.W = 2, 1, 16, 24, 32, 48
  d.x_min, d.y_min, d.win = 2, 1, 7
  d.sigma, d.c1, d.c2 = 1.5, 1e-4, 9e-4
  d.t_sb, d.t_sy, d.t_sx, d.t_sc = 32 * 48 * 3, 48 * 3, 3, 1
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_argument_errors_are_reported_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  big = 1 << 30
  p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused

  def calls(d, a=p, b=p, c=p, ws=p, nbytes=big):
    r = ctypes.byref(d) if d is not None else None
    return (lib.lsi_ssim_loss_fwd(r, a, b, c, ws, nbytes, None),
            lib.lsi_ssim_loss_bwd(r, a, b, c, ws, None),
            lib.lsi_eval_ssim(r, a, b, c, ws, nbytes, None))

  assert calls(None) == (EINVAL,) * 3
  for bad in (dict(win=4), dict(win=13), dict(win=1), dict(win=-7),
              dict(y_min=5),              # 16 - 10 = 6 rows < 7
              dict(x_min=9),              # 24 - 18 = 6 columns < 7
              dict(H=33), dict(W=50),     # non-integer factors
              dict(nl=0), dict(B=-1), dict(x_min=-1)):
    assert calls(_desc(_C, **bad)) == (EINVAL,) * 3, bad
  # a bad descriptor wins over a NULL pointer, a NULL pointer over the workspace
  assert calls(_desc(_C, win=4), a=None, nbytes=0) == (EINVAL,) * 3
  d = _desc(_C)
  for null in ('a', 'b', 'c', 'ws'):
    assert calls(d, **{null: None}, nbytes=0) == (ENULL,) * 3, null
  short = int(lib.lsi_loss_workspace_bytes()) - 1
  # (the backward takes no workspace: with these arguments it would launch)
  r = ctypes.byref(d)
  assert lib.lsi_ssim_loss_fwd(r, p, p, p, p, short, None) == EWORKSPACE
  assert lib.lsi_eval_ssim(r, p, p, p, p, short, None) == EWORKSPACE
  # exactly one window is a valid grid: the refusal is the NULL pointer's
  one = _desc(_C, Ht=7, Wt=7, H=7, W=7, x_min=0, y_min=0)
  assert calls(one, a=None) == (ENULL,) * 3


def test_header_binding_and_exports_agree(built_lib):
  from lsi import _C
  with open(os.path.join(ROOT, 'include', 'lsi_hip.h')) as f:
    h = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
  assert re.search(r'#define LSI_VERSION 100\b', h)
  handle = ctypes.CDLL(built_lib)
  n_params = {}
  for n in NEW:
    m = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % n, h)
    assert m, n
    n_params[n] = len(m.group(1).split(','))
    assert n in _C.SIGNATURES, n
    res, args = _C.SIGNATURES[n]
    assert res is ctypes.c_int and len(args) == n_params[n], n
    assert hasattr(handle, n), n
  assert n_params == {'lsi_ssim_window': 3, 'lsi_ssim_loss_fwd': 7,
                      'lsi_ssim_loss_bwd': 6, 'lsi_eval_ssim': 7}
  # the struct: 9 int32, 3 float, 4 int64 -- no padding
  m = re.search(r'typedef struct LsiSsimDesc \{(.*?)\} LsiSsimDesc;', h, flags=re.S)
  fields = re.findall(r'\b([A-Za-z_0-9]+)\s*[,;]', m.group(1))
  assert fields == [f[0] for f in _C.LsiSsimDesc._fields_]
  assert ctypes.sizeof(_C.LsiSsimDesc) == 9 * 4 + 3 * 4 + 4 * 8
  assert _C.LsiSsimDesc.t_sb.offset == 48


def test_no_cpu_path(built_lib):
  from lsi.loss import loss
  from lsi.nnutils import eval_metrics
  recons, target = torch.rand(1, 1, 16, 16, 3), torch.rand(1, 16, 16, 3)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    loss.ssim_view_synthesis_loss(recons, target)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    eval_metrics.MetricAccumulator('cpu').add_ssim(recons, target, 0.05)


def test_accumulator_has_no_ssim_key_before_add_ssim(built_lib):
  from lsi.nnutils import _hip_eval, eval_metrics
  acc = eval_metrics.MetricAccumulator('cpu')
  assert 'ssim' not in acc.sums() and 'ssim' not in acc.results()
  assert _hip_eval.SLOT_COUNT == 16 and len(_hip_eval.SLOTS) == 16
  assert 'ssim' not in _hip_eval.METRICS
  acc.acc_ssim = torch.tensor([3.0, 4.0], dtype=torch.float64)
  assert acc.sums()['ssim'] == (3.0, 4.0) and acc.results()['ssim'] == 0.75
  acc.reset()
  assert acc.sums()['ssim'] == (0.0, 0.0) and 'ssim' not in acc.results()


def test_flags_and_their_defaults():
  sys.path.insert(0, PKG)
  import ldi_enc_dec
  import ldi_pred_eval
  o = ldi_enc_dec.build_parser().parse_args([])
  assert (o.ssim_wt, o.ssim_win, o.ssim_sigma) == (0.0, 7, 1.5)
  o = ldi_enc_dec.build_parser().parse_args(
      ['--ssim_wt', '0.85', '--ssim_win', '11', '--ssim_sigma', '0'])
  assert (o.ssim_wt, o.ssim_win, o.ssim_sigma) == (0.85, 11, 0.0)
  e = ldi_pred_eval.build_parser().parse_args([])
  assert e.eval_ssim is False and e.ssim_wt == 0.0
  assert ldi_pred_eval.build_parser().parse_args(['--eval_ssim', 'true']).eval_ssim
