"""The launch ledger: which convolution entries of the library one training pass
of the U-Net and the LDI heads calls, in order, and with which options -- against
tests/conv_routes_expected.json, recorded before the bf16 and fp32 bindings were
folded into one.  Route order, the batch-norm groups handed to the kernels, the
two-tensor (skip connection) launches and the weight-gradient routes all show in
it.

  python tests/test_conv_routes_gpu.py [out.json]     records the file anew

Only public names and _C.lib are used, so the module runs on either side of a
change to the binding."""
import contextlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, 'tests', 'conv_routes_expected.json')

# name -> (batch, bf16 autocast, batch-norm groups, WGRAD_MIN_PIXELS or None, F32_CONV)
CONFIGS = {
    'bf16': (2, True, 1, None, False),
    'bf16_groups2': (4, True, 2, None, False),
    'bf16_row_ring': (2, True, 1, 0, False),
    'fp32_own': (2, False, 1, None, True),
    'fp32_library': (2, False, 1, None, False),
}
H, W = 128, 256   # the smallest image seven stride-2 levels take: a 1 x 2 bottleneck


class _Ledger(object):
  """Stands in for the loaded library: every lsi_conv* entry called is noted."""

  def __init__(self, lib):
    self._lib = lib
    self._fns = {}
    self.log = None

  def __getattr__(self, name):
    fn = self._fns.get(name)
    if fn is None:
      fn = self._fns[name] = self._wrap(name, getattr(self._lib, name))
    return fn

  def _wrap(self, name, fn):
    if not name.startswith('lsi_conv'):
      return fn
    run = name.endswith('_run')

    def call(*args):
      if self.log is not None:
        if run:
          io = args[2]._obj     # (ctypes.byref(LsiConvIO))
          self.log.append([name, int(args[1]), bool(io.x2), bool(io.out2), int(io.groups)])
        else:
          self.log.append([name])
      return fn(*args)
    return call


def _model(dev):
  from lsi.nnutils import nets
  torch.manual_seed(11)
  unet = nets.encoder_decoder_unet(nl_diff_enc_dec=3)
  heads = nets.ldi_predictor(unet.out_channels, n_layers=2, n_layerwise_steps=3,
                             skip_channels=unet.skip_channels)
  model = torch.nn.ModuleList([unet, heads]).to(dev).to(memory_format=torch.channels_last)
  return nets.own_kernel_param_layouts(model)


def _pass(model, img, bf16, groups):
  from lsi.nnutils import nets
  model.zero_grad(set_to_none=True)
  unet, heads = model
  cast = torch.autocast('cuda', dtype=torch.bfloat16) if bf16 else contextlib.nullcontext()
  with cast, nets.bn_groups(groups):
    _, feat, skips, _ = unet(img)
    tex, _, disps = heads(feat, skips, disp_scale=0.4)
  loss = (tex.float() ** 2).mean() + disps.float().mean()
  loss.backward()
  return tex, disps


def run_config(name, dev, patch):
  """One warm-up pass (packs made, geometry queries cached), then the recorded
  one.  `patch(obj, attr, value)`: monkeypatch.setattr or its like.
  -> (ledger, {tensor name: tensor} of the outputs and parameter gradients)."""
  from lsi import _C
  from lsi.nnutils import _hip_conv, nets
  batch, bf16, groups, wgrad_min, f32 = CONFIGS[name]
  patch(nets, 'F32_CONV', f32)
  if wgrad_min is not None:
    patch(_hip_conv, 'WGRAD_MIN_PIXELS', wgrad_min)
  ledger = _Ledger(_C.lib())
  patch(_C, 'lib', lambda: ledger)
  model = _model(dev)
  g = torch.Generator().manual_seed(5)
  img = torch.rand((batch, H, W, 3), generator=g).to(dev)
  _pass(model, img, bf16, groups)
  ledger.log = []
  tex, disps = _pass(model, img, bf16, groups)
  log, ledger.log = ledger.log, None
  torch.cuda.synchronize()
  out = {'tex': tex.detach(), 'disps': disps.detach()}
  for pname, p in model.named_parameters():
    if p.grad is not None:
      out['grad.' + pname] = p.grad.detach()
  return log, out


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_launch_ledger(name, dev, monkeypatch):
  with open(EXPECTED) as f:
    want = json.load(f)[name]
  log, _ = run_config(name, dev, monkeypatch.setattr)
  if name == 'fp32_library':
    assert log == []
  else:
    assert any(e[0].endswith('_run') and e[2] for e in log)   # (a two-tensor forward ran)
  assert len(log) == len(want), (len(log), len(want))
  for i, (got, exp) in enumerate(zip(log, want)):
    assert got == exp, (i, got, exp)


def _record(path):
  sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
  dev = torch.device('cuda:0')
  logs = {}
  for name in sorted(CONFIGS):
    undo = []

    def patch(obj, attr, value):
      undo.append((obj, attr, getattr(obj, attr)))
      setattr(obj, attr, value)
    try:
      logs[name], _ = run_config(name, dev, patch)
    finally:
      for obj, attr, value in reversed(undo):
        setattr(obj, attr, value)
  with open(path, 'w') as f:
    f.write('{\n')
    for i, name in enumerate(sorted(logs)):
      f.write(' %s: [\n' % json.dumps(name))
      f.write(',\n'.join('  ' + json.dumps(e) for e in logs[name]))
      f.write('\n ]%s\n' % (',' if i + 1 < len(logs) else ''))
    f.write('}\n')
  print('wrote %s: %s' % (path, {k: len(v) for k, v in logs.items()}))


if __name__ == '__main__':
  _record(sys.argv[1] if len(sys.argv) > 1 else EXPECTED)
