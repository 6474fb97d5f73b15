"""Host side of the convolution routes: the TF 'SAME' geometry every route
shares, and the fp32 kernels' refusal of batch-norm sums."""
import pytest
import torch

SIZES = list(range(1, 21)) + [256, 768]


def test_same_geometry_is_the_expression_the_routes_inlined():
  from lsi.nnutils import _hip_conv, nets
  for stride in (1, 2):
    for k in range(1, 8):
      for n in SIZES:
        assert nets._same_pad(n, k, stride)[0] == _hip_conv.same_geometry(n, n, k, stride)[2]
      for h in SIZES:
        for w in SIZES:
          oh, ow = -(-h // stride), -(-w // stride)
          pad_t = max((oh - 1) * stride + k - h, 0) // 2
          pad_l = max((ow - 1) * stride + k - w, 0) // 2
          assert _hip_conv.same_geometry(h, w, k, stride) == (oh, ow, pad_t, pad_l)
          assert nets._same_pad(h, k, stride)[0] == pad_t
          assert nets._same_pad(w, k, stride)[0] == pad_l


def test_fp32_kernels_refuse_batch_norm_sums(monkeypatch):
  """Only the bf16 epilogue leaves batch-norm sums: asking the fp32 precision for
  them is an error -- raised before the library is touched -- not ignored."""
  from lsi import _C
  from lsi.nnutils import _hip_conv

  def no_library():
    raise AssertionError('the library was called')
  monkeypatch.setattr(_C, 'lib', no_library)
  x = torch.zeros((2, 32, 4, 4)).contiguous(memory_format=torch.channels_last)
  wt = torch.zeros((32, 32, 3, 3))
  wt_t = torch.zeros((32, 32, 4, 4))
  with pytest.raises(ValueError):
    _hip_conv.conv2d(x, wt, 1, 1, 1, 4, 4, bn_groups=1, precision=_hip_conv.F32)
  with pytest.raises(ValueError):
    _hip_conv.conv2d_cat(x, x, torch.zeros((32, 64, 3, 3)), 1, 1, 1, 4, 4, bn_groups=1,
                         precision=_hip_conv.F32)
  with pytest.raises(ValueError):
    _hip_conv.conv_transpose2d(x, wt_t, 2, 1, bn_groups=1, precision=_hip_conv.F32)
