"""tools/conv_host_parity.py: a sha256 of every output of the implicit-GEMM
convolutions (bf16 and fp32) on seeded inputs, for the CONV, CONVT and
two-tensor cases of tests/test_conv_f32_gpu.py: both directions of every
descriptor (mode 0: its forward; mode 1: its data gradient = a transposed
convolution's forward), each with and without the split workspace, and the
weight gradient in both weight layouts.  Two builds whose listings agree compute
the same bits (LSI_HIP_LIB=<name> selects liblsi_hip_<name>.so); the batch-norm
sums are not asked for (float atomics: they do not repeat).

  python tools/conv_host_parity.py > new.txt
  LSI_HIP_LIB=parent python tools/conv_host_parity.py > parent.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'layered-scene-inference_amd'), os.path.join(ROOT, 'tests')):
  sys.path.insert(0, _p)
import torch  # noqa: E402
import test_conv_f32_gpu as cases  # noqa: E402
from lsi.nnutils import _hip_conv  # noqa: E402

dev = torch.device('cuda:0')


def sha(t):
  torch.cuda.synchronize()
  return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def descriptors():
  """(name, descriptor, channels of the first of two input tensors or 0)"""
  for n, h, w, cin, cout, k, s in cases.CONV:
    oh, ow, pt, pl = _hip_conv.same_geometry(h, w, k, s)
    yield ('conv %dx%dx%d %d->%d k%d s%d' % (n, h, w, cin, cout, k, s),
           _hip_conv._conv_desc(n, h, w, cin, oh, ow, cout, k, k, s, pt, pl), 0)
  for n, h, w, cin, cout in cases.CONVT:
    yield ('convt %dx%dx%d %d->%d' % (n, h, w, cin, cout),
           _hip_conv._conv_desc(n, 2 * h, 2 * w, cout, h, w, cin, 4, 4, 2, 1, 1), 0)
  for n, h, w, c1, c2, cout in cases.CAT:
    yield ('cat %dx%dx%d %d+%d->%d' % (n, h, w, c1, c2, cout),
           _hip_conv._conv_desc(n, h, w, c1 + c2, h, w, cout, 3, 3, 1, 1, 1), c1)


def main():
  for p, pname in ((_hip_conv.BF16, 'bf16'), (_hip_conv.F32, 'fp32')):
    for name, d, c1 in descriptors():
      g = torch.Generator().manual_seed(d.N + d.H * d.W + d.Cin + d.Cout)
      cl = lambda *shape: torch.randn(shape, generator=g).to(dev).to(p.dtype).contiguous(
          memory_format=torch.channels_last)
      x, gy = cl(d.N, d.Cin, d.H, d.W), cl(d.N, d.Cout, d.OH, d.OW)
      wt = (torch.randn((d.Cout, d.Cin, d.KH, d.KW), generator=g) * 0.05).to(dev)
      x1, x2 = (x[:, :c1].contiguous(memory_format=torch.channels_last),
                x[:, c1:].contiguous(memory_format=torch.channels_last)) if c1 else (x, None)
      out = lambda c, h, w: _hip_conv._empty_cl(d.N, c, h, w, dev, p.dtype)
      for split in (True, False):
        _hip_conv.SPLITK = split
        tag = 'split' if split else 'unsplit'
        y = _hip_conv._run(p, d, 0, wt, x1, out(d.Cout, d.OH, d.OW), x2=x2, c1=c1)
        print('%s %s fwd %s %s' % (pname, name, tag, sha(y)))
        if c1:
          g1, g2 = out(c1, d.H, d.W), out(d.Cin - c1, d.H, d.W)
          _hip_conv._run(p, d, 1, wt, gy, g1, out2=g2, c1=c1)
          print('%s %s dgrad %s %s %s' % (pname, name, tag, sha(g1), sha(g2)))
        else:
          gx = _hip_conv._run(p, d, 1, wt, gy, out(d.Cin, d.H, d.W))
          print('%s %s dgrad %s %s' % (pname, name, tag, sha(gx)))
      if _hip_conv.wgrad_bytes(p, d) == 0:
        print('%s %s wgrad: not taken' % (pname, name))
        continue
      for layout, w in (('contiguous', wt),
                        ('channels_last', wt.contiguous(memory_format=torch.channels_last))):
        gw = _hip_conv._wgrad(p, d, x1, gy, w, x2)
        # (the gradient's memory, in the layout it was written in)
        mem = gw.permute(0, 2, 3, 1) if layout == 'channels_last' else gw
        print('%s %s wgrad %s %s' % (pname, name, layout, sha(mem)))


if __name__ == '__main__':
  main()
