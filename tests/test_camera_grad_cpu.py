"""The camera gradient of forward_splat, the parts that need no GPU: the
projection matrices stay differentiable (and bit-equal to the host fast path)
when a camera requires grad, and the C ABI of the matrix gradient
(lsi_splat_bwd_m / lsi_splat_bwd_both_m, LSI_GRAD_M) checks its arguments
before any device call."""
import ctypes

import pytest
import torch


def _cams(b=3, seed=0, dtype=torch.float32):
  g = torch.Generator().manual_seed(seed)
  k = torch.tensor([[120.0, 0.0, 64.0], [0.0, 118.0, 32.0], [0.0, 0.0, 1.0]])
  k_s = k.repeat(b, 1, 1) + 0.5 * torch.rand((b, 3, 3), generator=g) * torch.tensor(
      [[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
  k_t = k.repeat(b, 1, 1)
  a = 0.05 * torch.rand((b, 3), generator=g)
  rot = torch.linalg.matrix_exp(torch.stack([
      torch.stack([torch.zeros(b), -a[:, 2], a[:, 1]], -1),
      torch.stack([a[:, 2], torch.zeros(b), -a[:, 0]], -1),
      torch.stack([-a[:, 1], a[:, 0], torch.zeros(b)], -1)], 1))
  t = torch.rand((b, 3, 1), generator=g) - 0.5
  return [x.to(dtype) for x in (k_s, k_t, rot, t)]


@pytest.mark.parametrize('inverse', [False, True])
def test_projection_matrix_requires_grad_and_is_bit_equal(built_lib, inverse):
  from lsi.geometry import projection
  fn = (projection.inverse_projection_matrix if inverse else
        projection.forward_projection_matrix)
  cams = _cams()
  fast = projection._host_matrices(*cams, inverse)   # lsi_projection_matrices
  assert fast is not None and not fast.requires_grad
  for i in range(4):
    args = [c.clone().requires_grad_(j == i) for j, c in enumerate(cams)]
    m = fn(*args)
    assert m.requires_grad, i
    assert torch.equal(m.detach(), fast), i
    m.sum().backward()
    assert args[i].grad is not None and bool(torch.isfinite(args[i].grad).all())
  with torch.no_grad():     # grad mode off: the fast path, as before
    m = fn(*[c.clone().requires_grad_(True) for c in cams])
  assert not m.requires_grad and torch.equal(m, fast)


@pytest.mark.parametrize('inverse', [False, True])
def test_projection_matrix_gradcheck_fp64(inverse):
  from lsi.geometry import projection
  fn = (projection.inverse_projection_matrix if inverse else
        projection.forward_projection_matrix)
  cams = [c.clone().requires_grad_(True) for c in _cams(b=2, dtype=torch.float64)]
  assert torch.autograd.gradcheck(fn, cams, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_grad_m_symbols_exported(built_lib):
  from lsi import _C
  handle = ctypes.CDLL(built_lib)
  for n in ('lsi_splat_bwd_m', 'lsi_splat_bwd_both_m'):
    assert hasattr(handle, n)
    assert n in _C.SIGNATURES
  assert _C.LSI_GRAD_M == 64


def _desc(_C, flags):
  d = _C.LsiSplatDesc()
  d.L, d.B, d.H, d.W, d.Ht, d.Wt = 2, 2, 16, 64, 8, 32
  d.tex_sl, d.tex_sb, d.tex_sy, d.tex_sx, d.tex_sc = 2 * 16 * 64 * 3, 16 * 64 * 3, 64 * 3, 3, 1
  d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx = 2 * 16 * 64, 16 * 64, 64, 1
  d.trg_downsampling, d.max_disp, d.zbuf_scale, d.bg_wt = 0.5, 0.4, 50.0, 1e-11
  d.flags = flags
  return d


def test_grad_m_argument_checks_before_any_device_call(built_lib):
  """Only host-side checks are reached: every call below is refused before a
  pointer is dereferenced or a kernel launched (the pointers are dummies)."""
  from lsi import _C
  lib = _C.lib()
  p = [ctypes.c_void_p(0x1000 + 0x100 * i) for i in range(20)]
  for base in (_C.LSI_COMPOSE, 0):
    d = _desc(_C, base | _C.LSI_GRAD_M)
    dd = _desc(_C, base)
    # the entries without _m refuse the flag
    if base:
      assert lib.lsi_splat_bwd(ctypes.byref(d), *p[:12], 1 << 30, None) == -1
    else:
      assert lib.lsi_splat_bwd_both(ctypes.byref(d), *p[:16], 1 << 30, None) == -1
    # the flag without g_M: LSI_ENULL; g_M without the flag: LSI_EINVAL
    if base:
      assert lib.lsi_splat_bwd_m(ctypes.byref(d), *p[:11], None, p[12], 1 << 30,
                                 None) == -2
      assert lib.lsi_splat_bwd_m(ctypes.byref(dd), *p[:11], p[11], p[12], 1 << 30,
                                 None) == -1
    else:
      assert lib.lsi_splat_bwd_both_m(ctypes.byref(d), *p[:15], None, p[16],
                                      1 << 30, None) == -2
      assert lib.lsi_splat_bwd_both_m(ctypes.byref(dd), *p[:15], p[15], p[16],
                                      1 << 30, None) == -1
    # the partials come on top of the gradient canvas
    need = lib.lsi_splat_bwd_workspace_bytes(ctypes.byref(d))
    need0 = lib.lsi_splat_bwd_workspace_bytes(ctypes.byref(dd))
    assert need >= need0 + 16 * 4 * (16 * 2 * 2), (need, need0)
  # the composed-output descriptor is refused by the _both_m entry as by _both
  d = _desc(_C, _C.LSI_COMPOSE | _C.LSI_GRAD_M)
  assert lib.lsi_splat_bwd_both_m(ctypes.byref(d), *p[:17], 1 << 30, None) == -1
