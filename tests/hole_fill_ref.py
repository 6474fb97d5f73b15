"""float32 NumPy restatement of the push-pull hole filler (csrc/lsi_fill.hip,
DESIGN.md 4.22): every operation is one float32 NumPy operation in the order of
the definition, so the kernel is compared with it bit for bit."""
import numpy as np

CONF, SPLAT = 0, 1
F = np.float32


def level0(img, w, mode=CONF, conf_min=1e-3, bg_value=1.0, bg_wt=0.0):
  """(p N x H x W x C, c N x H x W) of level 0."""
  img, w = np.asarray(img, F), np.asarray(w, F)
  with np.errstate(all='ignore'):
    if mode == CONF:
      c = np.where(w > 0, np.minimum(w, F(1)), F(0)).astype(F)
      p = img * c[..., None]
    else:
      c = np.where(w > F(bg_wt), (w - F(bg_wt)) / w, F(0)).astype(F)
      p = img - ((F(1) - c) * F(bg_value))[..., None]
    c = np.where(c < F(conf_min), F(0), c).astype(F)
    p = np.where((c == 0)[..., None], F(0), p).astype(F)
  return p, c


def push(v):
  """One push of N x H x W x K sums (the confidence is the last channel)."""
  n, h, w, k = v.shape
  pad = np.zeros((n, 2 * ((h + 1) // 2), 2 * ((w + 1) // 2), k), F)
  pad[:, :h, :w] = v
  with np.errstate(all='ignore'):
    s = ((pad[:, 0::2, 0::2] + pad[:, 0::2, 1::2]) +
         (pad[:, 1::2, 0::2] + pad[:, 1::2, 1::2]))
    sc = s[..., -1:]
    over = sc > 1
    out = np.where(over, s / np.where(over, sc, F(1)), s).astype(F)
    out[..., -1:] = np.where(over, F(1), sc)
  return out


def upsample(f, h, w):
  """The 2 x bilinear up-sample of N x Hu x Wu x C to N x h x w x C."""
  hu, wu = f.shape[1:3]
  y, x = np.arange(h), np.arange(w)
  cy, cx = y >> 1, x >> 1
  ny = np.clip(cy + np.where(y & 1, 1, -1), 0, hu - 1)
  nx = np.clip(cx + np.where(x & 1, 1, -1), 0, wu - 1)
  g = lambda iy, ix: f[:, iy][:, :, ix]
  with np.errstate(all='ignore'):
    return ((F(9) * g(cy, cx) + F(3) * g(cy, nx)) +
            (F(3) * g(ny, cx) + g(ny, nx))) * F(0.0625)


def fill(img, w, mode=CONF, conf_min=1e-3, bg_value=1.0, bg_wt=0.0):
  """F_0: N x H x W x C float32."""
  p, c = level0(img, w, mode, conf_min, bg_value, bg_wt)
  levels = [np.concatenate([p, c[..., None]], axis=-1)]
  while levels[-1].shape[1:3] != (1, 1):
    levels.append(push(levels[-1]))
  top = levels[-1]
  with np.errstate(all='ignore'):
    pos = top[..., -1:] > 0
    f = np.where(pos, top[..., :-1] / np.where(pos, top[..., -1:], F(1)),
                 F(bg_value)).astype(F)
    for v in levels[-2::-1]:
      u = upsample(f, v.shape[1], v.shape[2])
      f = (v[..., :-1] + (F(1) - v[..., -1:]) * u).astype(F)
  return f


def splat_canvas(fg, cover, bg_wt, bg_value=1.0, scale=1.0):
  """(img, wts) as forward_splat leaves them for a foreground `fg` N x H x W x C
  that reached a pixel with weight cover * scale over the canvas."""
  lw = (np.asarray(cover, F) * F(scale)).astype(F)
  wts = (lw + F(bg_wt)).astype(F)
  img = ((np.asarray(fg, F) * lw[..., None] + F(bg_wt) * F(bg_value)) / wts[..., None]).astype(F)
  return img, wts
