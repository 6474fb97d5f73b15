"""The disparity post-filters restated in NumPy (int64 throughout) from the
definition in DESIGN.md section 4.18: what csrc/lsi_disp_filter.hip is held to
bit for bit.  The median sorts the nine shifted planes; the components come from
a breadth-first search over an explicit queue -- no union-find, no tiles.
`components_scipy` is a second, independent statement through
scipy.sparse.csgraph."""
import collections

import numpy as np

ABSENT = 1 << 40          # sorts behind every value


def median3(img):
  """H x W int64 -> H x W int64."""
  h, w = img.shape
  pad = np.zeros((h + 2, w + 2), np.int64)          # outside: absent, like a hole
  pad[1:-1, 1:-1] = img
  planes = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], -1)
  n = (planes != 0).sum(-1)
  ordered = np.sort(np.where(planes != 0, planes, ABSENT), axis=-1)
  pick = np.clip((n - 1) // 2, 0, 8)
  med = np.take_along_axis(ordered, pick[..., None], -1)[..., 0]
  return np.where(img != 0, med, 0)


def links(img, rng):
  """(right, down): right[y, x] says (y, x) -- (y, x + 1) are linked, down[y, x]
  says (y, x) -- (y + 1, x)."""
  h, w = img.shape
  right = np.zeros((h, w), bool)
  down = np.zeros((h, w), bool)
  a, b = img[:, :-1], img[:, 1:]
  right[:, :-1] = (a != 0) & (b != 0) & (np.abs(a - b) <= rng)
  a, b = img[:-1], img[1:]
  down[:-1] = (a != 0) & (b != 0) & (np.abs(a - b) <= rng)
  return right, down


def component_sizes(img, rng):
  """H x W int64: the pixel count of each valid pixel's component, 0 at holes."""
  h, w = img.shape
  right, down = links(img, rng)
  size = np.zeros((h, w), np.int64)
  seen = img == 0
  for y0 in range(h):
    for x0 in range(w):
      if seen[y0, x0]:
        continue
      seen[y0, x0] = True
      members = [(y0, x0)]
      queue = collections.deque(members)
      while queue:
        y, x = queue.popleft()
        for ny, nx, ok in ((y, x + 1, right[y, x]), (y + 1, x, down[y, x]),
                           (y, x - 1, x > 0 and right[y, x - 1]),
                           (y - 1, x, y > 0 and down[y - 1, x])):
          if ok and not seen[ny, nx]:
            seen[ny, nx] = True
            members.append((ny, nx))
            queue.append((ny, nx))
      for y, x in members:
        size[y, x] = len(members)
  return size


def component_sizes_scipy(img, rng):
  """The same through scipy.sparse.csgraph.connected_components on the link
  graph."""
  from scipy import sparse
  from scipy.sparse import csgraph
  h, w = img.shape
  right, down = links(img, rng)
  idx = np.arange(h * w).reshape(h, w)
  src = np.concatenate([idx[right], idx[down]])
  dst = np.concatenate([idx[right] + 1, idx[down] + w])
  graph = sparse.coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(h * w, h * w))
  _, label = csgraph.connected_components(graph, directed=False)
  count = np.bincount(label, minlength=h * w)
  return np.where(img != 0, count[label].reshape(h, w), 0)


def speckle(img, speckle_size, rng, sizes=component_sizes):
  size = sizes(img, rng)
  return np.where((img != 0) & (size <= speckle_size), 0, img)


def filter_image(img, median=0, speckle_size=0, speckle_range=256, sizes=component_sizes):
  img = np.asarray(img).astype(np.int64)
  assert img.ndim == 2 and median in (0, 3)
  if median == 3:
    img = median3(img)
  if speckle_size > 0:
    img = speckle(img, speckle_size, speckle_range, sizes)
  return img


def filter_batch(disp, median=0, speckle_size=0, speckle_range=256, sizes=component_sizes):
  """B x H x W (or H x W) uint16 -> the same shape, uint16."""
  disp = np.asarray(disp)
  assert disp.dtype == np.uint16
  if disp.ndim == 2:
    return filter_image(disp, median, speckle_size, speckle_range, sizes).astype(np.uint16)
  return np.stack([filter_image(d, median, speckle_size, speckle_range, sizes)
                   for d in disp]).astype(np.uint16)


# -- patterns ---------------------------------------------------------------------
def serpentine(h, w, value=512):
  """A one-pixel-wide path: every even row whole, the odd rows one pixel that
  joins alternate ends.  Returns (map, path length)."""
  img = np.zeros((h, w), np.uint16)
  img[0::2] = value
  for i, y in enumerate(range(1, h - 1, 2)):      # (an odd last row joins nothing)
    img[y, w - 1 if i % 2 == 0 else 0] = value
  return img, int((img != 0).sum())


def random_map(seed, shape, speckle_range, valid=0.6):
  """Values from 4 levels spaced speckle_range +- 1 apart, `valid` of them set."""
  rs = np.random.RandomState(seed)
  base = 300
  levels = np.array([base, base + speckle_range - 1, base + 2 * speckle_range,
                     base + 3 * speckle_range - 1], np.int64)   # steps r - 1, r + 1, r - 1
  img = levels[rs.randint(0, 4, shape)]
  img[rs.rand(*shape) >= valid] = 0
  return img.astype(np.uint16)
