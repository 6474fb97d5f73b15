"""Prefetching KITTI loader: PNG decode on a pool of threads running ahead of
the step, the AREA resize on the host (in the worker) or on the device (one
launch of csrc/lsi_image.hip per output tensor of a batch).

`PrefetchLoader` wraps data.DataLoader and returns what its forward() returns,
for the same samples in the same order: the indices of every batch -- prefetched
ones included -- are drawn from the wrapped loader's own RNG by the consuming
thread, in the sequence the synchronous loader draws them.

  workers   threads that decode (Pillow releases the GIL while it inflates and
            unfilters a PNG), clamped to [1, 16] and divided by the world size:
            the ranks of one command stay within 16 threads together.  Never
            sized from the machine's CPU count.
  resize    'host':   data._load_image in the worker; values bit for bit those
                      of the synchronous loader.
            'device': the worker writes the decoded uint8 pixels and one
                      descriptor per image straight into a pinned staging
                      buffer; forward() issues one non-blocking upload and the
                      resize launches on the current stream and returns device
                      tensors for images and disparities, NumPy arrays for the
                      cameras (data.pair_cameras, untouched).
  prefetch_depth  batches decoded ahead of the one being returned.

With the wrapped loader's --kitti_augment on (augment.py), the parameters of
every pair are drawn in _schedule, in batch order, from the wrapped loader's
_aug_rng: the results do not depend on the thread count, the depth or timing.
The host route runs augment.augment_area_resize in the workers; on the device
route the workers write pixels as before and forward() fills the augmented
descriptors and the tone tables into the same staging buffer: still one upload
and one launch (lsi_augment_resize_u8) per output tensor.

With the wrapped loader's --kitti_gt_everywhere on, its pixel disparities and
Velodyne scans go through the same pool, behind the images of their batch.  The
host route runs augment.sample_disparity_px / velodyne.load_scan in the workers:
the synchronous loader's batch, bit for bit.  On the device route a worker
decodes a 16-bit map to uint16 into the staging buffer and reads a scan's bytes
into it; forward() fills the map descriptors and issues one
lsi_augment_sample_u16 launch for the 2 bs maps behind the one upload, and
returns device tensors for the maps (the two halves of that launch's output) and
for velo_pts (NaN-padded on the device), NumPy arrays for velo_n and velo_mats.

A staging buffer goes back to the pool only when an event recorded behind its
upload has completed.  A decode error is raised from the forward() that owns the
sample and names the file.  close() stops the workers; a collected loader or an
exiting interpreter does not wait on more than the decodes already running.
"""
import collections
import os
import threading
import time
import weakref
from concurrent import futures

import numpy as np

from lsi import _C
from lsi.data.kitti import data as kitti_data

MAX_THREADS = 16
# the records of include/lsi_hip.h, as the binding lays them out
DESC_DTYPE = np.dtype(_C.LsiImageDesc)
AUG_DESC_DTYPE = np.dtype(_C.LsiAugmentDesc)
AUG_FLIP = _C.LSI_AUG_FLIP
TABLE_BYTES = 3 * 256


def pool_size(workers, world_size=1):
  """Threads of one rank: the option clamped to [1, 16], shared by the ranks."""
  return max(1, min(MAX_THREADS, int(workers)) // max(1, int(world_size)))


def _round16(n):
  return (int(n) + 15) // 16 * 16


def decode_u8(path, nc):
  """data.decode_png's pixels as uint8, first nc channels: H x W x nc.  16-bit
  PNGs keep their high byte."""
  from PIL import Image  # pylint: disable=g-import-not-at-top
  with Image.open(path) as im:
    if im.mode in ('I;16', 'I;16B', 'I;16L', 'I'):
      arr = (np.asarray(im).astype(np.int64) >> 8).astype(np.uint8)
    elif im.mode in ('L', 'P', '1', 'LA'):
      arr = np.asarray(im.convert('L'), np.uint8)
    else:
      arr = np.asarray(im.convert('RGB'), np.uint8)
  if arr.ndim == 2:
    arr = arr[:, :, None]
  if arr.shape[2] < nc:
    raise ValueError('%s has %d channels, %d needed' % (path, arr.shape[2], nc))
  return arr[:, :, :nc]


def area_resize_u8(packed, desc_host, desc_dev, n, h, w, nc, out=None):
  """lsi_area_resize_u8 on the current stream: `packed` a uint8 device tensor
  (16-byte aligned, a multiple of 16 long), desc_host a DESC_DTYPE array of n
  records, desc_dev the address of their device copy.  Returns float32
  [n, h, w, nc] on packed's device."""
  import torch  # pylint: disable=g-import-not-at-top
  if not packed.is_cuda:
    raise RuntimeError('the device AREA resize needs a ROCm GPU (got device %s); '
                       'there is no CPU fallback' % packed.device)
  if packed.dtype != torch.uint8 or not packed.is_contiguous():
    raise RuntimeError('packed must be a contiguous uint8 tensor')
  desc_host = np.ascontiguousarray(desc_host, DESC_DTYPE)
  if desc_host.shape != (n,):
    raise ValueError('%d descriptors for %d images' % (desc_host.size, n))
  if out is None:
    out = torch.empty((n, h, w, nc), dtype=torch.float32, device=packed.device)
  _C.check(_C.lib().lsi_area_resize_u8(
      n, desc_host.ctypes.data, int(desc_dev), packed.data_ptr(), packed.numel(),
      h, w, nc, out.data_ptr(), _C.stream_ptr(packed.device)),
           'lsi_area_resize_u8')
  return out


def augment_desc(images_hwc, offsets, windows=None, flips=None, tables=None,
                 gains=None):
  """AUG_DESC_DTYPE records of n images: shapes (H, W, C), byte offsets, and
  per image a window (default: the whole image), a flip bit, a table index
  (default -1: identity) and C gains (default 1)."""
  n = len(images_hwc)
  desc = np.zeros(n, AUG_DESC_DTYPE)
  for m, (h, w, c) in enumerate(images_hwc):
    y0, x0, ch, cw = windows[m] if windows is not None else (0, 0, h, w)
    g = np.ones(3, np.float32)
    if gains is not None:
      g[:c] = np.asarray(gains[m], np.float32).reshape(-1)[:c]
    desc[m] = (offsets[m], h, w, c, AUG_FLIP if flips is not None and flips[m] else 0,
               y0, x0, ch, cw, tables[m] if tables is not None else -1, 0, g, 0)
  return desc


def augment_resize_u8(packed, desc_host, desc_dev, n, h, w, nc, tables_offset=0,
                      n_tables=0, out=None):
  """lsi_augment_resize_u8 on the current stream: area_resize_u8 with
  AUG_DESC_DTYPE records; the n_tables tone tables (uint8[nc][256] each) lie
  in `packed` from byte tables_offset.  Returns float32 [n, h, w, nc]."""
  import torch  # pylint: disable=g-import-not-at-top
  if not packed.is_cuda:
    raise RuntimeError('the device AREA resize needs a ROCm GPU (got device %s); '
                       'there is no CPU fallback' % packed.device)
  if packed.dtype != torch.uint8 or not packed.is_contiguous():
    raise RuntimeError('packed must be a contiguous uint8 tensor')
  desc_host = np.ascontiguousarray(desc_host, AUG_DESC_DTYPE)
  if desc_host.shape != (n,):
    raise ValueError('%d descriptors for %d images' % (desc_host.size, n))
  if out is None:
    out = torch.empty((n, h, w, nc), dtype=torch.float32, device=packed.device)
  _C.check(_C.lib().lsi_augment_resize_u8(
      n, desc_host.ctypes.data, int(desc_dev), packed.data_ptr(), packed.numel(),
      int(tables_offset), int(n_tables), h, w, nc, out.data_ptr(),
      _C.stream_ptr(packed.device)), 'lsi_augment_resize_u8')
  return out


def augment_sample_u16(packed, desc_host, desc_dev, n, h, w, out=None):
  """lsi_augment_sample_u16 on the current stream: nearest-neighbour samples of
  the n 16-bit disparity maps in `packed` through the windows and flips of
  their AUG_DESC_DTYPE records (C = 1, table -1), in pixels of the h x w image
  (augment.sample_disparity_px's bits).  Returns float32 [n, h, w, 1]."""
  import torch  # pylint: disable=g-import-not-at-top
  if not packed.is_cuda:
    raise RuntimeError('the device disparity sampling needs a ROCm GPU (got device '
                       '%s); there is no CPU fallback' % packed.device)
  if packed.dtype != torch.uint8 or not packed.is_contiguous():
    raise RuntimeError('packed must be a contiguous uint8 tensor')
  desc_host = np.ascontiguousarray(desc_host, AUG_DESC_DTYPE)
  if desc_host.shape != (n,):
    raise ValueError('%d descriptors for %d maps' % (desc_host.size, n))
  if out is None:
    out = torch.empty((n, h, w, 1), dtype=torch.float32, device=packed.device)
  _C.check(_C.lib().lsi_augment_sample_u16(
      n, desc_host.ctypes.data, int(desc_dev), packed.data_ptr(), packed.numel(),
      h, w, out.data_ptr(), _C.stream_ptr(packed.device)), 'lsi_augment_sample_u16')
  return out


class _Staging(object):
  """One pinned buffer: [descriptors | pixel bytes], filled by the workers of
  one batch.  alloc() hands out 16-byte aligned ranges; a range that does not
  fit is refused and the image travels as its own array (the batch is then
  re-packed into a larger buffer).  An augmenting loader's buffer holds
  AUG_DESC_DTYPE records and, behind them, n_tables tone tables; a loader that
  emits pixel disparities adds n_maps AUG_DESC_DTYPE records for the 16-bit
  maps, whose pixels (and the bytes of Velodyne scans) lie among the images':
  [descriptors | tables | map descriptors | pixel bytes]."""

  def __init__(self, n_desc, capacity, n_tables=0, dtype=DESC_DTYPE, n_maps=0):
    import torch  # pylint: disable=g-import-not-at-top
    self.tables_offset = _round16(n_desc * dtype.itemsize)
    self.n_tables = n_tables
    self.maps_offset = self.tables_offset + _round16(n_tables * TABLE_BYTES)
    self.header = self.maps_offset + _round16(n_maps * AUG_DESC_DTYPE.itemsize)
    self.capacity = _round16(capacity)
    self.tensor = torch.empty(self.header + self.capacity + 16, dtype=torch.uint8,
                              pin_memory=True)
    self.bytes = self.tensor.numpy()
    self.desc = self.bytes[:n_desc * dtype.itemsize].view(dtype)
    self.tables = self.bytes[self.tables_offset:self.tables_offset +
                             n_tables * TABLE_BYTES].reshape(n_tables, 3, 256)
    self.map_desc = self.bytes[self.maps_offset:self.maps_offset +
                               n_maps * AUG_DESC_DTYPE.itemsize].view(AUG_DESC_DTYPE)
    self.lock = threading.Lock()
    self.reset()

  def reset(self):
    self.used = self.header
    self.wanted = self.header

  def alloc(self, nbytes):
    nbytes = _round16(nbytes)
    with self.lock:
      self.wanted += nbytes
      if self.used + nbytes > self.header + self.capacity:
        return None
      off = self.used
      self.used += nbytes
      return off


def _host_task(stop, path, h, w, nc):
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  return kitti_data._load_image(path, h, w, nc)  # pylint: disable=protected-access


def _host_augment_task(stop, path, h, w, aug):
  from lsi.data.kitti import augment  # pylint: disable=g-import-not-at-top
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  arr = decode_u8(path, 3)
  table, gains = augment.image_params(aug, 3)
  return augment.augment_area_resize(
      arr, augment.window(aug, arr.shape[0], arr.shape[1]), aug.flip, table, gains,
      h, w), arr.shape


def _set_image(desc, slot, off, h, w, nc):
  """The image fields of record `slot` (either descriptor layout)."""
  rec = desc[slot:slot + 1]
  rec['offset'], rec['H'], rec['W'], rec['C'], rec['reserved'] = off, h, w, nc, 0


def _device_task(stop, path, nc, staging, slot):
  """Decodes `path` into `staging` and fills descriptor `slot`.  Returns
  (original shape, None) or, when the buffer is full, (shape, pixel array)."""
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  arr = decode_u8(path, nc)
  h, w = arr.shape[:2]
  if h * w > _C.LSI_IMAGE_MAX_PIXELS:
    raise ValueError('%s: %d x %d pixels exceed the resize kernel\'s bound' %
                     (path, h, w))
  off = staging.alloc(arr.size)
  if off is None:
    return (h, w, nc), np.ascontiguousarray(arr)
  staging.bytes[off:off + arr.size].reshape(arr.shape)[...] = arr
  _set_image(staging.desc, slot, off, h, w, nc)
  return (h, w, nc), None


def _host_px_task(stop, path, h, w, aug):
  """The h x w x 1 pixel disparities of one map, as the synchronous loader
  makes them."""
  from lsi.data.kitti import augment  # pylint: disable=g-import-not-at-top
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  if aug is None:
    return kitti_data.load_disparity_px(path, h, w)
  raw = kitti_data.decode_u16(path)
  return augment.sample_disparity_px(
      raw, augment.window(aug, raw.shape[0], raw.shape[1]), aug.flip, h, w)


def _scan_path_points(path):
  """Points of the scan file, 0 for a missing one; the refusal of
  velodyne.load_scan for a length that is no multiple of a point."""
  if not os.path.exists(path):
    return 0
  size = os.path.getsize(path)
  if size % 16 != 0:
    raise ValueError('%s is no Velodyne scan: %d bytes is not a multiple of the '
                     '16 bytes of a point' % (path, size))
  return size // 16


def _host_scan_task(stop, path):
  from lsi.data.kitti import velodyne  # pylint: disable=g-import-not-at-top
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  if not _scan_path_points(path):
    return np.zeros((0, 4), np.float32)
  return velodyne.load_scan(path)


def _device_px_task(stop, path, staging, slot):
  """Decodes the 16-bit map `path` into `staging` as host-order uint16 and
  fills the image fields of map descriptor `slot`.  Returns (shape, None) or,
  when the buffer is full, (shape, uint16 array)."""
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  raw = kitti_data.decode_u16(path)
  h, w = raw.shape
  off = staging.alloc(raw.nbytes)
  if off is None:
    return (h, w, 1), np.ascontiguousarray(raw)
  staging.bytes[off:off + raw.nbytes].view(np.uint16).reshape(h, w)[...] = raw
  _set_image(staging.map_desc, slot, off, h, w, 1)
  return (h, w, 1), None


def _device_scan_task(stop, path, staging):
  """Reads the scan `path` into `staging`.  Returns (points, byte offset, None)
  or, when the buffer is full, (points, None, float32 [points, 4] array); a
  missing file is a scan of 0 points."""
  if stop.is_set():
    raise RuntimeError('the loader was closed')
  n = _scan_path_points(path)
  if n == 0:
    return 0, 0, None
  off = staging.alloc(16 * n)
  if off is None:
    from lsi.data.kitti import velodyne  # pylint: disable=g-import-not-at-top
    return n, None, velodyne.load_scan(path)[:n]
  with open(path, 'rb') as f:
    if f.readinto(memoryview(staging.bytes[off:off + 16 * n])) != 16 * n:
      raise ValueError('%s: the scan changed while it was read' % path)
  return n, off, None


def _named(path, err):
  """`err` if it names the file, else an error of its type's family that does."""
  if path in str(err):
    return err
  new = RuntimeError('cannot decode %s: %s: %s' % (path, type(err).__name__, err))
  new.__cause__ = err
  return new


def _shutdown(stop, pool):
  stop.set()
  pool.shutdown(wait=False, cancel_futures=True)


class PrefetchLoader(object):
  """data.DataLoader with its decodes running ahead on threads (module doc)."""

  def __init__(self, loader, workers=4, resize='host', prefetch_depth=2,
               device=None, world_size=1):
    if resize not in ('host', 'device'):
      raise ValueError("resize must be 'host' or 'device', got %r" % (resize,))
    # (a loader without the attribute -- any object but data.DataLoader -- is
    # refused as before)
    gt_everywhere = bool(getattr(loader, 'gt_everywhere', False))
    if getattr(loader, 'output_disparities_px', False) and not gt_everywhere:
      raise ValueError(
          'kitti_dl_disparities_px (the pixel disparities --eval_depth scores '
          'against) is served by the synchronous loader only: run with '
          '--data_workers 0 --kitti_resize host (or with --kitti_gt_everywhere '
          'true)')
    if getattr(loader, 'output_velodyne', False) and not gt_everywhere:
      raise ValueError(
          'kitti_dl_velodyne (the Velodyne scans --eval_depth scores against) is '
          'served by the synchronous loader only: run with --data_workers 0 '
          '--kitti_resize host (or with --kitti_gt_everywhere true)')
    self._gt_px = gt_everywhere and bool(getattr(loader, 'output_disparities_px', False))
    self._gt_velo = gt_everywhere and bool(getattr(loader, 'output_velodyne', False))
    self.loader = loader
    self.resize = resize
    self.depth = max(1, int(prefetch_depth))
    self.device = device
    if resize == 'device':
      import torch  # pylint: disable=g-import-not-at-top
      dev = torch.device(device if device is not None else 'cuda')
      if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError(
            "resize='device' runs the AREA resize as a HIP kernel and needs a "
            'ROCm GPU (got device %s); use resize=\'host\' on a CPU run' % dev)
      self.device = dev
    self.n_threads = pool_size(workers, world_size)
    self._stop = threading.Event()
    self._pool = futures.ThreadPoolExecutor(self.n_threads,
                                            thread_name_prefix='kitti-decode')
    self._finalizer = weakref.finalize(self, _shutdown, self._stop, self._pool)
    self._pending = collections.deque()   # scheduled batches, oldest first
    self._free, self._uploading = [], []  # staging buffers; (event, staging)
    self._capacity = 0
    self._bs = None
    self.src_image_names = []

  # the wrapped loader's state, where KittiBatches and callers look for it
  @property
  def _rng(self):
    return self.loader._rng  # pylint: disable=protected-access

  @_rng.setter
  def _rng(self, rng):
    if self._pending:
      raise RuntimeError('the RNG must be set before the first forward()')
    self.loader._rng = rng  # pylint: disable=protected-access

  @property
  def _aug_rng(self):
    return self.loader._aug_rng  # pylint: disable=protected-access

  @_aug_rng.setter
  def _aug_rng(self, rng):
    if self._pending:
      raise RuntimeError('the RNG must be set before the first forward()')
    self.loader._aug_rng = rng  # pylint: disable=protected-access

  @property
  def output_disparities(self):
    return self.loader.output_disparities

  def __getattr__(self, name):  # file lists, h, w, opts ... of the wrapped loader
    if name == 'loader':
      raise AttributeError(name)
    return getattr(self.loader, name)

  # -- staging buffers ----------------------------------------------------------
  def _acquire(self, n_desc, first_path):
    # a buffer is free once the event behind its upload has completed
    still = []
    for ev, st in self._uploading:
      if ev.query():
        self._free.append(st)
      else:
        still.append((ev, st))
    self._uploading = still
    if not self._free and len(self._uploading) > self.depth + 1:
      # the device is far behind: wait for the oldest upload, do not grow
      ev, st = self._uploading.pop(0)
      ev.synchronize()
      self._free.append(st)
    while self._free:
      st = self._free.pop()  # (one of another size or batch layout is dropped)
      if st.capacity >= self._capacity and st.desc.shape[0] == n_desc:
        st.reset()
        return st
    if not self._capacity:
      # a first guess from one file's header; a batch that does not fit is
      # re-packed and the next buffers are made larger
      from PIL import Image  # pylint: disable=g-import-not-at-top
      try:
        with Image.open(first_path) as im:
          self._capacity = _round16(im.size[0] * im.size[1] * 3) * n_desc
          if self._gt_px:  # two bytes per pixel of every map
            self._capacity += _round16(im.size[0] * im.size[1] * 2) * 2 * self._bs
      except Exception:  # pylint: disable=broad-except
        self._capacity = 1 << 20  # (the decode task reports the file)
    return self._new_staging(n_desc, self._capacity)

  def _new_staging(self, n_desc, capacity):
    n_maps = 2 * self._bs if self._gt_px else 0
    if getattr(self.loader, 'augment', None) is None:
      return _Staging(n_desc, capacity, n_maps=n_maps)
    # one tone table per pair: the two views share it
    return _Staging(n_desc, capacity, n_tables=n_desc // 2, dtype=AUG_DESC_DTYPE,
                    n_maps=n_maps)

  # -- scheduling -------------------------------------------------------------
  def _schedule(self, bs):
    ld = self.loader
    if ld.cam_calibration is None:
      ld.preload_calib_files()
    ids = [ld._next_index() for _ in range(bs)]  # pylint: disable=protected-access
    lists = [(ld.img_list_src, 3), (ld.img_list_trg, 3)]
    if ld.output_disparities:
      lists += [(ld.img_list_disp_src, 1), (ld.img_list_disp_trg, 1)]
    # descriptor / result order: per list, the bs samples
    paths = [(lst[i], nc) for lst, nc in lists for i in ids]
    staging = None
    augs = None
    if getattr(ld, 'augment', None) is not None:
      from lsi.data.kitti import augment  # pylint: disable=g-import-not-at-top
      augs = [augment.sample(ld._aug_rng, ld.augment)  # pylint: disable=protected-access
              for _ in ids]
    if augs is not None and self.resize == 'host':
      futs = [self._pool.submit(_host_augment_task, self._stop, p, ld.h, ld.w,
                                augs[n % bs]) for n, (p, _) in enumerate(paths)]
    elif self.resize == 'device':
      staging = self._acquire(len(paths), paths[0][0])
      futs = [self._pool.submit(_device_task, self._stop, p, nc, staging, slot)
              for slot, (p, nc) in enumerate(paths)]
    else:
      futs = [self._pool.submit(_host_task, self._stop, p, ld.h, ld.w, nc)
              for p, nc in paths]
    if self._gt_px or self._gt_velo:
      self._schedule_gt(ids, paths, futs, staging, augs)
    self._pending.append((ids, paths, futs, staging, augs))

  def _schedule_gt(self, ids, paths, futs, staging, augs):
    """--kitti_gt_everywhere: the tasks of the batch's 16-bit maps (source
    views, then target views) and scans, behind those of its images."""
    ld = self.loader
    bs = len(ids)
    device = self.resize == 'device'
    if self._gt_px:
      for slot, (lst, i) in enumerate(
          (lst, i) for lst in (ld.img_list_disp_src, ld.img_list_disp_trg) for i in ids):
        paths.append((lst[i], 'px'))
        if device:
          futs.append(self._pool.submit(_device_px_task, self._stop, lst[i], staging, slot))
        else:
          futs.append(self._pool.submit(_host_px_task, self._stop, lst[i], ld.h, ld.w,
                                        augs[slot % bs] if augs is not None else None))
    if self._gt_velo:
      for i in ids:
        paths.append((ld.scan_list[i], 'scan'))
        if device:
          futs.append(self._pool.submit(_device_scan_task, self._stop, ld.scan_list[i],
                                        staging))
        else:
          futs.append(self._pool.submit(_host_scan_task, self._stop, ld.scan_list[i]))

  def forward(self, bs):
    """The next batch of the wrapped loader's sequence (module doc)."""
    if self._stop.is_set():
      raise RuntimeError('the loader was closed')
    if self._bs is not None and bs != self._bs and self._pending:
      raise ValueError('batches of %d are already being prefetched; got bs=%d' %
                       (self._bs, bs))
    self._bs = bs
    while len(self._pending) < self.depth + 1:
      self._schedule(bs)
    ids, paths, futs, staging, augs = self._pending.popleft()
    ld = self.loader
    results, error = [], None
    for (path, _), fut in zip(paths, futs):  # every task of the batch ends here
      try:
        results.append(fut.result())
      except Exception as e:  # pylint: disable=broad-except
        results.append(None)
        if error is None:
          error = _named(path, e)
    self.src_image_names = [ld.img_list_src[i] for i in ids]
    ld.src_image_names = self.src_image_names
    if error is not None:
      if staging is not None:
        self._free.append(staging)  # never uploaded: free at once
      raise error
    gt = None
    if self._gt_px or self._gt_velo:
      # the tasks of _schedule_gt: 2 bs maps, then bs scans, behind the images
      n_img = len(paths) - (2 * bs if self._gt_px else 0) - (bs if self._gt_velo else 0)
      gt = results[n_img:]
      paths, results = paths[:n_img], results[:n_img]
    shapes = [r[0] if self.resize == 'device' else r[1] for r in results]
    if augs is None:
      cams = [kitti_data.pair_cameras(ld.cam_calibration[ld.seq_id_list[i]],
                                      shapes[j], shapes[bs + j], ld.h, ld.w)
              for j, i in enumerate(ids)]
    else:
      cams = [ld.augmented_cameras(augs[j], shapes[j], shapes[bs + j],
                                   ld.cam_calibration[ld.seq_id_list[i]])
              for j, i in enumerate(ids)]
    out_cams = [np.stack([c[k] for c in cams]) for k in range(4)]
    if self.resize == 'host':
      imgs = [np.stack([r[0] for r in results[g * bs:(g + 1) * bs]])
              for g in range(len(paths) // bs)]
      if gt is not None:
        imgs += self._host_gt(gt, ids, shapes, augs)
      return imgs[:2] + out_cams + imgs[2:]
    imgs = self._upload_and_resize(staging, results, bs, augs, gt)
    if self._gt_velo:  # (the matrices stay on the host, like the cameras)
      imgs.append(self._velo_mats(ids, shapes, augs))
    return imgs[:2] + out_cams + imgs[2:]

  def _velo_mats(self, ids, shapes, augs):
    bs = len(ids)
    return np.stack([self.loader.velodyne_matrices(
        i, shapes[j], shapes[bs + j], augs[j] if augs is not None else None)
                     for j, i in enumerate(ids)])

  def _host_gt(self, gt, ids, shapes, augs):
    """The synchronous loader's ground-truth outputs from the workers' results:
    [disp_px_s, disp_px_t][velo_pts, velo_n, velo_mats]."""
    bs = len(ids)
    out = []
    if self._gt_px:
      out += [np.stack(gt[:bs]), np.stack(gt[bs:2 * bs])]
      gt = gt[2 * bs:]
    if self._gt_velo:
      out += list(kitti_data.pad_scans(gt)) + [self._velo_mats(ids, shapes, augs)]
    return out

  def _fill_augment(self, staging, augs, bs):
    """The windows, flip bits, table indices and gains of the 2 bs images, and
    the tables themselves, into the staging buffer (pair j: slots j, bs + j)."""
    from lsi.data.kitti import augment  # pylint: disable=g-import-not-at-top
    desc = staging.desc
    for j, aug in enumerate(augs):
      table, gains = augment.image_params(aug, 3)
      if table is not None:
        staging.tables[j] = table
      for slot in (j, bs + j):
        rec = desc[slot:slot + 1]
        rec['y0'], rec['x0'], rec['ch'], rec['cw'] = augment.window(
            aug, int(desc['H'][slot]), int(desc['W'][slot]))
        rec['flags'] = AUG_FLIP if aug.flip else 0
        rec['table'] = j if table is not None else -1
        rec['gain'] = gains
        rec['reserved'] = rec['reserved2'] = 0

  def _fill_maps(self, staging, augs, bs):
    """The windows and flip bits of the 2 bs disparity maps, each window from
    the map's own shape (pair j: slots j, bs + j); no table, gains of 1."""
    from lsi.data.kitti import augment  # pylint: disable=g-import-not-at-top
    desc = staging.map_desc
    for slot in range(2 * bs):
      aug = augs[slot % bs] if augs is not None else None
      rec = desc[slot:slot + 1]
      h, w = int(desc['H'][slot]), int(desc['W'][slot])
      rec['y0'], rec['x0'], rec['ch'], rec['cw'] = (
          augment.window(aug, h, w) if aug is not None else (0, 0, h, w))
      rec['flags'] = AUG_FLIP if aug is not None and aug.flip else 0
      rec['table'], rec['gain'] = -1, 1.0
      rec['reserved'] = rec['reserved2'] = 0

  def _upload_and_resize(self, staging, results, bs, augs=None, gt=None):
    import torch  # pylint: disable=g-import-not-at-top
    ld = self.loader
    spilled = [(slot, r[1]) for slot, r in enumerate(results) if r[1] is not None]
    maps = gt[:2 * bs] if self._gt_px else []
    scans = list(gt[2 * bs if self._gt_px else 0:]) if self._gt_velo else []
    gt_spilled = any(r[-1] is not None for r in maps + scans)
    if spilled or gt_spilled:
      # the buffer was too small: a larger one takes the whole batch (and sets
      # the size of the buffers made from now on)
      self._capacity = _round16(staging.wanted - staging.header) * 5 // 4
      big = self._new_staging(staging.desc.shape[0], self._capacity)
      n_fit = staging.used
      big.bytes[big.header:n_fit] = staging.bytes[staging.header:n_fit]
      big.desc[...] = staging.desc
      big.used = n_fit
      for slot, arr in spilled:
        off = big.alloc(arr.size)
        big.bytes[off:off + arr.size].reshape(arr.shape)[...] = arr
        _set_image(big.desc, slot, off, arr.shape[0], arr.shape[1], arr.shape[2])
      big.map_desc[...] = staging.map_desc
      for slot, (_, arr) in enumerate(maps):
        if arr is not None:
          off = big.alloc(arr.nbytes)
          big.bytes[off:off + arr.nbytes].view(np.uint16).reshape(arr.shape)[...] = arr
          _set_image(big.map_desc, slot, off, arr.shape[0], arr.shape[1], 1)
      for k, (n, _, arr) in enumerate(scans):
        if arr is not None:
          off = big.alloc(arr.nbytes)
          big.bytes[off:off + arr.nbytes].view(np.float32).reshape(arr.shape)[...] = arr
          scans[k] = (n, off, None)
      staging = big
    if augs is not None:
      self._fill_augment(staging, augs, bs)
    if self._gt_px:
      self._fill_maps(staging, augs, bs)
    used = staging.used + 16  # the pad behind the last image
    with torch.cuda.device(self.device):
      packed = torch.empty(used, dtype=torch.uint8, device=self.device)
      packed.copy_(staging.tensor[:used], non_blocking=True)
      event = torch.cuda.Event()
      event.record()
      self._uploading.append((event, staging))
      out = []
      if augs is not None:  # (an augmenting loader emits the two images only)
        both = augment_resize_u8(packed, staging.desc, packed.data_ptr(), 2 * bs,
                                 ld.h, ld.w, 3, staging.tables_offset,
                                 staging.n_tables)
        out = [both[:bs], both[bs:]]
        if gt is None:
          return out
      else:
        for g, nc in enumerate((3, 1) if ld.output_disparities else (3,)):
          n = 2 * bs
          first = g * n
          both = area_resize_u8(
              packed, staging.desc[first:first + n],
              packed.data_ptr() + first * DESC_DTYPE.itemsize, n, ld.h, ld.w, nc)
          out += [both[:bs], both[bs:]]
      if self._gt_px:
        # one launch for the 2 bs maps, [source views; target views]: the halves
        # are views of one tensor, which the trainer takes whole
        both = augment_sample_u16(packed, staging.map_desc,
                                  packed.data_ptr() + staging.maps_offset, 2 * bs,
                                  ld.h, ld.w)
        out += [both[:bs], both[bs:]]
      if self._gt_velo:
        counts = np.array([s[0] for s in scans], np.int32)
        n_max = max(4, (int(counts.max()) + 3) // 4 * 4)
        pts = torch.full((bs, n_max, 4), float('nan'), dtype=torch.float32,
                         device=self.device)
        for k, (n, off, _) in enumerate(scans):
          if n:
            pts[k, :n] = packed[off:off + 16 * n].view(torch.float32).view(n, 4)
        out += [pts, counts]
    return out

  # -- shutdown ---------------------------------------------------------------
  def close(self):
    """Stops the workers: queued decodes are dropped, running ones finish."""
    self._finalizer()
    self._pending.clear()
    # (a running decode takes milliseconds; never wait long for one)
    deadline = time.monotonic() + 0.5
    for t in list(getattr(self._pool, '_threads', ())):
      t.join(max(0.0, deadline - time.monotonic()))

  def workers_alive(self):
    return sum(t.is_alive() for t in list(getattr(self._pool, '_threads', ())))

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()
    return False
