"""Writes contact sheets as PNG files off the caller's thread."""
import html
import json
import os
import queue
import threading

import numpy as np
import torch

PNG_COMPRESS_LEVEL = 3  # fixed, so that a sheet's file is the same on every run


class VisualWriter(object):
  """`submit` copies a sheet to the host once -- one device-to-host copy into a
  pinned buffer, followed by an event on the current stream -- and returns; one
  worker thread waits for that event, encodes `<directory>/<stem>.png` with
  Pillow and writes it.  The worker makes no other GPU call and starts no
  process.  At most `max_pending` sheets are in flight: `submit` blocks beyond
  that.  `close()` joins the worker, writes `visuals.json` (per sheet: file,
  grid, cell size, names, value ranges) and a plain `index.html`, and re-raises
  the first exception the worker met.  Host uint8 arrays are accepted in place
  of device sheets (no copy to pin, no event).  `submit_mesh` hands the same
  worker the host records of a mesh (lsi.geometry.mesh) to write as
  `<directory>/<stem>.ply`; the page lists the meshes after the sheets."""

  def __init__(self, directory, max_pending=2):
    if max_pending < 1:
      raise ValueError('max_pending must be at least 1')
    self.directory = directory
    os.makedirs(directory, exist_ok=True)
    self.sheets = []             # the legend entries, in submission order
    self.meshes = []             # {file, vertices, faces} of the meshes, likewise
    self._slots = threading.Semaphore(max_pending)
    self._jobs = queue.Queue()
    self._pinned = {}            # bytes -> idle pinned buffers of that size
    self._error = None
    self._thread = threading.Thread(target=self._work, name='visual-writer',
                                    daemon=True)
    self._thread.start()

  def submit(self, stem, sheet_u8, names, meta):
    """sheet_u8: Hs x Ws x 3 uint8, a device tensor as SheetBuilder.pack returns
    it (padded rows are copied with their padding, as one block) or a host
    array; meta: SheetBuilder.meta()."""
    if self._thread is None:
      raise RuntimeError('the writer is closed')
    hs, ws, ch = sheet_u8.shape
    u8 = torch.uint8 if isinstance(sheet_u8, torch.Tensor) else np.dtype(np.uint8)
    if ch != 3 or sheet_u8.dtype != u8:
      raise ValueError('a sheet is Hs x Ws x 3 uint8')
    self._slots.acquire()
    try:
      if isinstance(sheet_u8, torch.Tensor) and sheet_u8.is_cuda:
        if sheet_u8.stride()[1:] != (3, 1) or sheet_u8.stride(0) < 3 * ws:
          sheet_u8 = sheet_u8.contiguous()
        pitch = sheet_u8.stride(0)
        nbytes = (hs - 1) * pitch + 3 * ws
        idle = self._pinned.setdefault(nbytes, [])
        host = idle.pop() if idle else torch.empty((nbytes,), dtype=torch.uint8,
                                                   pin_memory=True)
        host.copy_(torch.as_strided(sheet_u8, (nbytes,), (1,)), non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(sheet_u8.device))
      else:
        host, event, pitch = np.array(sheet_u8, dtype=np.uint8, order='C'), None, 3 * ws
    except BaseException:
      self._slots.release()
      raise
    entry = dict(meta or {}, file=stem + '.png', names=list(names),
                 height=int(hs), width=int(ws))
    self.sheets.append(entry)
    self._jobs.put((entry['file'], host, event, (hs, ws, pitch)))

  def submit_mesh(self, stem, vertices, faces):
    """vertices, faces: host record arrays of one item (LdiMesh.to_host)."""
    if self._thread is None:
      raise RuntimeError('the writer is closed')
    from lsi.geometry import mesh  # pylint: disable=g-import-not-at-top
    self._slots.acquire()
    entry = {'file': stem + '.ply', 'vertices': len(vertices), 'faces': len(faces)}
    self.meshes.append(entry)
    path = os.path.join(self.directory, entry['file'])
    self._jobs.put((entry['file'], lambda: mesh.write_ply(path, vertices, faces), None, None))
    return entry

  def _work(self):
    from PIL import Image  # pylint: disable=g-import-not-at-top
    while True:
      job = self._jobs.get()
      if job is None:
        return
      name, host, event, size = job
      try:
        if self._error is None and size is None:
          host()                   # a mesh: its file
        elif self._error is None:
          hs, ws, pitch = size
          if event is not None:
            event.synchronize()
            rows = np.lib.stride_tricks.as_strided(host.numpy(), (hs, ws, 3),
                                                   (pitch, 3, 1))
          else:
            rows = host
          Image.fromarray(np.ascontiguousarray(rows), 'RGB').save(
              os.path.join(self.directory, name), format='PNG',
              compress_level=PNG_COMPRESS_LEVEL)
      except BaseException as e:  # pylint: disable=broad-except
        self._error = e
      finally:
        if event is not None:
          self._pinned[host.numel()].append(host)
        self._slots.release()

  def close(self):
    """Idempotent."""
    if self._thread is None:
      return
    self._jobs.put(None)
    self._thread.join()
    self._thread = None
    self._pinned.clear()
    try:
      with open(os.path.join(self.directory, 'visuals.json'), 'w') as f:
        json.dump(self.sheets, f, indent=1)
      with open(os.path.join(self.directory, 'index.html'), 'w') as f:
        f.write(self._html())
    finally:
      if self._error is not None:
        raise self._error

  def _html(self):
    out = ['<!DOCTYPE html>', '<html><head><meta charset="utf-8">',
           '<title>visuals</title></head><body>']
    for s in self.sheets:
      out.append('<h2>%s</h2>' % html.escape(s['file']))
      out.append('<img src="%s" width="%d" height="%d">' %
                 (html.escape(s['file'], quote=True), s['width'], s['height']))
      cols = int(s.get('cols') or len(s['names']) or 1)
      ranges = s.get('ranges') or [None] * len(s['names'])
      out.append('<table border="1">')
      for r in range(0, len(s['names']), cols):
        cells = []
        for name, rng in zip(s['names'][r:r + cols], ranges[r:r + cols]):
          cells.append('<td>%s%s</td>' % (html.escape(name),
                                          ' [%g, %g]' % tuple(rng) if rng else ''))
        out.append('<tr>%s</tr>' % ''.join(cells))
      out.append('</table>')
    for m in self.meshes:
      out.append('<p><a href="%s">%s</a>: %d vertices, %d faces</p>' %
                 (html.escape(m['file'], quote=True), html.escape(m['file']),
                  m['vertices'], m['faces']))
    out.append('</body></html>')
    return '\n'.join(out) + '\n'
