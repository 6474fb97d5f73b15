"""Novel-view sequences from a predicted LDI: restore a checkpoint as the
evaluation does (`ldi_pred_eval.Tester`: same flags, same data loaders), predict
the layers of a stereo pair and move a camera through them.

  python layered-scene-inference_amd/ldi_render.py --dataset=synthetic \\
      --synth_scene=planes --n_layers=2 --checkpoint_dir=<training dir> \\
      --render_views=9 --render_span=0.5 [--num_render_iter=N]

The camera runs from the source view (s = 0) to the target view (s = 1) and
beyond both by `--render_span`: K values of s on linspace(-A, 1 + A, K), with 0
and 1 inserted where the grid misses them (lsi.geometry.trajectory).  Per
iteration the source LDI of batch element 0 is repeated over the cameras and
rendered by ONE forward_splat call (composed; any pose) at
`--render_downsampling` (1: full resolution), and the white canvas that shows
through cracks and dis-occluded bands is filled by ONE lsi_fill_holes call
(lsi.geometry.fill; `--fill_holes false` leaves it).  The frames
go to a contact sheet -- top row as rendered, bottom row filled, then the real
source and target images -- packed by one launch and written off-thread to
`<results_dir>/render/iter_%06d.png` with an `index.html`; `render.json` lists
per iteration and frame s, the hole fraction (the mean of 1 - c0 inside the
`--splat_bdry_ignore` crop) and, at s = 0 and s = 1, the PSNR against the real
image as rendered and as filled.

With `--save_mesh true` the source LDI of batch element 0 -- the LDI the frames
are splatted from -- is also written as a textured triangle mesh,
`iter_%06d.ply` next to the sheet (lsi.geometry.mesh, DESIGN.md 4.24: one
lsi_ldi_mesh call on the network's output in place; `--mesh_edge_ratio`,
`--mesh_merge_ratio`, `--mesh_disp_min`, `--mesh_flip_yz`), listed with its
vertex and face counts in `render.json` and `index.html`: a surface to orbit in
MeshLab, Blender or Open3D, cut at depth discontinuities, with the hidden layers
behind the foreground.  Without the flag nothing of this runs.

With `--render_mesh true` the same K cameras also render that surface with the
z-buffered triangle rasteriser (lsi.geometry.raster, DESIGN.md 4.25: one
lsi_ldi_raster call on the network's output in place, not repeated over the
cameras; the `--mesh_*` options above and `--mesh_max_extent`) and its holes are
filled by `fill.fill_holes`.  The sheet gains a `mesh` and a `mesh_filled` row
above the real images, every frame of `render.json` gains `hole_fraction_mesh`
(the mean of 1 - cov inside the same crop) and, at s = 0 and s = 1, `psnr_mesh`
and `psnr_mesh_filled`.  A mesh has no cracks between magnified texels, but a
triangle that `--mesh_edge_ratio` cuts or `--mesh_max_extent` drops is a hole of
the mesh too: `hole_fraction` - `hole_fraction_mesh` is the cracks' share of
the splat rendering's holes only where no triangle is cut (a smooth surface, or
`--mesh_edge_ratio 0`); on noisy disparities, an untrained network's for one,
the default ratio cuts most of the surface and the difference is negative.
Without the flag nothing of this runs.
"""
import json
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
  sys.path.insert(0, _HERE)

import ldi_enc_dec as train_script  # noqa: E402
import ldi_pred_eval as ev  # noqa: E402
from lsi.geometry import (fill, ldi as ldi_utils, mesh as mesh_utils, raster,  # noqa: E402
                          trajectory)
from lsi.loss import loss as loss_utils  # noqa: E402
from lsi.nnutils import eval_metrics  # noqa: E402


def build_parser():
  p = ev.build_parser()
  a = p.add_argument
  a('--render_views', type=int, default=9, help='K: cameras on the path')
  a('--render_span', type=float, default=0.5,
    help='A: the camera parameter runs over linspace(-A, 1 + A, K); 0 is the '
    'source view, 1 the target view (both are inserted if the grid misses them)')
  a('--render_downsampling', type=float, default=1.,
    help='size of the frames relative to the input images')
  a('--fill_holes', type=train_script._bool, default=True,
    help='fill what the splats left of the canvas (push-pull, lsi_fill_holes)')
  a('--fill_conf_min', type=float, default=1e-3,
    help='a pixel whose share from the layers is below this is a hole')
  a('--num_render_iter', type=int, default=4, help='pairs to render')
  a('--save_mesh', type=train_script._bool, default=False,
    help='write the source LDI of batch element 0 as a textured triangle mesh, '
    'iter_%%06d.ply (lsi.geometry.mesh, lsi_ldi_mesh)')
  a('--mesh_edge_ratio', type=float, default=mesh_utils.EDGE_RATIO,
    help='a triangle whose smallest disparity is below this times its largest is '
    'cut (a depth discontinuity); a starting value, not a tuned one')
  a('--mesh_merge_ratio', type=float, default=0.,
    help='> 0: a hidden-layer texel whose disparity is at least this times the '
    'disparity of the layer in front is dropped')
  a('--mesh_disp_min', type=float, default=1e-3,
    help='texels with a smaller disparity are no surface')
  a('--mesh_flip_yz', type=train_script._bool, default=True,
    help='y up, looking down -z, as mesh viewers expect (false: camera axes)')
  a('--render_mesh', type=train_script._bool, default=False,
    help='also render the frames by rasterising the LDI\'s triangle mesh '
    '(lsi.geometry.raster, lsi_ldi_raster) under the --mesh_* options')
  a('--mesh_max_extent', type=int, default=32,
    help='a triangle stretched over more target pixels than this, in x or y, is '
    'no surface and is not drawn (1 .. 256)')
  return p


def camera_parameters(views, span):
  """The K values of s, with 0 and 1 inserted where the grid misses them."""
  if views < 1 or not span >= 0:
    raise ValueError('--render_views >= 1 and --render_span >= 0 are needed')
  s = [float(v) for v in np.linspace(-span, 1.0 + span, views)]
  s = [0.0 if abs(v) < 1e-9 else 1.0 if abs(v - 1.0) < 1e-9 else v for v in s]
  return sorted(set(s) | {0.0, 1.0})


class Renderer(ev.Tester):
  """`Tester` with a camera path in place of the metrics."""

  def __init__(self, opts):
    super(Renderer, self).__init__(opts)
    self.s = camera_parameters(opts.render_views, opts.render_span)

  def cameras(self, k_s, k_t, rot, trans):
    """K cameras (k_s, k_t, rot, t) for batch element 0, CPU fp32 tensors."""
    k, r, t = trajectory.interpolate_cameras(k_s[:1], k_t[:1], rot[:1], trans[:1], self.s)
    n = len(self.s)
    k_src = k_s[:1].detach().cpu().float().expand(n, 3, 3).contiguous()
    return k_src, k[:, 0].contiguous(), r[:, 0].contiguous(), t[:, 0].contiguous()

  def splat(self, ldi_k, cams):
    """The K frames: (img 1 x K x Ht x Wt x 3, wts 1 x K x Ht x Wt x 1) of one
    composed forward_splat -- the call of eval_metrics.render_view, so a frame is
    the rendering the evaluation scores.  One launch renders all K cameras:
    general poses take the any-pose kernels, a path of rectified cameras the
    stream kernels (ldi.select_path)."""
    o = self.opts
    img, wts, _ = ldi_utils.forward_splat(
        ldi_k, None, *cams, compose_layers=True, compute_trg_disp=True,
        trg_downsampling=o.render_downsampling, zbuf_scale=o.zbuf_scale,
        bg_layer_disp=o.bg_layer_disp, max_disp=o.max_disp)
    return img, wts

  @torch.no_grad()
  def render_batch(self, batch=None):
    """One pair (None: the next one of the data loader) rendered along the path.
    Returns a dict: `s`, `cams`, `ldi` (the K-fold source LDI), `raw` and `wts`
    (forward_splat's outputs), `conf` (K x Ht x Wt, c0), `filled` (None with
    --fill_holes false), `imgs` (the real source and target image) and `frames`
    (what render.json holds)."""
    tr, o = self.trainer, self.opts
    if batch is None:
      batch = tr.data_loader.forward(o.batch_size)
    imgs_src, imgs_trg, k_s, k_t, rot, trans = batch[:6]
    dev = tr.device
    imgs_src, imgs_trg = imgs_src.to(dev), imgs_trg.to(dev)
    ldi_src, _ = tr.model(imgs_src, imgs_trg)
    # the mesh of batch element 0: the network's output read in place (views,
    # through their strides), before it is repeated over the cameras
    mesh = self.mesh([None if x is None else ev._f32(x)[:, :1] for x in ldi_src],
                     k_s[:1]) if o.save_mesh else None
    n = len(self.s)
    rep = lambda x: None if x is None else ev._f32(x)[:, :1].expand(
        -1, n, -1, -1, -1).contiguous()
    ldi_k = [rep(x) for x in ldi_src]
    cams = self.cameras(k_s, k_t, rot, trans)
    raw, wts = self.splat(ldi_k, cams)
    kw = dict(bg_layer_disp=o.bg_layer_disp, max_disp=o.max_disp, zbuf_scale=o.zbuf_scale,
              conf_min=o.fill_conf_min, n_layers=ldi_k[0].shape[0])
    filled = fill.fill_splat_holes(raw, wts, **kw) if o.fill_holes else None
    conf = fill.splat_confidence(wts, **kw)[0, ..., 0]
    ht, wt = conf.shape[1:]
    x0 = loss_utils._py2_round(wt * o.splat_bdry_ignore)
    y0 = loss_utils._py2_round(ht * o.splat_bdry_ignore)
    holes = (1.0 - conf[:, y0:ht - y0, x0:wt - x0]).mean(dim=(1, 2)).cpu()
    scored = [('psnr_raw', raw), ('psnr_filled', filled)]
    if o.render_mesh:
      # the K frames of the mesh: the network's output read in place, one item
      # under K cameras
      m_img, m_cov, m_filled = self.rasterize(
          [None if x is None else ev._f32(x)[:, :1] for x in ldi_src], cams)
      m_holes = (1.0 - m_cov[0, :, y0:ht - y0, x0:wt - x0]).mean(dim=(1, 2)).cpu()
      scored += [('psnr_mesh', m_img), ('psnr_mesh_filled', m_filled)]
    frames = []
    for i, s in enumerate(self.s):
      f = {'s': s, 'hole_fraction': float(holes[i])}
      if o.render_mesh:
        f['hole_fraction_mesh'] = float(m_holes[i])
      if s in (0.0, 1.0):
        real = ev._f32(imgs_src if s == 0.0 else imgs_trg)[:1]
        for key, img in scored:
          if img is not None:
            f[key] = self.psnr(img[:, i:i + 1], real, [x[i:i + 1] for x in cams])
      frames.append(f)
    out = {'s': list(self.s), 'cams': cams, 'ldi': ldi_k, 'raw': raw, 'wts': wts,
           'conf': conf, 'filled': filled, 'imgs': (imgs_src, imgs_trg), 'frames': frames}
    if mesh is not None:
      out['mesh'] = mesh           # (only with --save_mesh: an LdiMesh, not waited for)
    if o.render_mesh:              # (only with --render_mesh: 1 x K x Ht x Wt [x 3])
      out['mesh_raw'], out['mesh_cov'], out['mesh_filled'] = m_img, m_cov, m_filled
    return out

  def rasterize(self, ldi, cams):
    """The K frames of the mesh of a one-item LDI under --mesh_*: (img 1 x K x Ht
    x Wt x 3, cov 1 x K x Ht x Wt, img with its holes filled) of one
    lsi_ldi_raster and one lsi_fill_holes call.  The K matrices are built on the
    host; their copy to the device blocks the host, nothing else does."""
    o = self.opts
    ht, wt = int(o.img_height * o.render_downsampling), int(o.img_width * o.render_downsampling)
    img, cov, _ = raster.render_views(
        ldi, *cams, trg_downsampling=o.render_downsampling, trg_size=(ht, wt),
        disp_min=o.mesh_disp_min, edge_ratio=o.mesh_edge_ratio, merge_ratio=o.mesh_merge_ratio,
        max_extent=o.mesh_max_extent)
    filled = fill.fill_holes(img[0], cov[0], conf_min=o.fill_conf_min).unsqueeze(0)
    return img, cov, filled

  def mesh(self, ldi, k_s):
    """The LdiMesh of an LDI under --mesh_*: one lsi_ldi_mesh call, no
    synchronisation."""
    o = self.opts
    return mesh_utils.ldi_mesh(ldi, k_s.detach().cpu().float(), disp_min=o.mesh_disp_min,
                               edge_ratio=o.mesh_edge_ratio, merge_ratio=o.mesh_merge_ratio,
                               flip_yz=o.mesh_flip_yz)

  def psnr(self, frame, real, cams):
    """The evaluation's PSNR (eval_metrics.view_synthesis_metrics) of one frame
    1 x 1 x Ht x Wt x 3 against the real image 1 x H x W x 3."""
    out = eval_metrics.view_synthesis_metrics(
        None, None, cams[0], cams[1], cams[2], cams[3], real, self.opts,
        rendered=(frame, None))
    return float(out['psnr'][0])

  def render(self, batches=None):
    """`batches`: the iterations' batches instead of the data loader's.  Returns
    what render.json holds."""
    from lsi.visualization import SheetBuilder, VisualWriter  # pylint: disable=g-import-not-at-top
    o = self.opts
    self.restore()
    res_dir = os.path.join(o.results_dir or os.path.join(o.checkpoint_dir, 'results'),
                           'render')
    os.makedirs(res_dir, exist_ok=True)
    n = len(self.s)
    ht, wt = int(o.img_height * o.render_downsampling), int(o.img_width * o.render_downsampling)
    sb = SheetBuilder(self.trainer.device, n, max(ht, o.img_height), max(wt, o.img_width))
    writer = VisualWriter(res_dir)
    sheet, iters = None, []
    try:
      for it in range(o.num_render_iter):
        r = self.render_batch(batches[it] if batches else None)
        sb.clear()
        rows = [('raw', r['raw']), ('filled', r['filled'])]
        if o.render_mesh:
          rows += [('mesh', r['mesh_raw']), ('mesh_filled', r['mesh_filled'])]
        for key, img in rows:
          if img is not None:
            for i, s in enumerate(r['s']):
              sb.add_rgb('%s_s_%+.3f' % (key, s), img[0, i])
        sb.add_rgb('src_im', ev._f32(r['imgs'][0])[0])
        sb.add_rgb('trg_im', ev._f32(r['imgs'][1])[0])
        sheet = sb.pack(out=sheet)
        writer.submit('iter_%06d' % it, sheet, sb.names, sb.meta())
        sb.clear()
        iters.append({'file': 'iter_%06d.png' % it, 'frames': r['frames']})
        if 'mesh' in r:
          # counts and used records to the host (the mesh's one wait); the file
          # is written by the writer's thread
          (vertices, faces), = r['mesh'].to_host()
          iters[-1]['mesh'] = writer.submit_mesh('iter_%06d' % it, vertices, faces)
    finally:
      writer.close()
    with open(os.path.join(res_dir, 'render.json'), 'w') as f:
      json.dump(iters, f, indent=1)
    return iters


def main(argv=None):
  opts = train_script.apply_dataset_overrides(build_parser().parse_args(argv))
  renderer = Renderer(opts)
  try:
    iters = renderer.render()
  finally:
    close = getattr(getattr(renderer.trainer, 'data_loader', None), 'close', None)
    if close is not None:
      close()  # a prefetching loader's decode threads (--data_workers)
  if renderer.trainer.rank == 0:
    print(json.dumps({'restored': renderer.restored, 'iterations': len(iters),
                      'frames': iters[0]['frames'] if iters else []}))


if __name__ == '__main__':
  main()
