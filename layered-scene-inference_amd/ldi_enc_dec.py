"""Script for training an LDI predictor via the view-synthesis loss: the eager,
MI355X counterpart of the reference's `ldi_enc_dec.py` (same flag names and
defaults, same dataset-dependent overrides, same six loss terms).

  python layered-scene-inference_amd/ldi_enc_dec.py --dataset=kitti \\
      --batch_size=4 --n_layers=2 --img_height=256 --img_width=768 ...
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
      layered-scene-inference_amd/ldi_enc_dec.py ...      # DDP over RCCL

`--dataset=kitti` reads stereo pairs through lsi/data/kitti (--kitti_data_root,
--kitti_dataset_variant, --data_split, as the reference).  The data set is not
available in the build container (no network): `--kitti_procedural=true` keeps
the KITTI camera model and the dataset-dependent constants
(ldi_enc_dec.py:415-427) and feeds procedural pairs instead (a smooth random
texture seen from the two cameras through one fronto-parallel plane, so that
the view-synthesis loss has something consistent to explain); the SUN / PASCAL
textures of the synthetic scenes are procedural as well.
"""
import argparse
import contextlib
import math
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
  sys.path.insert(0, _HERE)

from lsi.geometry import ldi as ldi_utils  # noqa: E402
from lsi.geometry import projection  # noqa: E402
from lsi.loss import objective  # noqa: E402
from lsi.nnutils import helpers as nn_helpers  # noqa: E402
from lsi.nnutils import nets  # noqa: E402
from lsi.nnutils import train_utils  # noqa: E402


def _bool(v):
  return str(v).lower() in ('1', 'true', 'yes')


DEPTH_SUP_SOURCES = (
    "--dataset synthetic with --synth_scene planes or planes_batched (the scenes' "
    'foreground disparities), KITTI files with --kitti_dl_disparities_px true '
    '(stereo disparities) or KITTI files with --kitti_dl_velodyne true (Velodyne '
    'scans, rasterised on the device); KITTI files emit either on the val / '
    'test splits, and on the train split with --kitti_gt_everywhere true')


def depth_sup_source(opts):
  """Where --depth_sup_wt > 0 takes its ground truth from: 'planes', 'px' or
  'velodyne'; ValueError for a configuration that has none."""
  if opts.dataset == 'synthetic' and opts.synth_scene in ('planes', 'planes_batched'):
    return 'planes'
  if opts.dataset == 'kitti' and not opts.kitti_procedural:
    px = bool(getattr(opts, 'kitti_dl_disparities_px', False))
    velodyne = bool(getattr(opts, 'kitti_dl_velodyne', False))
    if px != velodyne:
      return 'px' if px else 'velodyne'
  raise ValueError('--depth_sup_wt > 0 needs ground-truth depth from exactly one of: '
                   + DEPTH_SUP_SOURCES)


def build_parser():
  p = argparse.ArgumentParser(description=__doc__)
  train_utils.define_default_flags(p)
  a = p.add_argument
  # experiment flags: names and defaults of reference ldi_enc_dec.py:39-123
  a('--exp_name', default='synth_ldi_pred_encdec')
  a('--n_layers', type=int, default=2)
  a('--pred_ldi_masks', type=_bool, default=False)
  a('--dataset', default='synthetic', choices=['synthetic', 'kitti'])
  a('--data_split', default='train', choices=['all', 'train', 'val', 'test'])
  # KITTI (reference ldi_enc_dec.py:76-83)
  a('--kitti_data_root', default='/datasets/kitti')
  a('--kitti_dataset_variant', default='mview',
    choices=['odom', 'mview', 'raw_city'])
  a('--kitti_dl_disparities', type=_bool, default=False)
  a('--kitti_dl_disparities_px', type=_bool, default=False,
    help='under the conditions of --kitti_dl_disparities: append the SPS-stereo '
    'disparities of both views in pixels of the resized image, both bytes of the '
    '16-bit PNG, nearest-neighbour sampled (the ground truth of --eval_depth; '
    'the synchronous loader only, unless --kitti_gt_everywhere)')
  a('--kitti_dl_velodyne', type=_bool, default=False,
    help='under the conditions of --kitti_dl_disparities: append the Velodyne '
    'scan of every pair (velodyne_points/data/N.bin, NaN-padded), its point '
    'count and the two 3 x 4 projections into the resized views (the standard '
    'ground truth of --eval_depth; the synchronous loader only, unless '
    '--kitti_gt_everywhere)')
  a('--kitti_gt_everywhere', type=_bool, default=False,
    help='--kitti_dl_disparities_px and --kitti_dl_velodyne take effect on the '
    'train split too, are served by the prefetching loader (--data_workers, '
    '--kitti_resize host or device) and are cropped, flipped and scaled with '
    'their pair under --kitti_augment (DESIGN.md 4.12c).  false: both stay with '
    'the synchronous loader on val / test, unaugmented')
  a('--kitti_procedural', type=_bool, default=False,
    help='no KITTI files: procedural stereo pairs seen through the KITTI camera '
    'model and constants (throughput runs, tests).  Without this switch a '
    'missing --kitti_data_root is an error')
  a('--data_workers', type=int, default=0,
    help='KITTI files: threads that decode PNGs ahead of the step '
    '(lsi/data/kitti/pipeline.py; clamped to [1, 16] and divided by the world '
    'size).  0 = the synchronous loader')
  a('--kitti_resize', default='host', choices=['host', 'device'],
    help="KITTI files: the AREA resize in NumPy ('host') or as one HIP launch "
    "per batch on the decoded uint8 pixels ('device': csrc/lsi_image.hip; "
    'needs a ROCm device)')
  a('--kitti_augment', type=_bool, default=False,
    help='KITTI files, training: augment every stereo pair -- random crop, '
    'horizontal flip and colour, images and cameras together (lsi/data/kitti/'
    'augment.py, DESIGN.md 4.12b); fused into the resize launch with '
    '--kitti_resize device.  false: the --aug_* values are not read')
  a('--aug_flip_prob', type=float, default=0.5)
  a('--aug_zoom_max', type=float, default=1.15,
    help='the crop window is the image divided by a zoom in [1, this] per '
    'axis, placed at random; 1 = no crop')
  a('--aug_color_prob', type=float, default=0.5,
    help='probability of a colour change: gamma, brightness and per-channel '
    'factors from the three ranges below')
  a('--aug_gamma', type=float, nargs=2, default=[0.8, 1.2], metavar=('LO', 'HI'))
  a('--aug_brightness', type=float, nargs=2, default=[0.5, 2.0], metavar=('LO', 'HI'))
  a('--aug_color', type=float, nargs=2, default=[0.8, 1.2], metavar=('LO', 'HI'))
  a('--aug_seed', type=int, default=0,
    help='seed of the augmentation draws (every rank draws its own sequence)')
  a('--self_cons_wt', type=float, default=1.0)
  a('--l0_self_cons', type=_bool, default=False)
  a('--indep_splat_wt', type=float, default=1.0)
  a('--compose_splat_wt', type=float, default=1.0)
  a('--splat_bdry_ignore', type=float, default=0.1)
  a('--ssim_wt', type=float, default=0.0,
    help='weight of the structural view-synthesis terms (DSSIM over '
    '--ssim_win windows, csrc/lsi_ssim.hip): ssim_wt * (compose_splat_wt * '
    'compose_ssim_loss + indep_splat_wt * indep_ssim_loss) is added to the '
    'total; 0 = the six reference terms only')
  a('--ssim_win', type=int, default=7, help='SSIM window size: odd, 3 .. 11')
  a('--ssim_sigma', type=float, default=1.5,
    help='sigma of the Gaussian SSIM window; <= 0: the box window')
  a('--edge_smooth_wt', type=float, default=0.0,
    help='weight of the edge-aware disparity smoothness term (csrc/'
    'lsi_edge_smooth.hip, DESIGN.md 4.14): edge_smooth_wt * edge_smooth_loss is '
    'added to the total, divided by max_disp when --edge_smooth_norm is false; '
    '0 = no such term')
  a('--edge_smooth_alpha', type=float, default=1.0,
    help='the weights are exp(-alpha * mean_c |guide gradient|)')
  a('--edge_smooth_order', type=int, default=1, choices=[1, 2],
    help='first or second differences of the disparities')
  a('--edge_smooth_norm', type=_bool, default=True,
    help="divide every plane's disparities by their mean (scale-free term)")
  a('--edge_smooth_guide', default='image', choices=['image', 'texture'],
    help="'image': every layer is guided by the view's input image; 'texture': "
    'each layer by its own predicted texture, detached')
  a('--depth_sup_wt', type=float, default=0.0,
    help='weight of the depth-supervision term against sparse ground truth '
    '(csrc/lsi_depth_sup.hip, DESIGN.md 4.20): depth_sup_wt * depth_sup_loss is '
    'added to the total; it supervises layer 0 of each view\'s disparities.  '
    'Ground truth: ' + DEPTH_SUP_SOURCES + '.  0 = no such term, no extra '
    'loader output')
  a('--depth_sup_mode', default='silog', choices=['silog', 'l1'],
    help='the scale-invariant log error of Eigen et al. 2014, or a plain L1')
  a('--depth_sup_lambda', type=float, default=0.5,
    help='silog: mean(d^2) - lambda mean(d)^2, 0 <= lambda <= 1')
  a('--depth_sup_min', type=float, default=1e-3,
    help='ground truth nearer than this depth is not scored')
  a('--depth_sup_max', type=float, default=80.,
    help='ground truth beyond this depth is not scored')
  a('--geo_cons_wt', type=float, default=0.0,
    help='weight of the geometric-consistency term between the two views\' '
    'layer-0 disparities (csrc/lsi_geo_cons.hip, DESIGN.md 4.21): geo_cons_wt * '
    'geo_cons_loss is added to the total, divided by max_disp in l1 mode; 0 = no '
    'such term, no extra launch')
  a('--geo_cons_mode', default='ratio', choices=['ratio', 'l1'],
    help='|dd - s| / (dd + s), scale-free, or a plain |dd - s|')
  a('--geo_cons_occl', type=float, default=0.0,
    help='a pixel whose projection lies behind the other view\'s surface, s - dd > '
    'geo_cons_occl * (s + dd), is not scored; 0 = every pixel that lands is')
  a('--photo_reproj_wt', type=float, default=0.0,
    help='weight of the backward-warp photometric term (csrc/lsi_photo_reproj.hip, '
    'DESIGN.md 4.23): every pixel\'s disparity is projected into the other view, '
    'that view\'s input image is sampled bilinearly where the point lands and the '
    'sample is compared with the colour the pixel should have there; '
    'photo_reproj_wt * photo_reproj_loss is added to the total; 0 = no such term, '
    'no extra launch')
  a('--photo_reproj_mode', default='l1', choices=['l1', 'charb'],
    help='|tex - s|, or the Charbonnier sqrt((tex - s)^2 + 1e-6), mean over the '
    'channels')
  a('--photo_reproj_occl', type=float, default=0.2,
    help='a point that lies behind the other view\'s layer-0 surface, sd - dd > '
    'photo_reproj_occl * (sd + dd), is not scored; 0 = every pixel that lands is')
  a('--photo_reproj_what', default='texture', choices=['texture', 'image'],
    help="'texture': every layer's predicted texture at that layer's disparity -- "
    "hidden layers learn their colours where the other view sees them; 'image': "
    "layer 0's disparity only, compared with the view's own input image (the "
    'classic monocular-depth term; no texture gradient)')
  a('--zbuf_scale', type=float, default=50)
  a('--trg_splat_downsampling', type=float, default=0.5)
  a('--disp_smoothness_wt', type=float, default=0.1)
  a('--incr_depth_wt', type=float, default=10.0)
  a('--use_unet', type=_bool, default=True)
  a('--n_layerwise_steps', type=int, default=3)
  a('--bg_layer_disp', type=float, default=1e-6)
  a('--depth_softmax_temp', type=float, default=1e-6)
  a('--max_disp', type=float, default=0)
  # build-specific switches
  # synthetic planar worlds (reference ldi_enc_dec.py:52-55, 86-123): procedural
  # textures replace the SUN / PASCAL images
  a('--synth_scene', default='pairs', choices=['pairs', 'planes', 'planes_batched'],
    help="synthetic inputs: 'pairs' = shifted smooth images generated on the "
    "device (throughput runs); 'planes' = box room + billboard objects "
    'rendered through planar_transform + compose (lsi/data/synthetic_planes); '
    "'planes_batched' = the same scenes, textures made on the device and the "
    'whole batch rendered by one fused launch (synthetic_planes.BatchedDataLoader)')
  a('--debug_synth_texture', type=_bool, default=False,
    help='feed the ground-truth fg / bg disparities in place of the predicted '
    'ones (n_layers = 2, --synth_scene planes): the renderer must then '
    'reconstruct the other view')
  a('--synth_ds_factor', type=int, default=1)
  a('--n_obj_min', type=int, default=1)
  a('--n_obj_max', type=int, default=4)
  a('--n_box_planes', type=int, default=5)
  a('--bf16', type=_bool, default=True,
    help='the network in bf16 (torch.autocast) with fp32 accumulation -- the '
    'product default on a ROCm device: every convolution then runs on this '
    "repo's MFMA kernels (csrc/lsi_conv*.hip), every batch norm on csrc/lsi_bn.hip "
    '(BASELINE config 4: "bf16 convs + fp32 splat"); the renderer and the losses '
    'are fp32 either way.  false = the reference\'s own arithmetic (fp32 '
    'convolutions): through the library (MIOpen), DESIGN.md 4.8')
  a('--fp32_convs', choices=('library', 'own'),
    default='own' if os.environ.get('LSI_F32_CONV', '') == '1' else 'library',
    help='with --bf16 false: the batch-normed convolutions on the library '
    '(MIOpen) or on the exact-fp32 MFMA kernels of csrc/lsi_conv_f32.hip (forward, '
    'data and weight gradients; DESIGN.md 4.7b).  Default: library (own when '
    'LSI_F32_CONV=1)')
  a('--batched_pairs', type=_bool, default=True,
    help='source and target images go through the network in one pass, every '
    'batch norm with separate statistics per view (same arithmetic as two passes)')
  a('--paired_splat', type=_bool, default=True,
    help='with --batched_pairs: the src -> trg and trg -> src renderings of a step '
    'are one forward_splat_both call on the 2 B LDIs the network pass produced')
  a('--fused_adam', type=_bool, default=True,
    help='torch.optim.Adam(fused=True) on the GPU')
  a('--miopen_tune', type=_bool, default=False,
    help='let MIOpen tune its convolution solvers for this run (one-time 50-100 s; '
    'MIOPEN_FIND_ENFORCE=3, cached in ~/.config/miopen)')
  a('--flat_grads', type=_bool, default=False,
    help='data parallel without the DDP wrapper: one flat gradient buffer, one '
    'all-reduce per step (implied by --hip_graph with more than one rank)')
  a('--channels_last', type=_bool, default=True)
  a('--cpu', type=_bool, default=False,
    help='keep the model on the CPU (plumbing tests only: the renderer and the '
    'losses are HIP kernels, compute_losses raises without a ROCm device)')
  a('--miopen_search', type=_bool, default=False,
    help='exhaustive MIOpen solver search (torch.backends.cudnn.benchmark)')
  a('--tf_checkpoint_complete', type=_bool, default=False,
    help='also hold the variables the reference creates and checkpoints but '
    'never trains (the fc stack on the U-Net bottleneck, upcnv3 .. icnv1), '
    'frozen: the exact variable list of a TF checkpoint (lsi/nnutils/'
    'tf_checkpoint.py)')
  a('--hip_graph', type=_bool, default=False,
    help='capture the training step in a HIP graph (single process)')
  return p


def apply_dataset_overrides(opts):
  """ldi_enc_dec.py:415-427."""
  opts.checkpoint_dir = os.path.join(opts.checkpoint_dir, opts.exp_name)
  if opts.dataset == 'synthetic':
    opts.bg_layer_disp = 2e-1
    opts.depth_softmax_temp = 0.4
    if opts.max_disp == 0:
      opts.max_disp = 1.0
  elif opts.dataset == 'kitti':
    opts.bg_layer_disp = 1e-3
    opts.depth_softmax_temp = 0.4
    if opts.max_disp == 0:
      opts.max_disp = 0.4
  return opts


class LdiNet(torch.nn.Module):
  """encoder-decoder + per-layer LDI heads (define_pred_graph,
  ldi_enc_dec.py:175-228); the same weights process src and trg images."""

  def __init__(self, opts):
    super().__init__()
    if opts.use_unet:
      complete = bool(getattr(opts, 'tf_checkpoint_complete', False))
      self.enc_dec = nets.encoder_decoder_unet(
          nl_diff_enc_dec=opts.n_layerwise_steps, with_fc=complete,
          with_dead_decoder=complete,
          in_hw=(opts.img_height, opts.img_width))
    else:
      self.enc_dec = nets.encoder_decoder_simple(
          nl_diff_enc_dec=opts.n_layerwise_steps,
          in_hw=(opts.img_height, opts.img_width))
    self.ldi_tex_disp = nets.ldi_predictor(
        self.enc_dec.out_channels, n_layers=opts.n_layers,
        n_layerwise_steps=opts.n_layerwise_steps,
        skip_channels=self.enc_dec.skip_channels,
        pred_masks=opts.pred_ldi_masks)
    self.max_disp = opts.max_disp
    # (the `fc` stack of the complete TF parameter set sees the batch as one)
    self.batched_pairs = bool(getattr(opts, 'batched_pairs', True))

  def predict(self, imgs):
    _, feat_dec, skip_feat, _ = self.enc_dec(imgs)
    # float32 LDI, disparities scaled by max_disp (ldi_enc_dec.py:203-205)
    return self.ldi_tex_disp(feat_dec, skip_feat, disp_scale=self.max_disp)

  def forward(self, imgs_src, imgs_trg):
    self.pair_ldi = None
    if not self.batched_pairs or imgs_src.shape != imgs_trg.shape:
      return self.predict(imgs_src), self.predict(imgs_trg)
    # One pass over [src; trg]: every batch norm keeps separate statistics for
    # the two halves (nets.bn_groups), so the result is the reference's two
    # passes (ldi_enc_dec.py:175-228) with half the kernel launches and the
    # convolutions at twice the batch.  The halves come back as views.
    b = imgs_src.shape[0]
    with nets.bn_groups(2):
      tex, masks, disps = self.predict(torch.cat([imgs_src, imgs_trg], dim=0))
    half = lambda t, k: None if t is None else t[:, k * b:(k + 1) * b]
    # (the un-halved LDI: the trainer renders both directions with one launch)
    self.pair_ldi = [tex, masks, disps]
    return ([half(tex, 0), half(masks, 0), half(disps, 0)],
            [half(tex, 1), half(masks, 1), half(disps, 1)])


class SyntheticPairs(object):
  """Procedural stereo-like pairs with the dataset's camera model."""

  def __init__(self, opts, device, seed):
    self.opts, self.device = opts, device
    # images are generated where they are consumed (the CPU version of this
    # generator cost 12-20 ms per batch, a third of a training step)
    self.gen = torch.Generator(device=device).manual_seed(seed)

  def forward(self, bs):
    o = self.opts
    h, w = o.img_height, o.img_width
    lo = torch.rand((bs, 3, h // 16 + 2, w // 16 + 2), generator=self.gen,
                    device=self.device)
    img = torch.nn.functional.interpolate(lo, size=(h, w + 64), mode='bicubic',
                                          align_corners=False).clamp(0, 1)
    shift = 16  # pixels of parallax of the (single, fronto-parallel) plane
    src = img[..., 32:32 + w].permute(0, 2, 3, 1).contiguous()
    trg = img[..., 32 - shift:32 - shift + w].permute(0, 2, 3, 1).contiguous()
    if o.dataset == 'kitti':
      k = torch.tensor([[0.58 * w, 0, w / 2.0], [0, 0.58 * w, h / 2.0],
                        [0, 0, 1.0]])
      t = torch.tensor([[-0.532], [0.0], [0.0]])
    else:
      k = torch.tensor([[float(w), 0, w / 2.0], [0, float(h), h / 2.0],
                        [0, 0, 1.0]])
      t = torch.tensor([[-0.3], [0.0], [0.0]])
    k = k.expand(bs, 3, 3).contiguous()
    rot = torch.eye(3).expand(bs, 3, 3).contiguous()
    t = t.expand(bs, 3, 1).contiguous()
    return (src, trg, k, k.clone(), rot, t)


def _halves_of(a, b):
  """The tensor whose two halves along the batch axis `a` and `b` are -- as the
  prefetching loader's device route returns its disparity maps -- or None."""
  base = getattr(a, '_base', None)
  if (base is None or base is not getattr(b, '_base', None) or
      base.dtype != torch.float32 or a.dtype != base.dtype or b.dtype != base.dtype or
      not (base.is_contiguous() and a.is_contiguous() and b.is_contiguous()) or
      base.dim() != a.dim() or a.shape != b.shape or a.shape[1:] != base.shape[1:] or
      base.shape[0] != 2 * a.shape[0] or a.data_ptr() != base.data_ptr() or
      b.data_ptr() != base.data_ptr() + a.numel() * a.element_size()):
    return None
  return base


class KittiBatches(object):
  """lsi.data.kitti.DataLoader batches (NumPy) as float32 torch tensors:
  (img_s, img_t, k_s, k_t, rot, trans[, disp_s, disp_t])."""

  def __init__(self, loader, rank=0):
    self.loader = loader
    # every rank walks the data in its own order
    loader._rng = __import__('numpy').random.RandomState(rank)
    if getattr(loader, 'augment', None) is not None:   # --kitti_augment
      loader._aug_rng = __import__('numpy').random.RandomState(
          [int(loader.aug_seed), rank])

  @property
  def src_image_names(self):
    return self.loader.src_image_names

  def forward(self, bs):
    # (integer outputs -- the point counts of --kitti_dl_velodyne -- stay integers)
    # (a prefetching loader hands on tensors: their dtype has no `kind`)
    return tuple(torch.as_tensor(a) if getattr(getattr(a, 'dtype', None), 'kind', None)
                 in ('i', 'u') else torch.as_tensor(a, dtype=torch.float32)
                 for a in self.loader.forward(bs))

  def close(self):
    """Stops a prefetching loader's workers (nothing to do otherwise)."""
    close = getattr(self.loader, 'close', None)
    if close is not None:
      close()


class Trainer(train_utils.Trainer):
  """LDI prediction trainer (reference ldi_enc_dec.py:126-410)."""

  def define_data_loader(self):
    opts = self.opts
    # (decided before a loader is built: a loader emits ground truth on request)
    self.depth_sup_source = (depth_sup_source(opts)
                             if getattr(opts, 'depth_sup_wt', 0.0) > 0 else None)
    if getattr(opts, 'kitti_augment', False) and (
        opts.dataset != 'kitti' or opts.kitti_procedural):
      raise ValueError(
          '--kitti_augment true augments KITTI files (--dataset kitti without '
          '--kitti_procedural): the synthetic and procedural generators are not '
          'augmented')
    if opts.dataset == 'synthetic' and (opts.synth_scene in ('planes',
                                                             'planes_batched') or
                                        opts.debug_synth_texture):
      from lsi.data import synthetic_planes  # pylint: disable=g-import-not-at-top
      if opts.debug_synth_texture and opts.n_layers != 2:
        raise ValueError('debug_synth_texture feeds (fg, bg) disparities: '
                         'n_layers must be 2')
      opts.synth_dl_eval_data = (bool(opts.debug_synth_texture) or
                                 self.depth_sup_source == 'planes' or
                                 bool(getattr(opts, 'synth_dl_eval_data', False)))
      loader = (synthetic_planes.BatchedDataLoader
                if opts.synth_scene == 'planes_batched' else
                synthetic_planes.DataLoader)
      self.data_loader = loader(opts, device=self.device, seed=1234 + self.rank)
    elif opts.dataset == 'kitti' and not opts.kitti_procedural:
      # reference ldi_enc_dec.py:134-137
      from lsi.data.kitti import data as kitti_data  # pylint: disable=g-import-not-at-top
      if not os.path.isdir(opts.kitti_data_root):
        raise FileNotFoundError(
            '--dataset=kitti: no directory %r (--kitti_data_root); pass '
            '--kitti_procedural=true for procedural pairs with KITTI cameras'
            % opts.kitti_data_root)
      loader = kitti_data.DataLoader(opts)
      workers = int(getattr(opts, 'data_workers', 0))
      resize = getattr(opts, 'kitti_resize', 'host')
      if workers != 0 or resize != 'host':
        if resize == 'device' and self.device.type != 'cuda':
          raise ValueError(
              '--kitti_resize device runs the AREA resize as a HIP kernel: it '
              'needs a ROCm device (this run is on %s); use --kitti_resize host'
              % self.device)
        from lsi.data.kitti import pipeline  # pylint: disable=g-import-not-at-top
        loader = pipeline.PrefetchLoader(
            loader, workers=workers, resize=resize, device=self.device,
            world_size=self.world)
      self.data_loader = KittiBatches(loader, self.rank)
    else:
      self.data_loader = SyntheticPairs(opts, self.device, 1234 + self.rank)
    bs = self.opts.batch_size
    self.pixel_coords = nn_helpers.pixel_coords(bs, self.opts.img_height,
                                                self.opts.img_width)

  def build_model(self):
    return LdiNet(self.opts)

  def _depth_sup_outputs(self, batch):
    """The loader outputs --depth_sup_wt > 0 builds its ground truth from."""
    src = self.depth_sup_source
    if src == 'planes' and len(batch) >= 14:
      return (src, batch[8], batch[10])        # disp_s_fg, disp_t_fg
    if src == 'px' and len(batch) >= 8:
      return (src, batch[-2], batch[-1])
    if src == 'velodyne' and len(batch) >= 9:
      return (src, batch[-3], batch[-2], batch[-1])  # points, counts, matrices
    raise ValueError(
        '--depth_sup_wt > 0: the loader emitted %d outputs, none of them ground '
        'truth (the KITTI loader emits it on the val / test splits only; on '
        'train with --kitti_gt_everywhere true).  The term takes it from: %s'
        % (len(batch), DEPTH_SUP_SOURCES))

  def feed(self):
    """One batch: (img_src, img_trg, k_s, k_t, rot, trans); with
    debug_synth_texture also the ground-truth LDI disparities (reference
    ldi_enc_dec.py:230-263); with --depth_sup_wt > 0 a seventh entry, the loader
    outputs `stage` makes the term's ground truth from."""
    batch = self.data_loader.forward(self.opts.batch_size)
    self.gt_disps = None
    if self.opts.debug_synth_texture:
      (_, _, _, _, _, _, _, _, d_s_fg, d_s_bg, d_t_fg, d_t_bg, _, _) = batch
      self.gt_disps = (torch.stack([d_s_fg, d_s_bg], 0),
                       torch.stack([d_t_fg, d_t_bg], 0))
    if getattr(self, 'depth_sup_source', None) is not None:
      return tuple(batch[:6]) + (self._depth_sup_outputs(batch),)
    return tuple(batch[:6])

  def stage(self, batch):
    """Images to the device; the two src->trg projection matrices are built on
    the host (tiny), kept there for the kernel-family choice and copied to the
    device.  plan = what the renderer would choose for these cameras."""
    imgs_src, imgs_trg, k_s, k_t, rot_mat, trans_mat = batch[:6]
    f32 = lambda t: t.detach().to('cpu', torch.float32)
    k_s, k_t, rot_mat, trans_mat = f32(k_s), f32(k_t), f32(rot_mat), f32(trans_mat)
    inv_rot_mat = nn_helpers.transpose(rot_mat)
    inv_trans_mat = -torch.matmul(inv_rot_mat, trans_mat)
    mat_trg = projection.forward_projection_matrix(k_s, k_t, rot_mat, trans_mat)
    mat_src = projection.forward_projection_matrix(k_t, k_s, inv_rot_mat,
                                                   inv_trans_mat)
    self.host_mats = {'trg': mat_trg.contiguous(), 'src': mat_src.contiguous()}
    plan = None
    if self.device.type == 'cuda':
      o = self.opts
      plan = tuple(
          ldi_utils.plan_key((o.n_layers, imgs_src.shape[0], o.img_height,
                              o.img_width), o.trg_splat_downsampling,
                             o.max_disp, self.host_mats[w])
          for w in ('trg', 'src'))
    dev = self.device

    def up(t):
      # A pageable host-to-device copy blocks the host until the GPU has drained
      # the kernels queued before it -- once per step that serialises the step's
      # launches with the previous step's kernels (eager training: 12 ms per step
      # instead of 10).  Through pinned memory the copy is asynchronous.
      if dev.type == 'cuda' and not t.is_cuda:
        return t.pin_memory().to(dev, non_blocking=True)
      return t.to(dev)
    staged = [up(imgs_src), up(imgs_trg), up(mat_trg), up(mat_src)]
    if getattr(self, 'gt_disps', None) is not None:
      # (part of the staged batch: a captured HIP graph replays on static copies)
      staged += [self.gt_disps[0].to(dev), self.gt_disps[1].to(dev)]
    if len(batch) > 6:
      staged += self._stage_depth_sup(batch[6], k_s, k_t, trans_mat, up)
    return staged, plan

  def _stage_depth_sup(self, outputs, k_s, k_t, trans_mat, up):
    """The depth-supervision ground truth of a batch, on the device: [gt] or
    [gt, gt_scale], gt 2 B x H x W x 1 -- the source views', then the target
    views' -- in the conventions of Evaluator.eval_depth."""
    o = self.opts
    if outputs[0] == 'planes':   # inverse depths already
      return [torch.cat([up(outputs[1].float()), up(outputs[2].float())], dim=0)]
    if outputs[0] == 'px':
      # pixel disparities d = f_x |t_x| / depth, each view with its own intrinsics
      t_x = trans_mat[:, 0, 0].abs()
      scale = torch.cat([1.0 / (k_s[:, 0, 0] * t_x), 1.0 / (k_t[:, 0, 0] * t_x)])
      # (the device route's sampling launch wrote [gt_src; gt_trg] as one tensor)
      both = _halves_of(outputs[1], outputs[2])
      if both is None:
        both = torch.cat([up(outputs[1].float()), up(outputs[2].float())], dim=0)
      return [up(both), up(scale.float())]
    # the scans rasterised into both views as inverse depths, 0 = no return
    from lsi.geometry import lidar  # pylint: disable=g-import-not-at-top
    pts, counts, mats = outputs[1:]
    inv = lidar.rasterize_points(
        up(pts.float()), None, counts, up(mats.float()), o.img_height, o.img_width,
        z_min=o.depth_sup_min, z_max=o.depth_sup_max, inverse=True)
    return [torch.cat([inv[:, 0], inv[:, 1]], dim=0)]

  def compute_losses(self, staged):
    opts = self.opts
    if self.device.type != 'cuda':
      raise RuntimeError('the renderer and the six loss terms are HIP kernels: '
                         'training needs a ROCm device')
    imgs_src, imgs_trg, mat_trg, mat_src = staged[:4]
    amp = (torch.autocast('cuda', dtype=torch.bfloat16) if opts.bf16
           else contextlib.nullcontext())
    if hasattr(self, 'model'):
      self.model.pair_ldi = None
    with amp:
      ldi_src, ldi_trg = self.train_model(imgs_src, imgs_trg)
    if opts.debug_synth_texture and len(staged) >= 6:
      # ldi_enc_dec.py:223-225: keep the graph, substitute the values
      ldi_src[2] = 0 * ldi_src[2] + staged[4]
      ldi_trg[2] = 0 * ldi_trg[2] + staged[5]

    # The pair as one buffer of 2 B views where the network made one (and no
    # ground-truth disparities were substituted into its halves), else one
    # group of views per direction: lsi/loss/objective.py
    pair = getattr(getattr(self, 'model', None), 'pair_ldi', None)
    if not getattr(opts, 'paired_splat', True) or (
        opts.debug_synth_texture and len(staged) >= 6):
      pair = None
    coef = objective.loss_coefficients(opts)
    source, gt = getattr(self, 'depth_sup_source', None), (None, None)
    if 'depth_sup' in coef:
      if source is None:
        raise ValueError('--depth_sup_wt > 0 needs ground-truth depth from: ' +
                         DEPTH_SUP_SOURCES)
      gt = staged[-2:] if source == 'px' else (staged[-1], None)
    groups, halves = objective.view_groups(
        ldi_src, ldi_trg, pair, (imgs_src, imgs_trg), (mat_trg, mat_src),
        (self.host_mats['trg'], self.host_mats['src']), gt)
    return objective.objective(groups, halves, opts, coef, source)


def main(argv=None):
  opts = apply_dataset_overrides(build_parser().parse_args(argv))
  trainer = Trainer(opts)
  trainer.setup()
  try:
    trainer.train()
  finally:
    close = getattr(trainer.data_loader, 'close', None)
    if close is not None:
      close()  # a prefetching loader's decode threads
  if trainer.dist is not None:
    trainer.dist.destroy_process_group()
  return trainer


if __name__ == '__main__':
  main()
