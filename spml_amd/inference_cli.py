"""Shared body of the seventeen inference programs under `pyscripts/inference/`: the reference's command line and config
surface (`parse_args`), the argument guards, snapshot loading, the seeded synthetic images that stand in for the
file-list loader (outside this repository, DESIGN 9: `--data_list synthetic`), the self-built memory bank of the kNN
programs, the timed loop over the images and the JSON line.  A program's `main` holds what is specific to its recipe:
which `spml_amd.inference` function it calls, with which extra inputs, and which fields it adds to the report.  The two
memory-bank programs (`prototype.py`, `prototype_msc.py`) and the two softmax pseudo-label programs (`pseudo_softmax.py`,
`pseudo_softmaxrw.py`) differ in constants only; their bodies are `run_prototypes` and `run_pseudo_softmax` below."""
import json
import os
import time

import numpy as np
import torch

NUM_SYNTHETIC_IMAGES = 4          # read at call time: the tests shorten the programs by patching this attribute
NUM_LABEL_VALUES = 256            # label maps hold classes and the ignore value 255 (prototype_msc.py:189-192)


def parse(description, argv, api_function, what='inference'):
  """`parse_args`, the reference's `--kmeans_num_clusters` / `--label_divisor` overrides (inference_msc.py:40-41; the
  softmax programs read neither), then the guards, in one order for every program: a file list, a missing `--save_dir`,
  a machine without a GPU.  -> (config, args, device), with `device` made the current one."""
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args(description, argv)
  if args.kmeans_num_clusters:
    config.network.kmeans_num_clusters = [int(i) for i in args.kmeans_num_clusters.split(',')]
  if args.label_divisor:
    config.network.label_divisor = args.label_divisor
  if args.data_list not in (None, 'synthetic'):
    raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                     'use --data_list synthetic or call spml_amd.inference.%s on your own images' % api_function)
  if not args.save_dir:
    raise SystemExit('--save_dir is required')
  if not torch.cuda.is_available():
    raise SystemExit('%s needs an MI355X (the HIP path has no CPU fallback)' % what)
  device = torch.device('cuda', 0)
  torch.cuda.set_device(device)
  return config, args, device


def output_dir(args, name):
  path = os.path.join(args.save_dir, name)
  os.makedirs(path, exist_ok=True)
  return path


def geometry(config):
  """-> (num_classes, crop_size, stride, side of the square synthetic images) of the `test` section."""
  crop_size, stride = tuple(config.test.crop_size), tuple(config.test.stride)
  size = config.test.image_size if config.test.image_size > 0 else crop_size[0]
  return config.dataset.num_classes, crop_size, stride, size


def embedding_makers(densepose=False):
  """`backbone_types` -> constructor of the embedding network.  `densepose`: the PSPNet is the DensePose recipe's
  (location + colour local features), as `pseudo_denseposerw_crf.py:21` imports it."""
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  if densepose:
    from spml_amd.models.embeddings.resnet_pspnet_densepose import resnet_101_pspnet
  else:
    from spml_amd.models.embeddings.resnet_pspnet import resnet_101_pspnet
  return {'panoptic_pspnet_101': resnet_101_pspnet, 'panoptic_deeplab_101': resnet_101_deeplab}


def load_models(config, args, device, head, densepose=False):
  """The embedding network (channels-last, `eval()`; `densepose`: see `embedding_makers`) and, for `head` 'segsort' or
  'softmax_classifier', the prediction model, both from `model-{max_iteration-1}.pth` of the snapshot directory: `embedding_model` through the reference's name
  mapping (`resume=True`); a segsort head strictly; a classifier head non-strictly from the `semantic_classifier.*`
  entries -- a stage-1 `SegsortSoftmax` snapshot carries the same names next to entries that model does not have.
  -> (embedding_model, prediction_model or None, snapshot path)."""
  makers = embedding_makers(densepose)
  if config.network.backbone_types not in makers:
    raise ValueError('Not support ' + str(config.network.backbone_types))
  if head == 'segsort' and config.network.prediction_types != 'segsort':
    raise ValueError('Not support ' + str(config.network.prediction_types))
  embedding_model = makers[config.network.backbone_types](config).to(device).to(memory_format=torch.channels_last)
  embedding_model.eval()
  prediction_model = None
  if head == 'segsort':
    from spml_amd.models.predictions.segsort import segsort
    prediction_model = segsort(config).to(device).eval()
  elif head == 'softmax_classifier':
    from spml_amd.models.predictions.softmax_classifier import softmax_classifier
    prediction_model = softmax_classifier(config).to(device).eval()
  path = os.path.join(args.snapshot_dir, 'model-{:d}.pth'.format(config.train.max_iteration - 1))
  state = torch.load(path, map_location=device, weights_only=True)
  embedding_model.load_state_dict(state['embedding_model'], resume=True)
  if head == 'segsort':
    prediction_model.load_state_dict(state['prediction_model'])
  elif head == 'softmax_classifier':
    entries = {k: v for k, v in state['prediction_model'].items() if k.startswith('semantic_classifier.')}
    missing = torch.nn.Module.load_state_dict(prediction_model, entries, strict=False).missing_keys
    if missing:
      raise ValueError('%s has no classifier head (missing %s)' % (path, ', '.join(missing)))
  return embedding_model, prediction_model, path


def synthetic_image(index, size, num_classes, device):
  """-> (image [1,3,S,S] float, semantic label [S,S], instance label [S,S]) of seeded synthetic image `index`: one to
  three object classes per image, as many as `num_classes` has."""
  from spml_amd import synth
  datas, targets = synth.make_batch(1, size, num_classes=num_classes, seed=4099 + index, device=device,
                                    palette=(1, max(1, min(3, num_classes - 1))))
  return datas['image'].float(), targets['semantic_label'][0], targets['instance_label'][0]


def dense_label(label, num_classes, empty_fill=None):
  """The synthetic generator keeps ~10 % of the labels (scribbles) and the memory-bank pass needs dense ones: every pixel
  at or above `num_classes` (the unlabelled value 254 and the ignore strip) takes the image's most frequent labelled
  class (its ground truth up to 171 pixels: one class per 171-pixel cell).  A small image may keep no labelled pixel at
  all, and the programs differ there: the kNN programs' own bank leaves such a map as it is (`empty_fill=None`), the
  memory-bank programs ignore the image as a whole (`empty_fill` = the ignore index everywhere), so that no prototype
  enters a bank file under the unlabelled value -- the retrieval side drops the ignore label and nothing else.  Both
  policies are kept as the programs had them: which of them a tiny image hits depends on the device's random stream."""
  labelled = label[label < num_classes]
  if labelled.numel():
    return torch.where(label < num_classes, label, torch.mode(labelled).values)
  return label if empty_fill is None else torch.full_like(label, empty_fill)


def build_synthetic_bank(embedding_model, config, args, device):
  """The synthetic mode on its own, without `--semantic_memory_dir`: the memory-bank pass over the synthetic images
  (prototype.py:107-211, through `full_resolution_prototypes`), written with `save_image_memory` to
  `<save_dir>/semantic_prototype`.  -> that directory."""
  from spml_amd import inference
  num_classes, crop_size, stride, size = geometry(config)
  memory_dir = output_dir(args, 'semantic_prototype')
  for index in range(NUM_SYNTHETIC_IMAGES):
    image, label, _ = synthetic_image(index, size, num_classes, device)
    padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]
    prototypes, prototype_labels, _ = inference.full_resolution_prototypes(
        embedding_model, padded, dense_label(label, num_classes), crop_size, stride, config.dataset.semantic_ignore_index)
    inference.save_image_memory(os.path.join(memory_dir, 'synthetic_{:04d}.npy'.format(index)), prototypes,
                                prototype_labels)
  return memory_dir


def load_bank(memory_dir, config, device):
  """The memory bank of a directory on the device, the ignore class dropped (inference_msc.py:92-111)."""
  from spml_amd import inference
  import spml_amd.utils.segsort.others as segsort_others
  prototypes, prototype_labels = segsort_others.load_memory_banks(memory_dir)
  return inference.drop_ignored_memory(prototypes.to(device), prototype_labels.to(device),
                                       config.dataset.semantic_ignore_index)


def timed_images(per_image):
  """`per_image(index)` for every synthetic image, between two device synchronisations -> (images done, seconds)."""
  done = 0
  torch.cuda.synchronize()
  t0 = time.time()
  for index in range(NUM_SYNTHETIC_IMAGES):
    per_image(index)
    done += 1
  torch.cuda.synchronize()
  return done, time.time() - t0


def save_label_map(directory, index, prediction):
  np.save(os.path.join(directory, 'synthetic_{:04d}.npy'.format(index)), prediction.to(torch.uint8).cpu().numpy())


def scores(counts):
  """`iou_stats` counts -> the `mIoU` / `pixel_acc` fields of the report (benchmark_by_mIoU.py)."""
  from spml_amd.utils.general import metrics
  result = metrics.mean_iou(counts)
  return {'mIoU': round(result['mean_iou'], 4), 'pixel_acc': round(result['pixel_acc'], 4)}


def report(done, seconds, **fields):
  print(json.dumps({'images': done, 'images_per_s': round(done / seconds, 3), **fields}))


def run_prototypes(description, scales, argv=None):
  """`prototype.py` and `prototype_msc.py` (`prototype_msc.py:34-207` of twke18/SPML): every image through
  `spml_amd.inference.multiscale_prototypes`; the programs differ in the scales of the image pyramid only (`[1]` against
  `[0.5, 1, 1.5]`, no flip in either).  The bank of every image is written to `<save_dir>/semantic_prototype/<name>.npy`
  in the reference's on-disk format, where `inference.py` / `inference_msc.py --semantic_memory_dir` read it."""
  from spml_amd import inference
  config, args, device = parse(description, argv, 'multiscale_prototypes', 'memory-bank generation')
  prototype_dir = output_dir(args, 'semantic_prototype')                                          # :43-44
  embedding_model, _, path = load_models(config, args, device, None)                              # :69-79
  num_classes, crop_size, stride, size = geometry(config)
  ignore_index = config.dataset.semantic_ignore_index
  per_image, out, views = [], None, []

  def one(index):
    nonlocal out, views
    image, label, _ = synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, scales, False, crop_size)                           # :92-95
    labels = inference.label_views(dense_label(label, num_classes, ignore_index), [hw for _, hw, _ in views])
    out = inference.multiscale_prototypes(embedding_model, views, labels, crop_size, stride, ignore_index,
                                          NUM_LABEL_VALUES)
    inference.save_image_memory(os.path.join(prototype_dir, 'synthetic_{:04d}.npy'.format(index)), out['prototype'],
                                out['prototype_label'])                                           # :200-207
    per_image.append(int(out['prototype'].shape[0]))

  done, seconds = timed_images(one)
  report(done, seconds, prototypes_per_image=per_image, views=len(views), scales=list(scales),
         majority_path=out['majority_path'], snapshot=path, save_dir=prototype_dir)


def run_pseudo_softmax(description, scales, combine, walk_steps, argv=None):
  """`pseudo_softmax.py` and `pseudo_softmaxrw.py` (`pseudo_softmaxrw_crf.py:33-204` of twke18/SPML): every image through
  `spml_amd.inference.pseudo_labels_softmax`; the programs differ in three constants only (scales of the image pyramid,
  how the views' class scores are combined, squarings of the transition matrix).  The label maps of the synthetic images
  give the image tags (:102-106) and the mIoU of the JSON line; the labels written are those of :176, before the denseCRF
  refinement (built for other programs; for these two it is the follow-up named there)."""
  from spml_amd import inference
  from spml_amd.utils.general import metrics
  config, args, device = parse(description, argv, 'pseudo_labels_softmax')
  semantic_dir = output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = load_models(config, args, device, 'softmax_classifier')
  num_classes, crop_size, _, size = geometry(config)
  counts, out = None, None

  def one(index):
    nonlocal counts, out
    image, label, _ = synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, scales, True, crop_size)                            # :109-125
    out = inference.pseudo_labels_softmax(embedding_model, prediction_model, views, (size, size),
                                          inference.label_tags_from_map(label, num_classes), combine=combine,
                                          walk_steps=walk_steps)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = timed_images(one)
  report(done, seconds, **scores(counts), scales=list(scales), is_flip=True, combine=combine, walk_steps=walk_steps,
         head_path=out['head_path'], snapshot=path, save_dir=semantic_dir)


class CrfStage(object):
  """The denseCRF stage of the `*_crf*.py` programs: the reference's `postprocessor` built from the six `--crf_*` options
  (inference_softmax_crf_msc.py:80-87) and device events around every call, for the stage's share of the image time."""

  def __init__(self, config, args):
    from spml_amd.models.crf import DenseCRF
    self.crf = DenseCRF(iter_max=args.crf_iter_max, pos_xy_std=args.crf_pos_xy_std, pos_w=args.crf_pos_w,
                        bi_xy_std=args.crf_bi_xy_std, bi_rgb_std=args.crf_bi_rgb_std, bi_w=args.crf_bi_w)
    self.pixel_means, self.pixel_stds = config.network.pixel_means, config.network.pixel_stds
    self.events, self.path = [], None

  def image_u8(self, image, valid_hw):
    """The uint8 image the reference rebuilds from the network's input (:159-164), cropped to the un-padded size."""
    from spml_amd import inference
    h, w = valid_hw
    return inference.denormalized_uint8(image, self.pixel_means, self.pixel_stds)[:h, :w].contiguous()

  def __call__(self, image_u8, prob):
    from spml_amd import inference
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = inference.dense_crf_refine(image_u8, prob, self.crf)
    end.record()
    self.events.append((start, end))
    self.path = out['crf_path']
    return out

  def refine_upsampled(self, image_u8, lowres):
    """The fused call of the random-walk programs (`DenseCRF.refine_upsampled`: the low-resolution walked maps are
    up-sampled inside the CRF's first kernel) between the same device events.  With this method and `path_name` the stage
    stands in for its `DenseCRF` as the `crf` of `inference.random_walk_crf_refine` and `pseudo_labels_softmax_crf`, so
    the events enclose the CRF alone and not the network and the walk in front of it."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = self.crf.refine_upsampled(image_u8, lowres)
    end.record()
    self.events.append((start, end))
    return out

  def _timed(self, call, *args):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call(*args)
    end.record()
    self.events.append((start, end))
    return out

  def refine_votes(self, image_u8, clu, topk, ncls):
    """The fused call of the kNN program (`DenseCRF.refine_votes`: the vote map is gathered from a per-segment table
    inside the CRF's first kernel) between the same device events, so that the stage stands in for its `DenseCRF` as the
    `crf` of `inference.knn_votes_crf_refine` and `predict_knn_full_resolution_crf`; `refine` is the route of that
    function outside the kernel's limits."""
    return self._timed(self.crf.refine_votes, image_u8, clu, topk, ncls)

  def refine(self, image_u8, prob):
    return self._timed(self.crf.refine, image_u8, prob)

  def path_name(self, h, w, ncls):
    self.path = self.crf.path_name(h, w, ncls)
    return self.path

  def fields(self, seconds):
    """Read after the loop's closing synchronisation: `crf_path` and the stage's share of the timed seconds."""
    ms = sum(a.elapsed_time(b) for a, b in self.events)
    return {'crf_path': self.path, 'crf_share': round(ms / (seconds * 1e3), 4)}
