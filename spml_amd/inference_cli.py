"""Shared body of the seventeen inference programs under `pyscripts/inference/`: the reference's command line and config
surface (`parse_args`), the argument guards, snapshot loading, where the images come from and the label maps go
(`ImageSource`: the seeded synthetic images of `--data_list synthetic`, or the reference's file list with the views made
and the label images finished on the GPU, DESIGN 8o -- eight programs so far, the other nine still refuse a list), the
self-built memory bank of the kNN programs, the timed loop over the images and the JSON line.  A program's `main` holds what is specific to its recipe:
which `spml_amd.inference` function it calls, with which extra inputs, and which fields it adds to the report.  The two
memory-bank programs (`prototype.py`, `prototype_msc.py`) differ in constants only; their body is `run_prototypes`.
The label-inference and softmax pseudo-label programs come in pairs, `X.py` and `X_crf.py`: the pair shares one body
(`run_softmax`, `run_knn`, `run_pseudo_softmax`) with the denseCRF stage (`CrfStage`) on or off.  `X.py` reads file
lists and takes `--crf`; `X_crf.py` runs the same body with the CRF always on and refuses a list, so the CRF of those five
programs reaches image files through `X.py --crf`: the source then adds the CRF's guide image to every
`SourceImage` (`spml_crf_guide_u8` from the bytes already on the device) and `emit_refined` finishes, scores (after and
before the CRF) and compares the label maps in one launch (`spml_label_export_scored_u8`).  `pseudo_softmax.py` runs
`run_pseudo_softmax` too; it has no CRF sibling in the reference and takes no `--crf`.  The image-tag recipe's two
pseudo-label steps reach image files the same way: `pseudo_softmaxrw.py --cam_dir` is the CAM walk of
`pseudo_camrw_crf.py` (the source adds the planes of every image's CAM file to its upload, `run_pseudo_softmax` calls
`pseudo_labels_cam[_crf]`), `inference_msc.py --pseudo_tags` the kNN pseudo labels of `pseudo_inference[_crf]_msc.py`
(`run_knn` with that program's scales, the image tags and `pseudo_labels_knn_multiscale`)."""
import collections
import json
import os
import time

import numpy as np
import torch

NUM_SYNTHETIC_IMAGES = 4          # read at call time: the tests shorten the programs by patching this attribute
NUM_LABEL_VALUES = 256            # label maps hold classes and the ignore value 255 (prototype_msc.py:189-192)


def reads_file_list(args):
  return args.data_list not in (None, 'synthetic')


def list_dataset(config, args, api_function, need_labels=False):
  """The reference's evaluation dataset (inference_softmax.py:45-54) over `--data_dir` (or `dataset.data_dir`) and
  `--data_list`.  A list that does not exist, or one without label columns under a program that needs them, ends the
  program."""
  from spml_amd.data.datasets import ListDataset
  if not os.path.isfile(args.data_list):
    raise SystemExit("data list '%s' does not exist (ListDataset reads 'image [semantic_label instance_label]' per "
                     'line); use --data_list synthetic or call spml_amd.inference.%s on your own images'
                     % (args.data_list, api_function))
  data_dir = args.data_dir if args.data_dir is not None else (config.dataset.data_dir or '')
  dataset = ListDataset(data_dir=data_dir, data_list=args.data_list, img_mean=config.network.pixel_means,
                        img_std=config.network.pixel_stds, size=None, random_crop=False, random_scale=False,
                        random_mirror=False, training=False)
  if len(dataset) < 1:
    raise SystemExit("data list '%s' is empty" % args.data_list)
  if need_labels and not dataset.semantic_label_paths:
    raise SystemExit("data list '%s' has no label columns: this program reads the semantic label of every image "
                     "('image semantic_label instance_label' per line)" % args.data_list)
  return dataset


def parse(description, argv, api_function, what='inference', file_lists=None, crf_option=False, pseudo_tags_option=False):
  """`parse_args`, the reference's `--kmeans_num_clusters` / `--label_divisor` overrides (inference_msc.py:40-41; the
  softmax programs read neither), then the guards, in one order for every program: a file list, a missing `--save_dir`,
  a machine without a GPU.  `file_lists`: None for a program that does not read file lists yet (it refuses one),
  'images' for one that does, 'labels' for one that also needs the list's label columns, or a function of the parsed
  arguments that gives one of the three (a program whose options decide).  `crf_option`: the program takes `--crf` (the
  denseCRF tail of its `*_crf*` sibling); `pseudo_tags_option`: it takes `--pseudo_tags`.
  -> (config, args, device), with `device` made the current one."""
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args(description, argv, crf_option, pseudo_tags_option)
  if args.kmeans_num_clusters:
    config.network.kmeans_num_clusters = [int(i) for i in args.kmeans_num_clusters.split(',')]
  if args.label_divisor:
    config.network.label_divisor = args.label_divisor
  if callable(file_lists):
    file_lists = file_lists(args)
  if reads_file_list(args):
    if file_lists is None:
      raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                       'use --data_list synthetic or call spml_amd.inference.%s on your own images' % api_function)
    list_dataset(config, args, api_function, need_labels=file_lists == 'labels')
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


class SourceImage(object):
  """One image of an `ImageSource`: `index`, `name` (of its output files, without a directory), `image_hw` (the size the
  label map is scored and written at), `views` (`(image [1,3,Hp,Wp], (rh, rw), is_flip)`, what the `predict_*` /
  `pseudo_*` functions take), `label_views` (the label `[rh, rw]` of every view; a source with labels only) and `label`
  (the semantic label `[h, w]` on the device, or None).  A source made `with_guide` adds `guide`, the uint8 image
  `[rh, rw, 3]` the denseCRF takes, at the resolution the CRF runs at: the file's own size for the multi-view programs
  (inference_softmax_crf_msc.py:159-164 uses the original image), the un-padded `test.image_size` view for a
  `single_view` one (inference_crf.py:247-252).  A source made `with_cams` adds `cam_planes` (fp32 `[K,h,w]` on the
  device, the planes of the image's CAM file, None for a file without entries) and `cam_classes` (their K dict keys,
  class - 1, as host integers: `spml_cam_ingest_f32` checks them on the host).  `instance`: the instance label `[h, w]`
  of a synthetic image, None for a file (`ListImageSource` does not upload the instance plane)."""

  def __init__(self, index, name, image_hw, views, label_views, label, guide=None, cam_planes=None, cam_classes=None,
               instance=None):
    self.index, self.name, self.image_hw = index, name, image_hw
    self.views, self.label_views, self.label, self.guide = views, label_views, label, guide
    self.cam_planes, self.cam_classes, self.instance = cam_planes, cam_classes, instance


def read_cam_file(cam_dir, name, image_hw, num_classes):
  """`<cam_dir>/<name>`, the reference's pickled dict `{class - 1: [h, w]}` (pseudo_camrw_crf.py:106-107)
  -> (keys int32 `[K]`, the K planes as a list of contiguous fp32 `[h, w]` arrays), in the dict's order; a plane the file
  holds as contiguous fp32 is the file's own array, so the caller's copy to where the planes go up from is the only one.
  A file that does not exist, a plane that does not have the image's shape or a key outside `0 .. num_classes - 2` ends
  the program with a message that names the file."""
  path = os.path.join(cam_dir, name)
  if not os.path.isfile(path):
    raise SystemExit("CAM file '%s' does not exist (--cam_dir holds one pickled {class - 1: [h, w]} dict per image)" % path)
  cams = np.load(path, allow_pickle=True).item()
  h, w = image_hw
  keys, planes = np.empty((len(cams),), np.int32), []
  for i, (key, value) in enumerate(cams.items()):
    if not 0 <= int(key) <= num_classes - 2:
      raise SystemExit("CAM file '%s' has the key %d: outside 0 .. %d (class - 1 of %d classes)"
                       % (path, int(key), num_classes - 2, num_classes))
    if tuple(np.shape(value)) != (h, w):
      raise SystemExit("CAM file '%s': the plane of key %d is %s, the image is %d x %d"
                       % (path, int(key), ' x '.join(str(s) for s in np.shape(value)), h, w))
    keys[i] = int(key)
    planes.append(np.ascontiguousarray(value, dtype=np.float32))
  return keys, planes


class ImageSource(object):
  """Where a program's images come from and where its label maps go: one interface, two implementations, so that a
  program's `main` does not branch.  `scales` / `is_flip`: the views of every image; `single_view`: the program resizes
  to `test.image_size` first (inference_softmax.py:89-94) and its label map goes back to the file's size; `with_labels`:
  every view comes with its label map (the memory-bank pass); `with_guide`: every image comes with the denseCRF's guide;
  `with_cams`: a directory of CAM files, every image comes with the planes and keys of its file (`read_cam_file`).

    for_program(...)        the implementation `--data_list` selects
    timed(per_image)        `per_image(SourceImage)` for every image, between two synchronisations -> (done, seconds)
    write(image, out, directory)
                            the label writer of the programs: `emit` of a per-image result, `emit_refined` of one that
                            carries the labels before the denseCRF
    emit(image, prediction, directory)
                            scores the label map `[h, w]` against the image's label and writes it
    emit_refined(image, refined, before, directory)
                            the same for the labels after the denseCRF; the labels before it are scored too and the
                            pixels the CRF changed are counted, all at the size `emit` scores at
    bank_name(image)        file name of the image's memory bank
    scores()                the `mIoU` / `pixel_acc` fields of the report
    crf_fields()            `mIoU_before_crf` and `changed_by_crf` of the report, after `emit_refined`
    fields()                further fields of the report"""

  def __init__(self, config, args, device, scales, is_flip, single_view=False, with_labels=False, with_guide=False,
               with_cams=None):
    self.config, self.args, self.device = config, args, device
    self.scales, self.is_flip, self.single_view, self.with_labels = list(scales), bool(is_flip), single_view, with_labels
    self.with_guide, self.with_cams = with_guide, with_cams
    self.num_classes, self.crop_size, self.stride, self.size = geometry(config)
    self.counts, self.counts_before, self.changed, self.pixels = None, None, None, 0

  @staticmethod
  def for_program(config, args, device, scales, is_flip, api_function, **kind):
    if reads_file_list(args):
      return ListImageSource(config, args, device, scales, is_flip, api_function, **kind)
    return SyntheticImageSource(config, args, device, scales, is_flip, **kind)

  def tags(self, image):
    """The image tags of the pseudo-label programs (pseudo_softmaxrw_crf.py:102-106)."""
    from spml_amd import inference
    return inference.label_tags_from_map(image.label, self.num_classes)

  def write(self, image, out, directory):
    """`out`: what a `spml_amd.inference` function returned for `image` (or `refined_by` made of it).  Its
    `semantic_prediction` is written; where it holds `semantic_prediction_before_crf` the run has a denseCRF stage."""
    before = out.get('semantic_prediction_before_crf')
    if before is None:
      self.emit(image, out['semantic_prediction'], directory)
    else:
      self.emit_refined(image, out['semantic_prediction'], before, directory)

  def score(self, prediction, label):
    from spml_amd.utils.general import metrics
    self.counts = metrics.iou_stats(prediction, label, self.num_classes, self.counts)

  def scores(self):
    return {'mIoU': None, 'pixel_acc': None} if self.counts is None else scores(self.counts)

  def crf_fields(self):
    """Read after the loop's closing synchronisation."""
    before = None if self.counts_before is None else scores(self.counts_before)['mIoU']
    changed = 0 if self.changed is None else int(self.changed)
    return {'mIoU_before_crf': before, 'changed_by_crf': round(changed / float(max(self.pixels, 1)), 4)}

  def fields(self):
    return {}


class SyntheticImageSource(ImageSource):
  """`--data_list synthetic` (or none): `synthetic_image` + `flip_scale_views` (+ `label_views` of the densified label),
  label maps as `.npy` (`save_label_map`); `with_cams`: the CAM file of image `index` is `synthetic_%04d.npy`, the name
  `pseudo_camrw_crf.py` reads."""

  def image(self, index):
    from spml_amd import inference
    image, label, instance = synthetic_image(index, self.size, self.num_classes, self.device)
    views = inference.flip_scale_views(image, self.scales, self.is_flip, self.crop_size)
    labels = None
    if self.with_labels:
      dense = dense_label(label, self.num_classes, self.config.dataset.semantic_ignore_index)
      labels = inference.label_views(dense, [hw for _, hw, _ in views])
    guide = None
    if self.with_guide:         # (a single view's padded image holds `image` in its top-left corner: one guide for both)
      guide = inference.denormalized_uint8(image, self.config.network.pixel_means, self.config.network.pixel_stds)
    name = 'synthetic_{:04d}'.format(index)
    planes, keys = None, None
    if self.with_cams:
      keys, planes = read_cam_file(self.with_cams, name + '.npy', (self.size, self.size), self.num_classes)
      planes = torch.from_numpy(np.stack(planes)).to(self.device) if len(keys) else None
    return SourceImage(index, name, (self.size, self.size), views, labels, label, guide, planes, keys, instance)

  def timed(self, per_image):
    return timed_images(lambda index: per_image(self.image(index)))

  def emit(self, image, prediction, directory):
    self.score(prediction, image.label)
    save_label_map(directory, image.index, prediction)

  def emit_refined(self, image, refined, before, directory):
    from spml_amd.utils.general import metrics
    if self.changed is None:
      self.changed = torch.zeros((), dtype=torch.int64, device=self.device)
    self.score(refined, image.label)
    self.counts_before = metrics.iou_stats(before, image.label, self.num_classes, self.counts_before)
    self.changed.add_((refined != before).sum())
    self.pixels += refined.numel()
    save_label_map(directory, image.index, refined)

  def bank_name(self, image):
    return image.name + '.npy'


def output_name(image_path):
  """inference.py:117: the base name of the image, `.jpg` -> `.png`."""
  return os.path.basename(image_path).replace('.jpg', '.png')


def write_label_pngs(gray_path, color_path, gray, color):
  """inference.py:243-255."""
  import PIL.Image as Image
  for path, array, mode in ((gray_path, gray, 'L'), (color_path, color, 'RGB')):
    if not os.path.isdir(os.path.dirname(path)):
      os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array, mode=mode).save(path)


UploadLayout = collections.namedtuple('UploadLayout', 'records_end rgb_at sem_at sem_end cam_at total')


def upload_layout(records_nbytes, h, w, has_semantic, num_cam_planes):
  """Where the parts of an image's one upload lie, in bytes: the view records `[0, records_end)`, the RGB bytes from
  `rgb_at`, the semantic plane `[sem_at, sem_end)` (empty without one) and the fp32 CAM planes from `cam_at` (None
  without planes) to `total`.  Every part starts on a multiple of 16: the kernels read the records and the image with
  wide loads and the planes as fp32."""
  def aligned(nbytes):
    return (nbytes + 15) // 16 * 16
  rgb_at = aligned(records_nbytes)
  sem_at = rgb_at + aligned(3 * h * w)
  sem_end = sem_at + (h * w if has_semantic else 0)
  if not num_cam_planes:
    return UploadLayout(records_nbytes, rgb_at, sem_at, sem_end, None, sem_end)
  cam_at = aligned(sem_end)
  return UploadLayout(records_nbytes, rgb_at, sem_at, sem_end, cam_at, cam_at + 4 * h * w * num_cam_planes)


class ListImageSource(ImageSource):
  """`--data_dir D --data_list L`: the files of `ListDataset(training=False)`, decoded ahead on a thread pool (threads,
  never processes: a forked child of a process that holds the GPU is not safe); the raw bytes and the view records go
  up from pinned memory in ONE `non_blocking` copy and `spml_image_views_u8` makes every view from them
  (`spml_amd.inference.views_from_records`); `spml_label_export_u8` writes the finished gray and colour bytes at the
  file's own size, one copy brings them into pinned memory and a writer pool saves `semantic_gray/<name>.png` (mode L)
  and `semantic_color/<name>.png` (mode RGB).  `with_guide`: `spml_crf_guide_u8` forms the denseCRF's guide from the
  bytes already on the device, and `emit_refined` finishes, scores (after and before the CRF) and compares in one launch
  (`spml_label_export_scored_u8`); the counts of the whole list stay in one device tensor.  `with_cams`: the
  reader thread also loads `<cam_dir>/<name with .png -> .npy>` (pseudo_camrw_crf.py:97,106) and the fp32 planes go up in
  the same copy, 16-byte aligned behind the semantic plane."""

  AHEAD = 4        # images decoded ahead of the one on the GPU

  def __init__(self, config, args, device, scales, is_flip, api_function, **kind):
    from concurrent.futures import ThreadPoolExecutor
    from spml_amd import inference
    from spml_amd.utils.general import vis
    ImageSource.__init__(self, config, args, device, scales, is_flip, **kind)
    self.dataset = list_dataset(config, args, api_function, need_labels=self.with_labels)
    self.has_labels = bool(self.dataset.semantic_label_paths)
    self.image_size = config.test.image_size if self.single_view else 0
    threads = max(1, min(int(config.num_threads), 4))
    self.readers, self.writers = ThreadPoolExecutor(max_workers=threads), ThreadPoolExecutor(max_workers=threads)
    self.pending = []
    path = config.dataset.color_map_path
    self.color_map = torch.from_numpy(vis.load_color_map(path) if path else vis.voc_color_map()).to(device)
    self.mean, self.std = inference._normalisation(device, config.network.pixel_means, config.network.pixel_stds)
    self.staging = [None, None]         # pinned upload buffers, used in turn: [tensor, event of its last copy]
    self.turn = 0

  def __len__(self):
    return len(self.dataset)

  def decode(self, index):
    """On a reader thread: the decoded files and the view records of image `index`."""
    from spml_amd import inference
    from spml_amd.data import transforms
    rgb, semantic, _ = self.dataset.read(index)
    plan = transforms.plan_views(rgb.shape[0], rgb.shape[1], self.scales, self.is_flip, self.crop_size, self.image_size,
                                 name=self.dataset.image_paths[index])
    cams = None
    if self.with_cams:
      name = output_name(self.dataset.image_paths[index]).replace('.png', '.npy')
      cams = read_cam_file(self.with_cams, name, rgb.shape[:2], self.num_classes)
    return rgb, semantic, inference.view_records(plan), cams

  def _stage(self, nbytes):
    slot = self.staging[self.turn]
    if slot is not None:
      slot[1].synchronize()             # the copy that last read this buffer has finished
    if slot is None or slot[0].numel() < nbytes:
      slot = [torch.empty((nbytes + nbytes // 4,), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
      self.staging[self.turn] = slot
    self.turn ^= 1
    return slot

  def image(self, index, decoded):
    """On the main thread: pack (records, RGB, semantic plane, CAM planes), one copy, one launch."""
    from spml_amd import inference
    rgb, semantic, records, cams = decoded
    h, w = rgb.shape[:2]
    at = upload_layout(records.nbytes, h, w, semantic is not None, 0 if cams is None else len(cams[1]))
    stage, event = self._stage(at.total)
    host = stage.numpy()
    host[:at.records_end] = records.view(np.uint8).reshape(-1)
    host[at.rgb_at:at.rgb_at + 3 * h * w] = rgb.reshape(-1)
    if semantic is not None:
      host[at.sem_at:at.sem_end] = semantic.reshape(-1)
    if at.cam_at is not None:
      for i, plane in enumerate(cams[1]):
        host[at.cam_at + 4 * h * w * i:at.cam_at + 4 * h * w * (i + 1)] = plane.reshape(-1).view(np.uint8)
    packed = torch.empty((at.total,), dtype=torch.uint8, device=self.device)
    packed.copy_(stage[:at.total], non_blocking=True)
    event.record()
    rgb_dev = packed[at.rgb_at:at.rgb_at + 3 * h * w].view(h, w, 3)
    sem_dev = packed[at.sem_at:at.sem_end].view(h, w) if semantic is not None else None
    cam_dev = packed[at.cam_at:at.total].view(torch.float32).view(-1, h, w) if at.cam_at is not None else None
    views, labels = inference.views_from_records(rgb_dev, records, packed[:at.records_end], self.mean, self.std,
                                                 sem_dev if self.with_labels else None)
    guide = None
    if self.with_guide:
      guide = inference.crf_guide(rgb_dev, self.config.network.pixel_means, self.config.network.pixel_stds,
                                  views[0][1] if self.single_view else None)
    return SourceImage(index, output_name(self.dataset.image_paths[index]), (h, w), views, labels, sem_dev, guide, cam_dev,
                       None if cams is None else cams[0])

  def timed(self, per_image):
    n, done = len(self), 0
    torch.cuda.synchronize()
    t0 = time.time()
    ahead = [self.readers.submit(self.decode, i) for i in range(min(self.AHEAD, n))]
    try:
      for index in range(n):
        decoded = ahead.pop(0).result()
        if index + self.AHEAD < n:
          ahead.append(self.readers.submit(self.decode, index + self.AHEAD))
        per_image(self.image(index, decoded))
        done += 1
      self.drain()
    finally:
      for future in ahead:
        future.cancel()
      self.readers.shutdown(wait=True)
      self.writers.shutdown(wait=True)
    torch.cuda.synchronize()
    return done, time.time() - t0

  def _label_bytes(self, image):
    """The bytes of an image's two label files on the device -> (`[gray | colour]` uint8 `[4 * h * w]`, gray `[h, w]`,
    colour `[h, w, 3]`: views of it the export kernels write into)."""
    h, w = image.image_hw
    out = torch.empty((4 * h * w,), dtype=torch.uint8, device=self.device)
    return out, out[:h * w].view(h, w), out[h * w:].view(h, w, 3)

  def emit(self, image, prediction, directory):
    """`prediction` `[rh, rw]` (the un-padded view of a single-view program, else the file's size) -> the file's size
    (INTER_NEAREST; the identity where the sizes agree), scored there, written by the writer pool."""
    from spml_amd import inference
    h, w = image.image_hw
    out, gray, color = self._label_bytes(image)
    inference.export_label_map(prediction.contiguous(), tuple(prediction.shape), (h, w), self.color_map, out=(gray, color))
    if image.label is not None:
      self.score(gray, image.label)
    self._queue(image, out, directory)

  def emit_refined(self, image, refined, before, directory):
    """`emit` for the labels after the denseCRF (`refined`, `before`: `[rh, rw]` as there): one launch writes the bytes
    and adds both score tables and the changed pixels into `self.crf_scores`."""
    from spml_amd import inference
    h, w = image.image_hw
    n = self.num_classes
    out, gray, color = self._label_bytes(image)
    if self.changed is None:
      self.crf_scores = torch.zeros((2 * 3 * n + 1,), dtype=torch.int64, device=self.device)
      self.changed = self.crf_scores[-1]
    inference.export_scored_label_map(refined.contiguous(), before.contiguous(), tuple(refined.shape), (h, w),
                                      self.color_map, image.label, n, self.crf_scores, out=(gray, color))
    if image.label is not None:
      self.counts, self.counts_before = self.crf_scores[:3 * n].view(3, n), self.crf_scores[3 * n:-1].view(3, n)
    self.pixels += h * w
    self._queue(image, out, directory)

  def _queue(self, image, out, directory):
    """The finished bytes `[gray | colour]` of an image: one copy into pinned memory, then the writer pool."""
    h, w = image.image_hw
    host = torch.empty((4 * h * w,), dtype=torch.uint8, pin_memory=True)
    host.copy_(out, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    color_dir = os.path.join(os.path.dirname(os.path.normpath(directory)), 'semantic_color')
    self.pending.append(self.writers.submit(self._write, host, event, (h, w), os.path.join(directory, image.name),
                                            os.path.join(color_dir, image.name)))

  @staticmethod
  def _write(host, event, hw, gray_path, color_path):
    event.synchronize()
    h, w = hw
    array = host.numpy()
    write_label_pngs(gray_path, color_path, array[:h * w].reshape(h, w), array[h * w:].reshape(h, w, 3))

  def drain(self):
    """Waits for every file handed to the writer pool (a failed write raises here)."""
    pending, self.pending = self.pending, []
    for future in pending:
      future.result()

  def bank_name(self, image):
    return image.name.replace('.png', '.npy')                                                    # prototype.py:195-197

  def fields(self):
    return {'data_list': self.args.data_list, 'has_labels': self.has_labels}


def memory_bank_dir(embedding_model, config, args, device):
  """`--semantic_memory_dir`; without it the synthetic mode builds its own bank, a data list needs one."""
  if args.semantic_memory_dir is not None:
    return args.semantic_memory_dir
  if reads_file_list(args):
    raise SystemExit('--semantic_memory_dir is required with a data list (prototype.py / prototype_msc.py write one)')
  return build_synthetic_bank(embedding_model, config, args, device)


def run_loop(source, per_image):
  """The one timed loop of the programs: `per_image(SourceImage)` -> that image's result dict, for every image of
  `source` (`source.timed`).  -> (images done, seconds, the last image's result, the last image's views): what the
  report reads after the loop."""
  last = {'out': None, 'views': []}

  def one(image):
    last.update(out=per_image(image), views=image.views)

  done, seconds = source.timed(one)
  return done, seconds, last['out'], last['views']


def route_fields(out, views=None, constants=(), paths=(), instance_iou=None):
  """The fields of a report that depend on the route chosen before the loop, in the report's order: `views` (their
  number; None for a single-view route), the route's `constants` (name, value pairs), the `paths` its function names in
  its result -- read off `out`, the last image's -- and the instance-weighted IoU where the route kept one."""
  fields = {} if views is None else {'views': len(views)}
  fields.update(constants)
  fields.update((key, out[key]) for key in paths)
  if instance_iou is not None:
    fields['instance_mIoU'] = round(instance_iou.result()['mean_iou'], 4)
  return fields


def refined_by(stage, image, out, prob):
  """The result `out` of a label-inference function with the denseCRF stage behind it: `prob(out)`, the class
  probabilities `[ncls, h, w]` the reference hands to its CRF, through `stage` on the image's guide; the refined labels
  take the place of `semantic_prediction` and the function's own become `semantic_prediction_before_crf`.  Without a
  stage `out` as it is."""
  if stage is None:
    return out
  refined = stage(image.guide, prob(out))
  return dict(out, semantic_prediction=refined['semantic_prediction'], semantic_prediction_before_crf=out['semantic_prediction'])


def run_prototypes(description, scales, argv=None, single_view=False):
  """`prototype.py` and `prototype_msc.py` (`prototype_msc.py:34-207` of twke18/SPML): every image through
  `spml_amd.inference.multiscale_prototypes`; the programs differ in the scales of the image pyramid (`[1]` against
  `[0.5, 1, 1.5]`, no flip in either) and in `single_view`: `prototype.py` resizes image and label to `test.image_size`
  first (prototype.py:96-105).  The bank of every image is written to `<save_dir>/semantic_prototype/<name>.npy` in the
  reference's on-disk format, where `inference.py` / `inference_msc.py --semantic_memory_dir` read it.  A data list
  needs its label columns."""
  from spml_amd import inference
  config, args, device = parse(description, argv, 'multiscale_prototypes', 'memory-bank generation', file_lists='labels')
  prototype_dir = output_dir(args, 'semantic_prototype')                                          # :43-44
  source = ImageSource.for_program(config, args, device, scales, False, 'multiscale_prototypes', single_view=single_view,
                                   with_labels=True)                                              # :92-95
  embedding_model, _, path = load_models(config, args, device, None)                              # :69-79
  _, crop_size, stride, _ = geometry(config)
  ignore_index = config.dataset.semantic_ignore_index
  per_image = []

  def one(image):
    out = inference.multiscale_prototypes(embedding_model, image.views, image.label_views, crop_size, stride, ignore_index,
                                          NUM_LABEL_VALUES)
    inference.save_image_memory(os.path.join(prototype_dir, source.bank_name(image)), out['prototype'],
                                out['prototype_label'])                                           # :200-207
    per_image.append(int(out['prototype'].shape[0]))
    return out

  done, seconds, out, views = run_loop(source, one)
  report(done, seconds, prototypes_per_image=per_image, views=len(views), scales=list(scales),
         majority_path=out['majority_path'], snapshot=path, save_dir=prototype_dir, **source.fields())


def crf_stage(config, args, crf):
  """The `CrfStage` of a run, or None.  `crf`: True in a `*_crf*.py` program, None in its list-reading sibling, where
  `--crf` decides, False in a program without the option."""
  return CrfStage(config, args) if crf or (crf is None and args.crf) else None


def run_pseudo_softmax(description, scales, combine, walk_steps, argv=None, file_lists='labels', crf=False, cam_alpha=None):
  """`pseudo_softmax.py`, `pseudo_softmaxrw.py` and `pseudo_softmaxrw_crf.py` (`pseudo_softmaxrw_crf.py:33-204` of
  twke18/SPML): every image through `spml_amd.inference.pseudo_labels_softmax`; the programs differ in three constants
  (scales of the image pyramid, how the views' class scores are combined, squarings of the transition matrix) and in
  `crf` (see `crf_stage`).  The label map of an image (synthetic, or the file's own: a data list needs its label columns)
  gives the image tags (:102-106) and the mIoU of the JSON line.  Without the CRF the labels written are those of :176;
  with it every image goes through `pseudo_labels_softmax_crf` on the source's guide image (:172-187) and the
  refined labels of :187 are written, the labels of :176 scored next to them.

  `cam_alpha` (the program's ALPHA; `pseudo_softmaxrw.py` alone passes one): with `--cam_dir` the program is the CAM walk
  of `pseudo_camrw_crf.py:37-198` on either kind of `--data_list` -- the two share the flip pair at scale 1,
  the affinity, the squarings and the tail, and differ in where the class maps come from.  The embedding network alone is
  loaded (:76-91), every image comes with the planes of its CAM file (`ImageSource(with_cams=...)`) and goes through
  `pseudo_labels_cam` / `pseudo_labels_cam_crf`; the reference never uses the label map there (`sem_labs`, :104), so a
  list needs no label columns and is scored only when it has them; the report carries `cam_dir`, `alpha` and `cam_path`
  in place of `combine` and `head_path`.  Without `--cam_dir` nothing of this is reached."""
  from spml_amd import inference
  api = 'pseudo_labels_softmax_crf' if crf else 'pseudo_labels_softmax'
  if cam_alpha is not None:
    listed = file_lists
    file_lists = lambda args: 'images' if args.cam_dir else listed
  config, args, device = parse(description, argv, api, file_lists=file_lists, crf_option=crf is None)
  cam_dir = args.cam_dir if cam_alpha is not None else None
  semantic_dir = output_dir(args, 'semantic_gray')
  stage = crf_stage(config, args, crf)                                                            # :66-73
  source = ImageSource.for_program(config, args, device, scales, True, api, with_guide=stage is not None,
                                   with_cams=cam_dir)                                             # :109-125
  embedding_model, prediction_model, path = load_models(config, args, device, None if cam_dir else 'softmax_classifier')
  num_classes = geometry(config)[0]

  def softmax_walk(image):                                                                        # :126-176
    return inference.pseudo_labels_softmax(embedding_model, prediction_model, image.views, image.image_hw,
                                           source.tags(image), combine=combine, walk_steps=walk_steps)

  def softmax_walk_crf(image):                                                                    # :126-187
    return inference.pseudo_labels_softmax_crf(embedding_model, prediction_model, image.views, image.image_hw,
                                               source.tags(image), image.guide, stage, combine=combine,
                                               walk_steps=walk_steps)

  def cam_walk(image):
    return inference.pseudo_labels_cam(embedding_model, image.views, image.image_hw, image.cam_planes, image.cam_classes,
                                       num_classes, alpha=cam_alpha, walk_steps=walk_steps)

  def cam_walk_crf(image):
    return inference.pseudo_labels_cam_crf(embedding_model, image.views, image.image_hw, image.cam_planes,
                                           image.cam_classes, num_classes, image.guide, stage, alpha=cam_alpha,
                                           walk_steps=walk_steps)

  if cam_dir:
    labels = cam_walk if stage is None else cam_walk_crf
    route = dict(constants=(('cam_dir', cam_dir), ('alpha', cam_alpha), ('walk_steps', walk_steps)), paths=('cam_path',))
  else:
    labels = softmax_walk if stage is None else softmax_walk_crf
    route = dict(constants=(('combine', combine), ('walk_steps', walk_steps)), paths=('head_path',))

  def one(image):
    out = labels(image)
    source.write(image, out, semantic_dir)
    return out

  done, seconds, out, _ = run_loop(source, one)
  report(done, seconds, **source.scores(), **crf_report(stage, source, seconds), scales=list(scales), is_flip=True,
         **route_fields(out, **route), snapshot=path, save_dir=semantic_dir, **source.fields())


def crf_report(stage, source, seconds):
  """The fields a run with the denseCRF adds to its report: `mIoU_before_crf`, `changed_by_crf` (the share of output
  pixels whose label the CRF changed), `crf_path` and `crf_share`; none without the stage."""
  return {} if stage is None else dict(source.crf_fields(), **stage.fields(seconds))


def run_softmax(description, scales, is_flip, argv=None, single_view=False, file_lists='images', crf=None):
  """The four softmax label-inference programs: `inference_softmax.py` / `inference_softmax_crf.py` (`single_view`: one
  view at `test.image_size` through `predict_softmax_full_resolution`, inference_softmax_crf.py:27-176) and
  `inference_softmax_msc.py` / `inference_softmax_crf_msc.py` (the flip pairs of `scales` through
  `predict_softmax_multiscale`, inference_softmax_crf_msc.py:30-177).  `crf`: see `crf_stage`.  With the CRF the class
  probabilities -- the soft-max of the summed logits cropped to the view (:153-154), or the mean over the views
  (:156) -- go with the source's guide image through `dense_crf_refine` (:158-168) and the arg-max of the
  refined marginals is written; the labels before the CRF are the plain program's."""
  from spml_amd import inference
  api = 'dense_crf_refine' if crf else ('predict_softmax_full_resolution' if single_view else 'predict_softmax_multiscale')
  config, args, device = parse(description, argv, api, file_lists=file_lists, crf_option=crf is None)
  semantic_dir = output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = load_models(config, args, device, 'softmax_classifier')
  _, crop_size, stride, _ = geometry(config)
  stage = crf_stage(config, args, crf)
  source = ImageSource.for_program(config, args, device, scales, is_flip, api, single_view=single_view,
                                   with_guide=stage is not None)

  def one_view(image):
    padded, (h, w), _ = image.views[0]
    out = inference.predict_softmax_full_resolution(embedding_model, prediction_model, padded, (h, w), crop_size, stride)
    return refined_by(stage, image, out, lambda out: torch.softmax(out['semantic_logit'], dim=1)[0, :, :h, :w].contiguous())

  def all_views(image):
    out = inference.predict_softmax_multiscale(embedding_model, prediction_model, image.views, image.image_hw, crop_size,
                                               stride)
    return refined_by(stage, image, out,
                      lambda out: out['semantic_prob'] / torch.full((), float(len(image.views)), device=device))

  predict, paths = (one_view, ('head_path',)) if single_view else (all_views, ('combine_path', 'head_path'))

  def one(image):
    out = predict(image)
    source.write(image, out, semantic_dir)
    return out

  done, seconds, out, views = run_loop(source, one)
  report(done, seconds, **source.scores(), **route_fields(out, None if single_view else views, paths=paths),
         **crf_report(stage, source, seconds), snapshot=path, save_dir=semantic_dir, **source.fields())


def run_knn(description, scales, is_flip, argv=None, single_view=False, file_lists='images', crf=None, pseudo_tags=None):
  """The four kNN label-inference programs: `inference.py` / `inference_crf.py` (`single_view`: one view at
  `test.image_size`, inference_crf.py:35-280) and `inference_msc.py` / `inference_crf_msc.py` (the flip pairs of `scales`
  through `predict_knn_multiscale`, inference_crf_msc.py:35-283), against the memory bank of `--semantic_memory_dir`
  (`memory_bank_dir`).  `crf`: see `crf_stage`.  With the CRF a single view goes through the fused
  `predict_knn_full_resolution_crf` (votes gathered inside the CRF's first kernel), the view mean of the
  votes of a multi-view program through `dense_crf_refine` (:251-260), on the source's guide image.

  `pseudo_tags`: `(scales, floor)` in the program that takes `--pseudo_tags` (`inference_msc.py` alone).  With the option
  the run is the tag recipe's kNN pseudo-label step (`pseudo_inference_crf_msc.py:143-275`) on either kind of
  `--data_list`: those scales, the tags of the image's label map (a list needs its label columns) and
  `pseudo_labels_knn_multiscale`; with `--crf` the tag-normalised map is what the CRF stage refines (:265-273).  The
  report gains `normalize_path` and, on synthetic images, `instance_mIoU` as `pseudo_inference_msc.py` reports it; the
  instance-weighted IoU of a list is `benchmark_by_instance.py`'s on the written directory."""
  from spml_amd import inference
  api = 'predict_full_resolution' if single_view else 'predict_knn_multiscale'
  if crf and single_view:
    api = 'predict_knn_full_resolution_crf'
  if pseudo_tags is not None:
    listed = file_lists
    file_lists = lambda args: 'labels' if args.pseudo_tags else listed
  config, args, device = parse(description, argv, api, file_lists=file_lists, crf_option=crf is None,
                               pseudo_tags_option=pseudo_tags is not None)
  tagged = pseudo_tags is not None and args.pseudo_tags
  floor = None
  if tagged:
    scales, floor = pseudo_tags
  semantic_dir = output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = load_models(config, args, device, 'segsort')
  num_classes, crop_size, stride, _ = geometry(config)
  stage = crf_stage(config, args, crf)
  source = ImageSource.for_program(config, args, device, scales, is_flip, api, single_view=single_view,
                                   with_guide=stage is not None)
  memory_dir = memory_bank_dir(embedding_model, config, args, device)
  prototypes, prototype_labels = load_bank(memory_dir, config, device)
  ignore_index = config.dataset.semantic_ignore_index
  by_instance = None
  if tagged and not reads_file_list(args):
    from spml_amd.utils.general import metrics
    by_instance = metrics.InstanceIoU(num_classes)
  models, windows, bank = (embedding_model, prediction_model), (crop_size, stride), (prototypes, prototype_labels)

  def one_view(image):
    padded, valid_hw, _ = image.views[0]
    return inference.predict_full_resolution(*models, padded, valid_hw, *windows, *bank, ignore_index)

  def one_view_crf(image):
    padded, valid_hw, _ = image.views[0]
    return inference.predict_knn_full_resolution_crf(*models, padded, valid_hw, *windows, *bank, num_classes, image.guide,
                                                     stage, ignore_index)

  def view_votes(image):
    return inference.predict_knn_multiscale(*models, image.views, image.image_hw, *windows, *bank, num_classes)

  def tagged_view_votes(image):
    return inference.pseudo_labels_knn_multiscale(*models, image.views, image.image_hw, *windows, *bank, num_classes,
                                                  source.tags(image), floor=floor, return_prob=stage is not None)

  votes = tagged_view_votes if tagged else view_votes

  def all_views(image):
    return refined_by(stage, image, votes(image), lambda out: out['semantic_prob'])

  if not single_view:
    predict, paths = all_views, ('combine_path', 'normalize_path') if tagged else ('combine_path',)
  elif stage is None:
    predict, paths = one_view, ()
  else:
    predict, paths = one_view_crf, ('votes_path',)

  def one(image):
    out = predict(image)
    source.write(image, out, semantic_dir)
    if by_instance is not None:
      by_instance.update(out['semantic_prediction'], image.label, image.instance.clamp(0, 255))
    return out

  done, seconds, out, views = run_loop(source, one)
  report(done, seconds, **source.scores(),
         **route_fields(out, None if single_view else views, paths=paths, instance_iou=by_instance),
         **crf_report(stage, source, seconds), memory_prototypes=int(prototypes.shape[0]), snapshot=path,
         semantic_memory_dir=memory_dir, save_dir=semantic_dir, **source.fields())


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
    out = self._timed(inference.dense_crf_refine, image_u8, prob, self.crf)
    self.path = out['crf_path']
    return out

  def refine_upsampled(self, image_u8, lowres):
    """The fused call of the random-walk programs (`DenseCRF.refine_upsampled`: the low-resolution walked maps are
    up-sampled inside the CRF's first kernel) between the same device events.  With this method and `path_name` the stage
    stands in for its `DenseCRF` as the `crf` of `inference.random_walk_crf_refine` and `pseudo_labels_softmax_crf`, so
    the events enclose the CRF alone and not the network and the walk in front of it."""
    return self._timed(self.crf.refine_upsampled, image_u8, lowres)

  def _timed(self, call, *args):
    """`call(*args)` between two device events of the stage: the one place they are recorded."""
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
