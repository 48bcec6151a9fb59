#!/usr/bin/env python3
"""Pseudo-label generation by nearest-neighbour retrieval for the image-tag recipe, with the reference's command line and
config surface (`pyscripts/inference/pseudo_inference_crf_msc.py:38-289` of twke18/SPML) without its `--crf_*` options:
the denseCRF (:265-273) is outside this repository, the stage ends at the arg-max of what the CRF would have been fed.

  python3 pyscripts/inference/pseudo_inference_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory and the prototype memory bank from
`--semantic_memory_dir` (what `prototype_msc.py` writes; the ignore class dropped: :101-121).  Every image becomes the
eight views of `spml_amd.inference.flip_scale_views` (scales 0.5, 1, 1.5, 2, each flipped and plain, zero-padded to the
crop size: :133-153) and goes through `spml_amd.inference.pseudo_labels_knn_multiscale`: per view the work of
`inference_msc.py`, then one HIP launch pair that takes the mean over the views, normalises every class the image
carries by its maximum over the image (floored at 0.15) and takes the arg-max (:252-263, :275).  The image's tags are
the classes of its label map (:138-141).  As in the other entry points the file-list loader is outside this repository:
`--data_list synthetic` feeds seeded synthetic images of `test.image_size`, and without `--semantic_memory_dir` the bank
is built from those images first, written with `save_image_memory` to `<save_dir>/semantic_prototype` and read back.
Label maps are written as `semantic_gray/<name>.npy` (uint8); one JSON line reports images/s, mIoU and pixel accuracy
(`pyscripts/benchmark/benchmark_by_mIoU.py`), the instance-weighted mIoU (`benchmark_by_instance.py`, from the synthetic
instance map), the number of views and the paths taken by the per-view tail and by the normalisation."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NUM_SYNTHETIC_IMAGES = 4
SCALES = [0.5, 1, 1.5, 2]                                                                    # :135
FLOOR = 0.15                                                                                 # :260


def separate_comma(str_comma):
  return [int(i) for i in str_comma.split(',')]


def synthetic_image(index, size, num_classes, device):
  """-> (image [1,3,S,S], semantic label [S,S], instance label [S,S]) of one seeded synthetic image."""
  from spml_amd import synth
  datas, targets = synth.make_batch(1, size, num_classes=num_classes, seed=4099 + index, device=device,
                                    palette=(1, max(1, min(3, num_classes - 1))))
  return datas['image'].float(), targets['semantic_label'][0], targets['instance_label'][0]


def main(argv=None):
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args('Inference for semantic segmentation.', argv)
  if args.kmeans_num_clusters:
    config.network.kmeans_num_clusters = separate_comma(args.kmeans_num_clusters)             # :43
  if args.label_divisor:
    config.network.label_divisor = args.label_divisor                                         # :44
  if args.data_list not in (None, 'synthetic'):
    raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                     'use --data_list synthetic or call spml_amd.inference.pseudo_labels_knn_multiscale '
                     'on your own images')
  if not torch.cuda.is_available():
    raise SystemExit('inference needs an MI355X (the HIP path has no CPU fallback)')
  if not args.save_dir:
    raise SystemExit('--save_dir is required')
  from spml_amd import inference
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  from spml_amd.models.embeddings.resnet_pspnet import resnet_101_pspnet
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.utils.general import metrics
  import spml_amd.utils.segsort.others as segsort_others
  device = torch.device('cuda', 0)
  torch.cuda.set_device(device)
  semantic_dir = os.path.join(args.save_dir, 'semantic_gray')
  os.makedirs(semantic_dir, exist_ok=True)

  makers = {'panoptic_pspnet_101': resnet_101_pspnet, 'panoptic_deeplab_101': resnet_101_deeplab}
  if config.network.backbone_types not in makers:
    raise ValueError('Not support ' + str(config.network.backbone_types))                    # :73
  if config.network.prediction_types != 'segsort':
    raise ValueError('Not support ' + str(config.network.prediction_types))                  # :78
  embedding_model = makers[config.network.backbone_types](config).to(device).to(memory_format=torch.channels_last)
  prediction_model = segsort(config).to(device)
  embedding_model.eval()
  prediction_model.eval()
  path = os.path.join(args.snapshot_dir, 'model-{:d}.pth'.format(config.train.max_iteration - 1))
  state = torch.load(path, map_location=device, weights_only=True)
  embedding_model.load_state_dict(state['embedding_model'], resume=True)
  prediction_model.load_state_dict(state['prediction_model'])

  num_classes = config.dataset.num_classes
  crop_size, stride = tuple(config.test.crop_size), tuple(config.test.stride)
  size = config.test.image_size if config.test.image_size > 0 else crop_size[0]
  memory_dir = args.semantic_memory_dir
  if memory_dir is None:
    # synthetic mode on its own: the memory-bank pass over the synthetic images, as inference_msc.py builds it
    memory_dir = os.path.join(args.save_dir, 'semantic_prototype')
    os.makedirs(memory_dir, exist_ok=True)
    for index in range(NUM_SYNTHETIC_IMAGES):
      image, label, _ = synthetic_image(index, size, num_classes, device)
      padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]
      labelled = label[label < num_classes]
      if labelled.numel():                  # dense labels for the pass: the other pixels take the most frequent class
        label = torch.where(label < num_classes, label, torch.mode(labelled).values)
      prototypes, prototype_labels, _ = inference.full_resolution_prototypes(
          embedding_model, padded, label, crop_size, stride, config.dataset.semantic_ignore_index)
      inference.save_image_memory(os.path.join(memory_dir, 'synthetic_{:04d}.npy'.format(index)), prototypes,
                                  prototype_labels)
  prototypes, prototype_labels = segsort_others.load_memory_banks(memory_dir)                 # :104-105
  prototypes, prototype_labels = inference.drop_ignored_memory(
      prototypes.to(device), prototype_labels.to(device), config.dataset.semantic_ignore_index)   # :109-121

  counts, by_instance, out, views, done = None, metrics.InstanceIoU(num_classes), None, [], 0
  torch.cuda.synchronize()
  t0 = time.time()
  for index in range(NUM_SYNTHETIC_IMAGES):
    image, label, instance = synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, SCALES, True, crop_size)                        # :133-153
    tags = inference.label_tags_from_map(label, num_classes)                                  # :138-141
    out = inference.pseudo_labels_knn_multiscale(embedding_model, prediction_model, views, (size, size), crop_size,
                                                 stride, prototypes, prototype_labels, num_classes, tags, floor=FLOOR)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    by_instance.update(out['semantic_prediction'], label, instance.clamp(0, 255))
    np.save(os.path.join(semantic_dir, 'synthetic_{:04d}.npy'.format(index)),
            out['semantic_prediction'].to(torch.uint8).cpu().numpy())
    done += 1
  torch.cuda.synchronize()
  seconds = time.time() - t0
  scores = metrics.mean_iou(counts)
  print(json.dumps({'images': done, 'images_per_s': round(done / seconds, 3), 'mIoU': round(scores['mean_iou'], 4),
                    'pixel_acc': round(scores['pixel_acc'], 4),
                    'instance_mIoU': round(by_instance.result()['mean_iou'], 4), 'views': len(views),
                    'combine_path': out['combine_path'], 'normalize_path': out['normalize_path'],
                    'memory_prototypes': int(prototypes.shape[0]), 'snapshot': path, 'semantic_memory_dir': memory_dir,
                    'save_dir': semantic_dir}))


if __name__ == '__main__':
  main()
