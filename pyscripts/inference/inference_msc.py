#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by nearest-neighbour retrieval, with the reference's command
line and config surface (`pyscripts/inference/inference_msc.py:35-255` of twke18/SPML), the form the recipes report
their kNN numbers through:

  python3 pyscripts/inference/inference_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:83-89) and the prototype memory bank from
`--semantic_memory_dir` (`segsort_others.load_memory_banks`, the ignore class dropped: :92-111).  Every image becomes
the ten views of `spml_amd.inference.flip_scale_views` (scales 0.5, 0.75, 1, 1.25, 1.5, each flipped and plain,
zero-padded to the crop size: :123-137) and goes through `spml_amd.inference.predict_knn_multiscale` (per view the
sliding-window embedding, k-means over the un-padded view, top-20 retrieval per segment and one HIP launch pair for
votes, resize, un-flip and sum; then the mean over the views and one arg-max).  As in the training entry points the
file-list loader is outside this repository: `--data_list synthetic` feeds seeded synthetic images of
`test.image_size`.  Without `--semantic_memory_dir` the synthetic mode builds the bank itself: the prototypes of the
synthetic images (`full_resolution_prototypes`, what `prototype.py` does) are written with `save_image_memory` to
`<save_dir>/semantic_prototype` and read back from those files.  Label maps are written as `semantic_gray/<name>.npy`
(uint8; no image library is needed); one JSON line reports images/s, mIoU and pixel accuracy
(`pyscripts/benchmark/benchmark_by_mIoU.py`), the number of views and the path taken by the per-view tail."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NUM_SYNTHETIC_IMAGES = 4
SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :125


def separate_comma(str_comma):
  return [int(i) for i in str_comma.split(',')]


def synthetic_image(index, size, num_classes, device):
  from spml_amd import synth
  datas, targets = synth.make_batch(1, size, num_classes=num_classes, seed=4099 + index, device=device,
                                    palette=(1, max(1, min(3, num_classes - 1))))
  return datas['image'].float(), targets['semantic_label'][0]


def main(argv=None):
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args('Inference for semantic segmentation.', argv)
  if args.kmeans_num_clusters:
    config.network.kmeans_num_clusters = separate_comma(args.kmeans_num_clusters)             # :40
  if args.label_divisor:
    config.network.label_divisor = args.label_divisor                                         # :41
  if args.data_list not in (None, 'synthetic'):
    raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                     'use --data_list synthetic or call spml_amd.inference.predict_knn_multiscale '
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
    raise ValueError('Not support ' + str(config.network.backbone_types))                    # :70
  if config.network.prediction_types != 'segsort':
    raise ValueError('Not support ' + str(config.network.prediction_types))                  # :75
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
    # synthetic mode on its own: the memory-bank pass over the synthetic images (prototype.py:107-211)
    memory_dir = os.path.join(args.save_dir, 'semantic_prototype')
    os.makedirs(memory_dir, exist_ok=True)
    for index in range(NUM_SYNTHETIC_IMAGES):
      image, label = synthetic_image(index, size, num_classes, device)
      padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]
      # the synthetic generator keeps ~10 % of the labels (scribbles) and the pass needs dense ones: the other pixels
      # take the image's most frequent labelled class (its ground truth up to 171 pixels: one class per 171-pixel cell)
      labelled = label[label < num_classes]
      if labelled.numel():
        label = torch.where(label < num_classes, label, torch.mode(labelled).values)
      prototypes, prototype_labels, _ = inference.full_resolution_prototypes(
          embedding_model, padded, label, crop_size, stride, config.dataset.semantic_ignore_index)
      inference.save_image_memory(os.path.join(memory_dir, 'synthetic_{:04d}.npy'.format(index)), prototypes,
                                  prototype_labels)
  prototypes, prototype_labels = segsort_others.load_memory_banks(memory_dir)                 # :94-95
  prototypes, prototype_labels = inference.drop_ignored_memory(
      prototypes.to(device), prototype_labels.to(device), config.dataset.semantic_ignore_index)   # :99-111

  counts, out, views, done = None, None, [], 0
  torch.cuda.synchronize()
  t0 = time.time()
  for index in range(NUM_SYNTHETIC_IMAGES):
    image, label = synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, SCALES, True, crop_size)                        # :123-137
    out = inference.predict_knn_multiscale(embedding_model, prediction_model, views, (size, size), crop_size, stride,
                                           prototypes, prototype_labels, num_classes)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    np.save(os.path.join(semantic_dir, 'synthetic_{:04d}.npy'.format(index)),
            out['semantic_prediction'].to(torch.uint8).cpu().numpy())
    done += 1
  torch.cuda.synchronize()
  seconds = time.time() - t0
  scores = metrics.mean_iou(counts)
  print(json.dumps({'images': done, 'images_per_s': round(done / seconds, 3), 'mIoU': round(scores['mean_iou'], 4),
                    'pixel_acc': round(scores['pixel_acc'], 4), 'views': len(views),
                    'combine_path': out['combine_path'], 'memory_prototypes': int(prototypes.shape[0]),
                    'snapshot': path, 'semantic_memory_dir': memory_dir, 'save_dir': semantic_dir}))


if __name__ == '__main__':
  main()
