#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by the softmax classifier, with the reference's command line
and config surface (`pyscripts/inference/inference_softmax_msc.py:29-167` of twke18/SPML), the form every stage-2 recipe
reports its number through:

  python3 pyscripts/inference/inference_softmax_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:70-76): `embedding_model` through the reference's
name mapping (`resume=True`), `prediction_model` non-strictly -- a stage-1 `SegsortSoftmax` snapshot carries the same
`semantic_classifier.*` names next to entries this model does not have.  Every image becomes the ten views of
`spml_amd.inference.flip_scale_views` (scales 0.5, 0.75, 1, 1.25, 1.5, each flipped and plain, zero-padded to the crop
size: :90-103) and goes through `spml_amd.inference.predict_softmax_multiscale` (sliding windows and the HIP classifier
head per view, one HIP kernel per view for counts, crop, resize, softmax, un-flip and sum, one arg-max).  As in the
training entry points the file-list loader is outside this repository: `--data_list synthetic` feeds seeded synthetic
images of `test.image_size`.  Label maps are written as `semantic_gray/<name>.npy` (uint8; no image library is needed);
one JSON line reports images/s, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`), the number of
views and the paths taken by the classifier head and by the per-view tail."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NUM_SYNTHETIC_IMAGES = 4
SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :92


def main(argv=None):
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args('Inference for semantic segmentation.', argv)
  if not torch.cuda.is_available():
    raise SystemExit('inference needs an MI355X (the HIP path has no CPU fallback)')
  if not args.save_dir:
    raise SystemExit('--save_dir is required')
  if args.data_list not in (None, 'synthetic'):
    raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                     'use --data_list synthetic or call spml_amd.inference.predict_softmax_multiscale '
                     'on your own images')
  from spml_amd import inference, synth
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  from spml_amd.models.embeddings.resnet_pspnet import resnet_101_pspnet
  from spml_amd.models.predictions.softmax_classifier import softmax_classifier
  from spml_amd.utils.general import metrics
  device = torch.device('cuda', 0)
  torch.cuda.set_device(device)
  semantic_dir = os.path.join(args.save_dir, 'semantic_gray')
  os.makedirs(semantic_dir, exist_ok=True)

  makers = {'panoptic_pspnet_101': resnet_101_pspnet, 'panoptic_deeplab_101': resnet_101_deeplab}
  if config.network.backbone_types not in makers:
    raise ValueError('Not support ' + str(config.network.backbone_types))                    # :63
  embedding_model = makers[config.network.backbone_types](config).to(device).to(memory_format=torch.channels_last)
  prediction_model = softmax_classifier(config).to(device)
  embedding_model.eval()
  prediction_model.eval()
  path = os.path.join(args.snapshot_dir, 'model-{:d}.pth'.format(config.train.max_iteration - 1))
  state = torch.load(path, map_location=device, weights_only=True)
  embedding_model.load_state_dict(state['embedding_model'], resume=True)
  head = {k: v for k, v in state['prediction_model'].items() if k.startswith('semantic_classifier.')}
  missing = torch.nn.Module.load_state_dict(prediction_model, head, strict=False).missing_keys
  if missing:
    raise ValueError('%s has no classifier head (missing %s)' % (path, ', '.join(missing)))

  num_classes = config.dataset.num_classes
  crop_h, crop_w = config.test.crop_size
  size = config.test.image_size if config.test.image_size > 0 else crop_h
  counts, out, views, done = None, None, [], 0
  torch.cuda.synchronize()
  t0 = time.time()
  for index in range(NUM_SYNTHETIC_IMAGES):
    datas, targets = synth.make_batch(1, size, num_classes=num_classes, seed=4099 + index, device=device,
                                      palette=(1, 3))
    views = inference.flip_scale_views(datas['image'].float(), SCALES, True, (crop_h, crop_w))     # :90-103
    out = inference.predict_softmax_multiscale(embedding_model, prediction_model, views, (size, size),
                                               (crop_h, crop_w), tuple(config.test.stride))
    counts = metrics.iou_stats(out['semantic_prediction'], targets['semantic_label'][0], num_classes, counts)
    np.save(os.path.join(semantic_dir, 'synthetic_{:04d}.npy'.format(index)),
            out['semantic_prediction'].to(torch.uint8).cpu().numpy())
    done += 1
  torch.cuda.synchronize()
  seconds = time.time() - t0
  scores = metrics.mean_iou(counts)
  print(json.dumps({'images': done, 'images_per_s': round(done / seconds, 3), 'mIoU': round(scores['mean_iou'], 4),
                    'pixel_acc': round(scores['pixel_acc'], 4), 'views': len(views), 'head_path': out['head_path'],
                    'combine_path': out['combine_path'], 'snapshot': path, 'save_dir': semantic_dir}))


if __name__ == '__main__':
  main()
