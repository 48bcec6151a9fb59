"""Body of the two pseudo-label programs (`pyscripts/inference/pseudo_softmax.py`, `pseudo_softmaxrw.py`): the
reference's command line and config surface (`pseudo_softmaxrw_crf.py:33-204` of twke18/SPML), snapshot loading as
in `pyscripts/inference/inference_softmax.py`, every image through `spml_amd.inference.pseudo_labels_softmax`.  The
programs differ in three constants only (scales of the image pyramid, how the views' class scores are combined,
squarings of the transition matrix).  The file-list loader and denseCRF are outside this repository:
`--data_list synthetic` feeds seeded synthetic images of `test.image_size`, whose label maps give the image tags
(:102-106) and the mIoU of the JSON line; the labels written are those of :176, before the CRF refinement."""
import json
import os
import time

import numpy as np
import torch

NUM_SYNTHETIC_IMAGES = 4


def run(description, scales, combine, walk_steps, argv=None):
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args(description, argv)
  if not torch.cuda.is_available():
    raise SystemExit('inference needs an MI355X (the HIP path has no CPU fallback)')
  if not args.save_dir:
    raise SystemExit('--save_dir is required')
  if args.data_list not in (None, 'synthetic'):
    raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                     'use --data_list synthetic or call spml_amd.inference.pseudo_labels_softmax '
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
    raise ValueError('Not support ' + str(config.network.backbone_types))                    # :76
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
  crop_size = tuple(config.test.crop_size)
  size = config.test.image_size if config.test.image_size > 0 else crop_size[0]
  counts, head_path, done = None, None, 0
  torch.cuda.synchronize()
  t0 = time.time()
  for index in range(NUM_SYNTHETIC_IMAGES):
    datas, targets = synth.make_batch(1, size, num_classes=num_classes, seed=4099 + index, device=device,
                                      palette=(1, 3))
    label = targets['semantic_label'][0]
    views = inference.flip_scale_views(datas['image'], scales, True, crop_size)              # :109-125
    out = inference.pseudo_labels_softmax(embedding_model, prediction_model, views, (size, size),
                                          inference.label_tags_from_map(label, num_classes), combine=combine,
                                          walk_steps=walk_steps)
    head_path = out['head_path']
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    np.save(os.path.join(semantic_dir, 'synthetic_{:04d}.npy'.format(index)),
            out['semantic_prediction'].to(torch.uint8).cpu().numpy())
    done += 1
  torch.cuda.synchronize()
  seconds = time.time() - t0
  scores = metrics.mean_iou(counts)
  print(json.dumps({'images': done, 'images_per_s': round(done / seconds, 3), 'mIoU': round(scores['mean_iou'], 4),
                    'pixel_acc': round(scores['pixel_acc'], 4), 'scales': list(scales), 'is_flip': True,
                    'combine': combine, 'walk_steps': walk_steps, 'head_path': head_path, 'snapshot': path,
                    'save_dir': semantic_dir}))
