"""Body of the two memory-bank programs (`pyscripts/inference/prototype.py`, `prototype_msc.py`): the reference's
command line and config surface (`prototype_msc.py:34-207` of twke18/SPML), snapshot loading as in
`pyscripts/inference/inference_msc.py`, every image through `spml_amd.inference.multiscale_prototypes`.  The programs
differ in the scales of the image pyramid only (`[1]` against `[0.5, 1, 1.5]`, no flip in either).  The file-list loader
is outside this repository: `--data_list synthetic` feeds seeded synthetic images of `test.image_size`.  The
bank of every image is written to `<save_dir>/semantic_prototype/<name>.npy` in the reference's on-disk format
(`save_image_memory`), where `inference.py` / `inference_msc.py --semantic_memory_dir` read it."""
import json
import os
import time

import torch

NUM_SYNTHETIC_IMAGES = 4
NUM_LABEL_VALUES = 256            # label maps hold classes and the ignore value 255 (prototype_msc.py:189-192)


def synthetic_image(index, size, num_classes, device, ignore_index=255):
  """Image `[1,3,size,size]` and dense label `[size,size]` of synthetic image `index` (the images of inference_msc.py).
  The generator keeps ~10 % of the labels (scribbles) and the bank pass needs dense ones: every other pixel (the
  unlabelled value 254 and the ignore strip) takes the image's most frequent labelled class, as inference_msc.py does
  for its own bank.  A small image may keep no labelled pixel at all: it is then ignored as a whole (`ignore_index`
  everywhere), so that no prototype enters the bank under the unlabelled value -- the retrieval side drops the ignore
  label and nothing else."""
  from spml_amd import synth
  datas, targets = synth.make_batch(1, size, num_classes=num_classes, seed=4099 + index, device=device,
                                    palette=(1, max(1, min(3, num_classes - 1))))
  label = targets['semantic_label'][0]
  labelled = label[label < num_classes]
  fill = torch.mode(labelled).values if labelled.numel() else torch.full_like(label, ignore_index)
  label = torch.where(label < num_classes, label, fill)
  return datas['image'].float(), label


def run(description, scales, argv=None):
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args(description, argv)
  if args.kmeans_num_clusters:
    config.network.kmeans_num_clusters = [int(i) for i in args.kmeans_num_clusters.split(',')]     # :39
  if args.label_divisor:
    config.network.label_divisor = args.label_divisor                                             # :40
  if args.data_list not in (None, 'synthetic'):
    raise SystemExit('file-list data loading (ListDataset) is outside the scope of this repository; '
                     'use --data_list synthetic or call spml_amd.inference.multiscale_prototypes '
                     'on your own images')
  if not torch.cuda.is_available():
    raise SystemExit('memory-bank generation needs an MI355X (the HIP path has no CPU fallback)')
  if not args.save_dir:
    raise SystemExit('--save_dir is required')
  from spml_amd import inference
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  from spml_amd.models.embeddings.resnet_pspnet import resnet_101_pspnet
  device = torch.device('cuda', 0)
  torch.cuda.set_device(device)
  prototype_dir = os.path.join(args.save_dir, 'semantic_prototype')                               # :43-44
  os.makedirs(prototype_dir, exist_ok=True)

  makers = {'panoptic_pspnet_101': resnet_101_pspnet, 'panoptic_deeplab_101': resnet_101_deeplab}
  if config.network.backbone_types not in makers:
    raise ValueError('Not support ' + str(config.network.backbone_types))                        # :69
  embedding_model = makers[config.network.backbone_types](config).to(device).to(memory_format=torch.channels_last)
  embedding_model.eval()
  path = os.path.join(args.snapshot_dir, 'model-{:d}.pth'.format(config.train.max_iteration - 1))
  state = torch.load(path, map_location=device, weights_only=True)
  embedding_model.load_state_dict(state['embedding_model'], resume=True)                          # :75-79

  num_classes = config.dataset.num_classes
  crop_size, stride = tuple(config.test.crop_size), tuple(config.test.stride)
  size = config.test.image_size if config.test.image_size > 0 else crop_size[0]
  per_image, out, views, done = [], None, [], 0
  torch.cuda.synchronize()
  t0 = time.time()
  for index in range(NUM_SYNTHETIC_IMAGES):
    image, label = synthetic_image(index, size, num_classes, device, config.dataset.semantic_ignore_index)
    views = inference.flip_scale_views(image, scales, False, crop_size)                           # :92-95
    labels = inference.label_views(label, [hw for _, hw, _ in views])
    out = inference.multiscale_prototypes(embedding_model, views, labels, crop_size, stride,
                                          config.dataset.semantic_ignore_index, NUM_LABEL_VALUES)
    inference.save_image_memory(os.path.join(prototype_dir, 'synthetic_{:04d}.npy'.format(index)), out['prototype'],
                                out['prototype_label'])                                           # :200-207
    per_image.append(int(out['prototype'].shape[0]))
    done += 1
  torch.cuda.synchronize()
  seconds = time.time() - t0
  print(json.dumps({'images': done, 'images_per_s': round(done / seconds, 3), 'prototypes_per_image': per_image,
                    'views': len(views), 'scales': list(scales), 'majority_path': out['majority_path'],
                    'snapshot': path, 'save_dir': prototype_dir}))
