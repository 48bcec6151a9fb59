#!/usr/bin/env python3
"""Stage 2: training the softmax classifier on a frozen embedding network, with the reference's command
line and config surface (`pyscripts/train/train_classifier.py:33-185` of twke18/SPML):

  python3 pyscripts/train/train_classifier.py --data_dir D --data_list L --snapshot_dir S --cfg_path config_classifier.yaml
  torchrun --nproc-per-node 8 pyscripts/train/train_classifier.py ...      (one process per GPU, RCCL)

`config.network.pretrained` must name stage 1's snapshot (`model-{iter}.pth`; its `embedding_model` entry
is loaded, :97-104 -- "Pre-trained model is required."); `prediction_types` must be `softmax_classifier`
(:84-87), `backbone_types` `panoptic_deeplab_101` / `panoptic_pspnet_101` (:78-82).  The step itself is
`spml_amd.train.ClassifierTrainer.step`; snapshots are the reference's two files (:172-180).  As in the
stage-1 entry point `--data_dir` / `--data_list` name a file list, read here as the reference's
ListTagClassifierDataset reads it (random grayscale and blur on, :54-65; spml_amd/data); `--data_list synthetic` (or no
list anywhere) feeds seeded synthetic batches of the same shape."""
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None, dataset='list_tag', description='Training for softmax classifier only.'):
  """`dataset`: 'list_tag' as pyscripts/train/train_classifier.py:21-24 (ListTagClassifierDataset, DeepLab / PSPNet
  embedding), 'densepose' as pyscripts/train/train_densepose_classifier.py:21-23 (DenseposeClassifierDataset, the
  DensePose PSPNet embedding)."""
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args(description, argv)
  if not torch.cuda.is_available():
    raise SystemExit('training needs an MI355X (the HIP path has no CPU fallback)')
  from spml_amd.data.batcher import resolve_data_list, training_batcher
  source = resolve_data_list(args, config)  # (a list that does not exist ends the program here, by name)
  world = int(os.environ.get('WORLD_SIZE', '1'))
  rank = int(os.environ.get('RANK', '0'))
  local = int(os.environ.get('LOCAL_RANK', '0'))
  torch.cuda.set_device(local)
  device = torch.device('cuda', local)
  if world > 1:
    dist.init_process_group('nccl', device_id=device)
  from spml_amd import synth
  from spml_amd.train import ClassifierTrainer
  os.makedirs(args.snapshot_dir, exist_ok=True)
  model_path = os.path.join(args.snapshot_dir, 'model-{:d}.pth')
  state_path = os.path.join(args.snapshot_dir, 'model-{:d}.state.pth')
  torch.manual_seed(235)                    # train_classifier.py:26-27
  if dataset == 'densepose':
    from spml_amd.data.datasets.densepose_dataset import DenseposeClassifierDataset as dataset_class
    trainer = ClassifierTrainer(config, device, channels_last=True, models=densepose_models(config))
  else:
    from spml_amd.data.datasets.list_tag_dataset import ListTagClassifierDataset as dataset_class
    trainer = ClassifierTrainer(config, device, channels_last=True)
  if not config.network.pretrained:
    raise ValueError('Pre-trained model is required.')
  print('Loading pre-trained model: {:s}'.format(config.network.pretrained))
  trainer.load_pretrained(config.network.pretrained)
  batches = training_batcher(dataset_class, source, config, device, rank, world, first_iteration=trainer.curr_iter,
                             random_grayscale=True, random_blur=True)
  t0 = time.time()
  for curr_iter in range(trainer.curr_iter, config.train.max_iteration):
    if batches is None:
      datas, targets = synth.make_batch(config.train.batch_size, config.train.crop_size[0],
                                        num_classes=config.dataset.num_classes, seed=235 + 1009 * rank + curr_iter,
                                        device=device, supervision=args.supervision, palette=(1, 3))
    else:
      datas, targets = next(batches)
    datas['image'] = datas['image'].contiguous(memory_format=torch.channels_last)
    out = trainer.step(datas, targets)
    if rank == 0 and (curr_iter % 10 == 0 or curr_iter == config.train.max_iteration - 1):
      print('iter {:d}: loss = {:.3f}, acc = {:.3f}, lr = {:.6f}  ({:.2f} s)'.format(
          curr_iter, float(out['loss']), float(out['accuracy']), out['lr'], time.time() - t0), flush=True)
    if rank == 0 and config.train.snapshot_step and (
        (curr_iter + 1) % config.train.snapshot_step == 0 or curr_iter == config.train.max_iteration - 1):
      state = trainer.state_dict()
      torch.save({'embedding_model': state['embedding_model'],
                  'prediction_model': state['prediction_model']}, model_path.format(curr_iter))
      torch.save(state['optimizer'], state_path.format(curr_iter))
  if batches is not None:
    batches.close()
  if world > 1:
    dist.destroy_process_group()


def densepose_models(config):
  """The modules pyscripts/train/train_densepose_classifier.py:22-23 binds, with its refusals (:75-83)."""
  import spml_amd.models.embeddings.resnet_pspnet_densepose as dp_emb
  from spml_amd.models.predictions.softmax_classifier import softmax_classifier
  if config.network.backbone_types != 'panoptic_pspnet_101':
    raise ValueError('Not support ' + str(config.network.backbone_types))
  if config.network.prediction_types != 'softmax_classifier':
    raise ValueError('Not support ' + str(config.network.prediction_types))
  return dp_emb.resnet_101_pspnet(config), softmax_classifier(config)


if __name__ == '__main__':
  main()
