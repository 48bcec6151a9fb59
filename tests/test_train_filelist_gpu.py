"""The four training programs from a file list: two iterations each at a crop of 97 from generated PNGs, through
spml_amd.data and csrc/augment.hip; snapshots written, losses finite."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_augment import load_program
from test_train_cli import YAML

pytestmark = pytest.mark.gpu


def write_dataset(root, num_classes, n=6):
  """`n` images of different sizes with blocky labels (16-pixel cells; an ignore strip), and their list."""
  from PIL import Image
  rng = np.random.RandomState(17)
  os.makedirs(os.path.join(root, 'files'), exist_ok=True)
  lines = []
  for k in range(n):
    h, w = 80 + 11 * k, 140 - 9 * k
    cells = lambda hi: rng.randint(0, hi, (h // 16 + 1, w // 16 + 1))[np.arange(h)[:, None] // 16, np.arange(w)[None] // 16]
    rgb = np.clip(cells(200)[..., None] + rng.randint(0, 56, (h, w, 3)), 0, 255).astype(np.uint8)
    sem = cells(num_classes).astype(np.uint8)
    sem[:, :6] = 255
    inst = cells(4).astype(np.uint8)
    for name, a in (('%d.png' % k, rgb), ('%d_sem.png' % k, sem), ('%d_inst.png' % k, inst)):
      Image.fromarray(a).save(os.path.join(root, 'files', name))
    lines.append('files/%d.png files/%d_sem.png files/%d_inst.png' % (k, k, k))
  path = os.path.join(root, 'train.txt')
  with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
  return path


def run_program(name, cfg_text, work, tag, data_dir, data_list, capsys):
  cfg = os.path.join(work, tag + '.yaml')
  with open(cfg, 'w') as f:
    f.write(cfg_text)
  snap = os.path.join(work, tag)
  load_program(name).main(['--snapshot_dir', snap, '--cfg_path', cfg, '--data_dir', data_dir, '--data_list', data_list])
  out = capsys.readouterr().out
  losses = [float(v) for v in re.findall(r'iter \d+: loss = (-?[\d.]+|nan|inf)', out)]
  assert len(losses) == 2 and all(math.isfinite(v) for v in losses), out
  model = torch.load(os.path.join(snap, 'model-1.pth'), map_location='cpu')
  assert sorted(model.keys()) == ['embedding_model', 'prediction_model']
  opt = torch.load(os.path.join(snap, 'model-1.state.pth'), map_location='cpu', weights_only=False)
  assert 'state' in opt and 'param_groups' in opt
  return os.path.join(snap, 'model-1.pth')


VOC = YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101')
DENSEPOSE = (YAML.replace('panoptic_deeplab_50', 'panoptic_pspnet_101').replace('num_classes: 21', 'num_classes: 15')
             .replace('sem_occ_loss_types: segsort', 'sem_occ_loss_types: none')
             .replace('memory_bank_size: 2', 'memory_bank_size: 0'))


def classifier(text, pretrained):
  return (text.replace('prediction_types: segsort', 'prediction_types: softmax_classifier')
          .replace('kmeans_iterations: 3', 'kmeans_iterations: 0').replace('pretrained: ""', 'pretrained: "%s"' % pretrained))


def test_voc_stages_train_from_a_file_list(tmp_path, capsys):
  work = str(tmp_path)
  data_list = write_dataset(work, 21)
  stage1 = run_program('train', VOC, work, 'stage1', work, data_list, capsys)
  run_program('train_classifier', classifier(VOC, stage1), work, 'stage2', work, data_list, capsys)


def test_densepose_stages_train_from_a_file_list(tmp_path, capsys):
  work = str(tmp_path)
  data_list = write_dataset(work, 15)
  stage1 = run_program('train_densepose', DENSEPOSE, work, 'dp1', work, data_list, capsys)
  stage2 = run_program('train_densepose_classifier', classifier(DENSEPOSE, stage1), work, 'dp2', work, data_list, capsys)
  one, two = torch.load(stage1, map_location='cpu'), torch.load(stage2, map_location='cpu')
  assert any(k.startswith('lfn.') for k in two['embedding_model'])               # the DensePose embedding network ...
  for k, v in one['embedding_model'].items():
    assert torch.equal(two['embedding_model'][k], v), k                          # ... frozen
  assert any(k.startswith('semantic_classifier.') for k in two['prediction_model'])


def test_densepose_classifier_keeps_the_refusals(tmp_path):
  mod = load_program('train_densepose_classifier')
  cfg = tmp_path / 'c.yaml'
  base = ['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--data_list', 'synthetic']
  cfg.write_text(classifier(DENSEPOSE, ''))
  with pytest.raises(ValueError, match='Pre-trained model is required'):
    mod.main(base)
  cfg.write_text(classifier(DENSEPOSE, '').replace('panoptic_pspnet_101', 'panoptic_deeplab_101'))
  with pytest.raises(ValueError, match='Not support panoptic_deeplab_101'):
    mod.main(base)
  cfg.write_text(DENSEPOSE)
  with pytest.raises(ValueError, match='Not support segsort'):
    mod.main(base)


@pytest.mark.parametrize('name', ['train', 'train_classifier', 'train_densepose', 'train_densepose_classifier'])
def test_a_missing_list_ends_the_program_by_name(tmp_path, name):
  cfg = tmp_path / 'c.yaml'
  cfg.write_text({'train': VOC, 'train_densepose': DENSEPOSE, 'train_classifier': classifier(VOC, ''),
                  'train_densepose_classifier': classifier(DENSEPOSE, '')}[name])
  missing = str(tmp_path / 'no_such_list.txt')
  with pytest.raises(SystemExit, match='no_such_list.txt'):
    load_program(name).main(['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--data_dir', str(tmp_path),
                             '--data_list', missing])
