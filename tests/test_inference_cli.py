"""The shared body of the inference programs (spml_amd/inference_cli.py) and the per-view helpers of
spml_amd/inference.py, as far as they run without a GPU: the guards of all eight programs in their one order, the dense
label rule with both of its empty-image policies, the synthetic image, the crop batching and the view grouping."""
import importlib.util
import os

import pytest
import torch

from spml_amd import inference, inference_cli, synth
from test_train_cli import ROOT, YAML

PROGRAMS = [('inference_softmax', 'predict_softmax_full_resolution'),
            ('inference_softmax_msc', 'predict_softmax_multiscale'),
            ('inference_msc', 'predict_knn_multiscale'),
            ('pseudo_inference_msc', 'pseudo_labels_knn_multiscale'),
            ('prototype', 'multiscale_prototypes'),
            ('prototype_msc', 'multiscale_prototypes'),
            ('pseudo_softmax', 'pseudo_labels_softmax'),
            ('pseudo_softmaxrw', 'pseudo_labels_softmax')]


def load_program(name):
  spec = importlib.util.spec_from_file_location('spml_%s_cli' % name,
                                                os.path.join(ROOT, 'pyscripts', 'inference', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.mark.parametrize('name,api_function', PROGRAMS)
def test_every_program_runs_the_guards_in_one_order(name, api_function, tmp_path):
  prog = load_program(name)
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  common = ['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg)]
  # 1. a file list, before everything else: with no --save_dir and (here) no GPU it is still the file list that is named
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'train.txt'])
  text = str(info.value.code)
  assert info.value.code not in (0, None) and 'ListDataset' in text and 'spml_amd.inference.%s ' % api_function in text
  # 2. a missing --save_dir, before the GPU is asked for
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'synthetic'])
  assert str(info.value.code) == '--save_dir is required'
  # 3. no GPU
  if torch.cuda.is_available():
    return
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'synthetic', '--save_dir', str(tmp_path / 'o')])
  assert info.value.code not in (0, None) and 'no CPU fallback' in str(info.value.code)
  assert not os.path.exists(str(tmp_path / 'o'))              # nothing was written


def test_dense_label_fills_with_the_most_frequent_class_and_keeps_both_empty_policies():
  label = torch.tensor([[3, 3, 254, 255],
                        [3, 7, 254, 255],
                        [7, 254, 254, 255],
                        [255, 255, 255, 255]])
  want = torch.where(label < 21, label, torch.tensor(3))
  before = label.clone()
  assert torch.equal(inference_cli.dense_label(label, 21), want)
  assert torch.equal(inference_cli.dense_label(label, 21, empty_fill=255), want)
  assert torch.equal(label, before)                           # the caller's map is not written
  empty = torch.tensor([[254, 255], [255, 254]])
  assert torch.equal(inference_cli.dense_label(empty, 21), empty)
  assert torch.equal(inference_cli.dense_label(empty, 21, empty_fill=None), empty)
  assert torch.equal(inference_cli.dense_label(empty, 21, empty_fill=255), torch.full((2, 2), 255))


def test_synthetic_image_is_the_seeded_batch_of_the_programs():
  image, label, instance = inference_cli.synthetic_image(1, 65, 21, 'cpu')
  datas, targets = synth.make_batch(1, 65, num_classes=21, seed=4100, device='cpu', palette=(1, 3))
  assert image.dtype == torch.float32 and torch.equal(image, datas['image'])
  assert torch.equal(label, targets['semantic_label'][0]) and torch.equal(instance, targets['instance_label'][0])
  image, label, instance = inference_cli.synthetic_image(0, 65, 2, 'cpu')          # two classes: one object class
  assert tuple(image.shape) == (1, 3, 65, 65) and tuple(label.shape) == (65, 65) == tuple(instance.shape)
  assert set(label.unique().tolist()) <= {0, 1, 254, 255}


class RecordingModel(torch.nn.Module):
  def __init__(self):
    super().__init__()
    self.weight = torch.nn.Parameter(torch.zeros(1))
    self.batches = []

  def generate_embeddings(self, datas, targets=None, resize_as_input=False):
    assert resize_as_input
    self.batches.append(datas['image'])
    return {'embedding': datas['image'][:, :2] * 2}


def test_window_embeddings_batches_crops_across_images_in_window_order():
  gen = torch.Generator().manual_seed(5)
  images = [torch.randn(1, 3, 32, 32, generator=gen) for _ in range(2)]
  model = RecordingModel()
  got = list(inference._window_embeddings(model, images, (16, 16), (8, 8)))
  ends = [int(e) for e in inference.sliding_window_ends(32, 16, 8)]
  assert ends == [16, 24, 32]
  want = [(k, eh - 16, ew - 16) for k in range(2) for eh in ends for ew in ends]     # image-major, rows outer
  assert [g[:3] for g in got] == want and len(want) == 18
  assert [b.shape[0] for b in model.batches] == [8, 8, 2]                            # the second spans both images
  crops = torch.cat(model.batches, 0)
  for i, (k, sh, sw, emb) in enumerate(got):
    crop = images[k][:, :, sh:sh + 16, sw:sw + 16]
    assert torch.equal(crops[i:i + 1], crop)
    assert tuple(emb.shape) == (1, 2, 16, 16) and torch.equal(emb, crop[:, :2] * 2)


def test_views_are_grouped_by_consecutive_padded_size():
  views = [(torch.zeros(1, 3, h, w), (h - 1, w - 1), False) for h, w in ((16, 16), (16, 16), (24, 16), (16, 16))]
  groups = inference._group_by_padded_size(views)
  assert [len(g) for g in groups] == [2, 1, 1]
  assert all(a is b for a, b in zip([v for g in groups for v in g], views))          # the views themselves, in call order
