"""Routes of the inference programs (spml_amd/inference_cli.py) on the CPU: every wired program and option combination
runs its real `main` on two synthetic images with what needs a device replaced by recording fakes -- `parse`'s device,
`load_models`, the memory bank, `CrfStage`, the synchronisations, the scoring and the `spml_amd.inference` functions that
run per image, which return tensors of the right shapes under the keys the real ones return.  What is pinned, per
combination: which `spml_amd.inference` function ran per image and the constant keyword arguments it got (`combine`,
`walk_steps`, `alpha`, `floor`, `return_prob`), whether the CRF stage was called from the program, which of `emit` /
`emit_refined` received the result, and the ordered keys of the JSON line.  The table was recorded before the four `run_*`
bodies were cut into a run loop, a label writer and per-image functions chosen before the loop; it is written out here,
not generated.  The models are faked, so no snapshot is written: the tiny config alone is read.

Second part: the layout of the one pinned upload of `ListImageSource.image` (records, RGB, semantic plane, CAM planes)
(`upload_layout`) against a restatement of the arithmetic the method carried inline."""
import contextlib
import inspect
import io
import json
import os

import numpy as np
import pytest
import torch

from spml_amd import inference, inference_cli
from spml_amd.utils.general import metrics
from test_crf_lists_gpu import tiny_config
from test_inference_cli import load_program

CONSTANTS = ('combine', 'walk_steps', 'alpha', 'floor', 'return_prob')
SIZE, NCLS = 65, 2                                       # of `tiny_config`
COMMON = ['images', 'images_per_s', 'mIoU', 'pixel_acc']
CRF = ['mIoU_before_crf', 'changed_by_crf', 'crf_path', 'crf_share']
TAIL = ['snapshot', 'save_dir']
KNN_TAIL = ['memory_prototypes', 'snapshot', 'semantic_memory_dir', 'save_dir']
WALK = {'combine': 'prob_mean', 'walk_steps': 6}
CAM = {'alpha': 6, 'walk_steps': 6}
TAGGED = {'floor': 0.15}

# (program, options) -> (what runs per image, the keys of the JSON line in order)
ROUTES = {
    ('prototype', ()): ([('multiscale_prototypes', {}), 'save_image_memory'],
                        ['images', 'images_per_s', 'prototypes_per_image', 'views', 'scales', 'majority_path'] + TAIL),
    ('prototype_msc', ()): ([('multiscale_prototypes', {}), 'save_image_memory'],
                            ['images', 'images_per_s', 'prototypes_per_image', 'views', 'scales', 'majority_path'] + TAIL),
    ('inference_softmax', ()): ([('predict_softmax_full_resolution', {}), 'emit'], COMMON + ['head_path'] + TAIL),
    ('inference_softmax', ('--crf',)): ([('predict_softmax_full_resolution', {}), 'stage', 'emit_refined'],
                                        COMMON + ['head_path'] + CRF + TAIL),
    ('inference_softmax_crf', ()): ([('predict_softmax_full_resolution', {}), 'stage', 'emit_refined'],
                                    COMMON + ['head_path'] + CRF + TAIL),
    ('inference_softmax_msc', ()): ([('predict_softmax_multiscale', {}), 'emit'],
                                    COMMON + ['views', 'combine_path', 'head_path'] + TAIL),
    ('inference_softmax_msc', ('--crf',)): ([('predict_softmax_multiscale', {}), 'stage', 'emit_refined'],
                                            COMMON + ['views', 'combine_path', 'head_path'] + CRF + TAIL),
    ('inference_softmax_crf_msc', ()): ([('predict_softmax_multiscale', {}), 'stage', 'emit_refined'],
                                        COMMON + ['views', 'combine_path', 'head_path'] + CRF + TAIL),
    ('inference', ()): ([('predict_full_resolution', {}), 'emit'], COMMON + KNN_TAIL),
    ('inference', ('--crf',)): ([('predict_knn_full_resolution_crf', {}), 'emit_refined'],
                                COMMON + ['votes_path'] + CRF + KNN_TAIL),
    ('inference_crf', ()): ([('predict_knn_full_resolution_crf', {}), 'emit_refined'],
                            COMMON + ['votes_path'] + CRF + KNN_TAIL),
    ('inference_msc', ()): ([('predict_knn_multiscale', {}), 'emit'], COMMON + ['views', 'combine_path'] + KNN_TAIL),
    ('inference_msc', ('--crf',)): ([('predict_knn_multiscale', {}), 'stage', 'emit_refined'],
                                    COMMON + ['views', 'combine_path'] + CRF + KNN_TAIL),
    ('inference_crf_msc', ()): ([('predict_knn_multiscale', {}), 'stage', 'emit_refined'],
                                COMMON + ['views', 'combine_path'] + CRF + KNN_TAIL),
    ('inference_msc', ('--pseudo_tags',)): (
        [('pseudo_labels_knn_multiscale', dict(TAGGED, return_prob=False)), 'emit', 'instance_iou'],
        COMMON + ['views', 'combine_path', 'normalize_path', 'instance_mIoU'] + KNN_TAIL),
    ('inference_msc', ('--pseudo_tags', '--crf')): (
        [('pseudo_labels_knn_multiscale', dict(TAGGED, return_prob=True)), 'stage', 'emit_refined', 'instance_iou'],
        COMMON + ['views', 'combine_path', 'normalize_path', 'instance_mIoU'] + CRF + KNN_TAIL),
    ('pseudo_softmax', ()): ([('pseudo_labels_softmax', {'combine': 'logit_mean', 'walk_steps': 0}), 'emit'],
                             COMMON + ['scales', 'is_flip', 'combine', 'walk_steps', 'head_path'] + TAIL),
    ('pseudo_softmaxrw', ()): ([('pseudo_labels_softmax', WALK), 'emit'],
                               COMMON + ['scales', 'is_flip', 'combine', 'walk_steps', 'head_path'] + TAIL),
    ('pseudo_softmaxrw', ('--crf',)): ([('pseudo_labels_softmax_crf', WALK), 'emit_refined'],
                                       COMMON + CRF + ['scales', 'is_flip', 'combine', 'walk_steps', 'head_path'] + TAIL),
    ('pseudo_softmaxrw_crf', ()): ([('pseudo_labels_softmax_crf', WALK), 'emit_refined'],
                                   COMMON + CRF + ['scales', 'is_flip', 'combine', 'walk_steps', 'head_path'] + TAIL),
    ('pseudo_softmaxrw', ('--cam_dir',)): ([('pseudo_labels_cam', CAM), 'emit'],
                                           COMMON + ['scales', 'is_flip', 'cam_dir', 'alpha', 'walk_steps', 'cam_path'] + TAIL),
    ('pseudo_softmaxrw', ('--cam_dir', '--crf')): (
        [('pseudo_labels_cam_crf', CAM), 'emit_refined'],
        COMMON + CRF + ['scales', 'is_flip', 'cam_dir', 'alpha', 'walk_steps', 'cam_path'] + TAIL),
}
# views per image, where the JSON line says so: the flip pairs of the program's scales (pseudo tags: PSEUDO_SCALES)
VIEWS = {'prototype': 1, 'prototype_msc': 3, 'inference_softmax_msc': 10, 'inference_softmax_crf_msc': 10, 'inference_msc': 10,
         'inference_crf_msc': 10}


class FakeStage(object):
  """Stands in for `inference_cli.CrfStage`: a call from the program is written down, the labels come back as zeros."""
  calls = None

  def __init__(self, config, args):
    self.iter_max = args.crf_iter_max

  def __call__(self, image_u8, prob):
    assert image_u8.dtype == torch.uint8 and tuple(image_u8.shape) == tuple(prob.shape[1:]) + (3,)
    self.calls.append('stage')
    return {'semantic_prob': prob, 'semantic_prediction': torch.zeros(prob.shape[1:], dtype=torch.long), 'crf_path': 'fake_crf'}

  def fields(self, seconds):
    return {'crf_path': 'fake_crf', 'crf_share': 0.25}


class FakeInstanceIoU(object):
  calls = None

  def __init__(self, num_classes):
    pass

  def update(self, prediction, label, instance):
    assert prediction.shape == label.shape == instance.shape
    self.calls.append('instance_iou')

  def result(self):
    return {'mean_iou': 12.3456}


def labels(hw, value=0):
  return torch.full(tuple(hw), value, dtype=torch.long)


def fake_results():
  """name of a per-image `spml_amd.inference` function -> its result from the bound arguments: the keys of the real
  one that a program reads, at the real shapes."""
  def walked(path_key, refined):
    def make(a):
      out = {'semantic_prediction': labels(a['image_hw'], 1), path_key: 'fake_' + path_key[:-5]}
      if refined:
        assert tuple(a['image_u8'].shape) == tuple(a['image_hw']) + (3,) and isinstance(a['crf'], FakeStage)
        out.update(semantic_prediction_before_crf=labels(a['image_hw']), crf_path='fake_crf')
      return out
    return make

  def softmax_single(a):
    pad = tuple(a['image'].shape[-2:])
    return {'semantic_logit': torch.zeros((1, NCLS) + pad), 'semantic_prediction': labels(a['valid_hw']), 'head_path': 'fake_head'}

  def multi(extra):
    def make(a):
      prob = torch.ones((NCLS,) + tuple(a['image_hw']))
      if 'label_tags' in a:
        assert a['label_tags'].dtype == torch.bool and a['label_tags'].numel() == NCLS
        prob = prob if a['return_prob'] else None
      return dict({'semantic_prob': prob, 'semantic_prediction': labels(a['image_hw']), 'combine_path': 'fake_combine'}, **extra)
    return make

  def knn_crf(a):
    assert tuple(a['image_u8'].shape) == tuple(a['valid_hw']) + (3,) and isinstance(a['crf'], FakeStage)
    return {'semantic_prediction': labels(a['valid_hw'], 1), 'semantic_prediction_before_crf': labels(a['valid_hw']),
            'crf_path': 'fake_crf', 'votes_path': 'fake_votes'}

  def prototypes(a):
    assert len(a['label_views']) == len(a['views'])
    return {'prototype': torch.zeros((3, 4)), 'prototype_label': torch.zeros((3,), dtype=torch.long), 'majority_path': 'fake_majority'}

  return {'multiscale_prototypes': prototypes,
          'predict_softmax_full_resolution': softmax_single,
          'predict_softmax_multiscale': multi({'head_path': 'fake_head'}),
          'predict_full_resolution': lambda a: {'semantic_prediction': labels(a['valid_hw'])},
          'predict_knn_full_resolution_crf': knn_crf,
          'predict_knn_multiscale': multi({}),
          'pseudo_labels_knn_multiscale': multi({'normalize_path': 'fake_normalize'}),
          'pseudo_labels_softmax': walked('head_path', False), 'pseudo_labels_softmax_crf': walked('head_path', True),
          'pseudo_labels_cam': walked('cam_path', False), 'pseudo_labels_cam_crf': walked('cam_path', True)}


def trace_program(name, options, tmp_path, monkeypatch):
  """Runs `pyscripts/inference/<name>.py` on two synthetic images with the fakes in place.
  -> (the recorded calls in order, the JSON line as an ordered dict)."""
  calls = []
  cfg = tiny_config(tmp_path, NCLS, 'segsort' if name in ('inference', 'inference_crf', 'inference_msc', 'inference_crf_msc',
                                                            'prototype', 'prototype_msc') else 'softmax_classifier')
  real_parse = inference_cli.parse

  def parse(*args, **kwargs):
    with monkeypatch.context() as m:
      m.setattr(torch.cuda, 'is_available', lambda: True)
      m.setattr(torch.cuda, 'set_device', lambda device: None)
      config, parsed, _ = real_parse(*args, **kwargs)
    return config, parsed, torch.device('cpu')

  monkeypatch.setattr(inference_cli, 'parse', parse)
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  monkeypatch.setattr(inference_cli, 'load_models', lambda config, args, device, head, densepose=False:
                      ('embedding model', None if head is None else 'prediction model', 'fake_snapshot'))
  monkeypatch.setattr(inference_cli, 'load_bank', lambda memory_dir, config, device:
                      (torch.zeros((5, 4)), torch.zeros((5,), dtype=torch.long)))
  monkeypatch.setattr(inference_cli, 'CrfStage', type('Stage', (FakeStage,), {'calls': calls}))
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: None)
  monkeypatch.setattr(metrics, 'iou_stats', lambda prediction, label, num_classes, counts=None:
                      torch.zeros((3, num_classes), dtype=torch.int64) if counts is None else counts)
  monkeypatch.setattr(metrics, 'mean_iou', lambda counts: {'mean_iou': 50.0, 'pixel_acc': 60.0})
  monkeypatch.setattr(metrics, 'InstanceIoU', type('Instance', (FakeInstanceIoU,), {'calls': calls}))
  for function, result in fake_results().items():
    def fake(*args, _name=function, _result=result, _signature=inspect.signature(getattr(inference, function)), **kwargs):
      given = _signature.bind(*args, **kwargs).arguments                     # (what the program passed: no defaults)
      calls.append((_name, {k: given[k] for k in CONSTANTS if k in given}))
      return _result(given)
    monkeypatch.setattr(inference, function, fake)
  monkeypatch.setattr(inference, 'save_image_memory', lambda path, prototypes, labels_: calls.append('save_image_memory'))
  monkeypatch.setattr(inference, 'full_resolution_prototypes',               # (the kNN programs' own bank, before the loop)
                      lambda *a: (torch.zeros((3, 4)), torch.zeros((3,), dtype=torch.long), None))
  for method in ('emit', 'emit_refined'):
    def recorded(self, image, *rest, _method=method, _real=getattr(inference_cli.SyntheticImageSource, method)):
      calls.append(_method)
      return _real(self, image, *rest)
    monkeypatch.setattr(inference_cli.SyntheticImageSource, method, recorded)

  argv = ['--snapshot_dir', str(tmp_path / 'none'), '--cfg_path', str(cfg), '--save_dir', str(tmp_path / 'results'),
          '--data_list', 'synthetic']
  for option in options:
    argv.append(option)
    if option == '--cam_dir':
      cams = tmp_path / 'cams'
      os.makedirs(str(cams))
      for index in range(2):
        np.save(str(cams / ('synthetic_%04d.npy' % index)), {0: np.full((SIZE, SIZE), 0.5, np.float32)}, allow_pickle=True)
      argv.append(str(cams))
  printed = io.StringIO()
  with contextlib.redirect_stdout(printed):
    load_program(name).main(argv)
  line, = [l for l in printed.getvalue().splitlines() if l.startswith('{')]
  return calls, json.loads(line)


@pytest.mark.parametrize('name,options', sorted(ROUTES))
def test_route_of_every_program(name, options, tmp_path, monkeypatch):
  per_image, keys = ROUTES[(name, options)]
  calls, result = trace_program(name, options, tmp_path, monkeypatch)
  # the kNN programs build their own bank first: two images' banks, then the loop
  if 'semantic_memory_dir' in keys:
    assert calls[:2] == ['save_image_memory'] * 2
    calls = calls[2:]
  assert calls == per_image * 2
  assert list(result) == keys
  assert result['images'] == 2 and result['snapshot'] == 'fake_snapshot'
  assert result['save_dir'] == str(tmp_path / 'results' / ('semantic_prototype' if name.startswith('prototype') else 'semantic_gray'))
  # the fields that depend on the route carry what the last image's function returned
  for key in ('head_path', 'combine_path', 'votes_path', 'normalize_path', 'cam_path', 'majority_path'):
    if key in keys:
      assert result[key] == 'fake_' + key[:-5], key
  if 'views' in keys:
    assert result['views'] == (8 if '--pseudo_tags' in options else VIEWS[name])
  if 'instance_mIoU' in keys:
    assert result['instance_mIoU'] == 12.3456
  if 'cam_dir' in keys:
    assert result['cam_dir'] == str(tmp_path / 'cams') and result['alpha'] == 6 and result['walk_steps'] == 6
  if 'combine' in keys:
    assert (result['combine'], result['walk_steps']) == (per_image[0][1]['combine'], per_image[0][1]['walk_steps'])
  if 'mIoU' in keys:
    assert (result['mIoU'], result['pixel_acc']) == (50.0, 60.0)
  if 'crf_path' in keys:
    assert result['crf_path'] == 'fake_crf' and result['crf_share'] == 0.25 and result['mIoU_before_crf'] == 50.0
    # the fakes' refined labels differ from the ones before the CRF everywhere, or nowhere where the stage's zeros
    # meet zeros
    assert result['changed_by_crf'] == (0.0 if 'stage' in per_image else 1.0)
  written = sorted(os.listdir(result['save_dir']))
  assert written == ([] if name.startswith('prototype') else ['synthetic_0000.npy', 'synthetic_0001.npy'])


# ------------------------------------------------------------------------------------------------------------------
# the upload layout
def inline_layout(records_nbytes, h, w, has_semantic, num_cam_planes):
  """The arithmetic `ListImageSource.image` carried inline, restated: -> (records end, RGB start, semantic start,
  semantic end, CAM start or None, total)."""
  rec_bytes = (records_nbytes + 15) // 16 * 16
  sem_at = rec_bytes + (3 * h * w + 15) // 16 * 16
  total = sem_end = sem_at + (h * w if has_semantic else 0)
  cam_at = None
  if num_cam_planes:
    cam_at = (sem_end + 15) // 16 * 16
    total = cam_at + 4 * h * w * num_cam_planes
  return records_nbytes, rec_bytes, sem_at, sem_end, cam_at, total


@pytest.mark.parametrize('num_cam_planes', [0, 1, 3])
@pytest.mark.parametrize('has_semantic', [False, True])
@pytest.mark.parametrize('hw', [(97, 129), (129, 110)])
@pytest.mark.parametrize('records_nbytes', [28, 10 * 28, 64])
def test_upload_layout(records_nbytes, hw, has_semantic, num_cam_planes):
  h, w = hw
  assert (h * w) % 16 != 0 and (3 * h * w) % 16 != 0 and (records_nbytes % 16 != 0 or records_nbytes == 64)
  records_end, rgb_at, sem_at, sem_end, cam_at, total = inline_layout(records_nbytes, h, w, has_semantic, num_cam_planes)
  assert tuple(inference_cli.upload_layout(records_nbytes, h, w, has_semantic, num_cam_planes)) == (
      records_end, rgb_at, sem_at, sem_end, cam_at, total)
  regions = [(0, records_end), (rgb_at, rgb_at + 3 * h * w)]
  if has_semantic:
    regions.append((sem_at, sem_end))
  else:
    assert sem_end == sem_at
  if num_cam_planes:
    regions.append((cam_at, cam_at + 4 * h * w * num_cam_planes))
    assert cam_at % 4 == 0                                                   # the planes are read as fp32
  else:
    assert cam_at is None
  for start, _ in regions:
    assert start % 16 == 0
  for (_, end), (start, _) in zip(regions, regions[1:]):
    assert end <= start < end + 16                                           # in order, no overlap, no more than padding
  # the upload ends with the last plane; without planes behind it the RGB region keeps its padding
  assert total == (regions[-1][1] if num_cam_planes else sem_end) and regions[-1][1] <= total < regions[-1][1] + 16
  assert all(end - start > 0 for start, end in regions)
