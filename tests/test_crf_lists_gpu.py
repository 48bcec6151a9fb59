"""The dense CRF on image lists on the GPU: `spml_crf_guide_u8` and `spml_label_export_scored_u8` against the numpy
restatements (tests/crf_lists_ref.py) at the shapes of tests/inference_io_cases.py, the five programs with `--crf` on a
list of four PNG files, and `prog --crf` against its `*_crf*` sibling on synthetic images.

The resized guide is held to the fp64 restatement through the bound the views already hold (`IMAGE_BOUND` of
tests/test_inference_io_gpu.py, on the normalised value): the chain multiplies by `255 * std[c]` and is monotone, so a
byte may differ from the restatement's by one, and only where the restatement's value before the truncation lies within
`255 * std[c] * IMAGE_BOUND` of an integer."""
import json
import os

import numpy as np
import PIL.Image as Image
import pytest
import torch

import crf_lists_ref as crf_ref
import inference_io_cases as cases
from spml_amd import _ffi, inference, inference_cli
from spml_amd.utils.general import metrics, vis
from test_dense_crf_gpu import tiny_config, write_snapshot
from test_inference_io_gpu import IMAGE_BOUND, check_label_folders, load_program
from test_train_cli import YAML

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CRF_PROGRAMS = ['inference_softmax', 'inference_softmax_msc', 'inference', 'inference_msc', 'pseudo_softmaxrw']
SIBLING = {'inference_softmax': 'inference_softmax_crf', 'inference_softmax_msc': 'inference_softmax_crf_msc',
           'inference': 'inference_crf', 'inference_msc': 'inference_crf_msc', 'pseudo_softmaxrw': 'pseudo_softmaxrw_crf'}


def unpadded(view):
  image, (rh, rw), flip = view
  assert not flip
  return image[0, :, :rh, :rw]


# ------------------------------------------------------------------------------------------------------------------
# the guide
@pytest.mark.parametrize('hw', [(23, 37), (41, 29)])
def test_guide_at_the_files_size_is_the_table(hw):
  rgb, _ = cases.source(hw)
  assert set(np.unique(rgb)) == set(range(256)) and (3 * hw[0] * hw[1]) % 12 != 0      # (a tail behind the last span)
  rgb_dev = torch.from_numpy(rgb).to(DEV)
  assert _ffi.crf_guide_path_name(hw) == 'guide_table'
  got = inference.crf_guide(rgb_dev, cases.MEAN, cases.STD)
  assert got.dtype == torch.uint8 and tuple(got.shape) == hw + (3,) and got.is_contiguous()
  want = crf_ref.guide_same_size(rgb, cases.MEAN, cases.STD)
  assert np.array_equal(got.cpu().numpy(), want)
  assert int((want.astype(np.int64) != rgb).sum()) > 0                                   # the round trip is lossy here
  view, = inference.device_views(rgb_dev, [1], False, cases.CROP, cases.MEAN, cases.STD)
  assert torch.equal(got, inference.denormalized_uint8(unpadded(view), cases.MEAN, cases.STD))
  # every byte is written, into a buffer of the caller's too
  mean, std = inference._normalisation(torch.device(DEV), cases.MEAN, cases.STD)
  for fill in (0, 255):
    out = torch.full(hw + (3,), fill, dtype=torch.uint8, device=DEV)
    _ffi.crf_guide(rgb_dev, mean, std, cases.MEAN, cases.STD, out=out)
    assert torch.equal(out, got)


@pytest.mark.parametrize('hw,new_hw,how', [((23, 43), (12, 22), dict(scales=[1], image_size=23)),
                                           ((23, 37), (40, 64), dict(scales=[1.75]))])
def test_resized_guide_is_the_denormalised_view(hw, new_hw, how):
  rgb, _ = cases.source(hw)
  rgb_dev = torch.from_numpy(rgb).to(DEV)
  assert _ffi.crf_guide_path_name(hw, new_hw) == 'guide_resized'
  got = inference.crf_guide(rgb_dev, cases.MEAN, cases.STD, new_hw)
  assert got.dtype == torch.uint8 and tuple(got.shape) == new_hw + (3,)
  view, = inference.device_views(rgb_dev, how['scales'], False, cases.CROP, cases.MEAN, cases.STD, how.get('image_size', 0))
  assert view[1] == new_hw
  assert torch.equal(got, inference.denormalized_uint8(unpadded(view), cases.MEAN, cases.STD))      # the shared code
  want, before_cut = crf_ref.guide_resized(rgb, new_hw, cases.MEAN, cases.STD)
  diff = got.cpu().numpy().astype(np.int64) - want.astype(np.int64)
  near = np.abs(before_cut - np.rint(before_cut)) <= 255.0 * np.asarray(cases.STD) * IMAGE_BOUND
  print('%r -> %r: %d of %d bytes differ from the fp64 restatement, %d values within the bound of an integer'
        % (hw, new_hw, int((diff != 0).sum()), diff.size, int(near.sum())))
  assert int(np.abs(diff).max()) <= 1
  assert not (diff != 0)[~near].any()
  for fill in (0, 255):
    mean, std = inference._normalisation(torch.device(DEV), cases.MEAN, cases.STD)
    out = torch.full(new_hw + (3,), fill, dtype=torch.uint8, device=DEV)
    _ffi.crf_guide(rgb_dev, mean, std, cases.MEAN, cases.STD, new_hw, out=out)
    assert torch.equal(out, got)


# ------------------------------------------------------------------------------------------------------------------
# the scored export
@pytest.mark.parametrize('ncls', [1, 21, 256])
@pytest.mark.parametrize('pred_hw,valid_hw,out_hw', cases.EXPORT_CASES)
def test_scored_export(pred_hw, valid_hw, out_hw, ncls):
  refined, before = cases.prediction(pred_hw, valid_hw), cases.prediction(pred_hw, valid_hw, seed=1)
  truth, table = cases.source(out_hw)[1], cases.color_map()
  assert {254, 255, 20} <= set(np.unique(truth))
  refined_dev, before_dev, truth_dev, table_dev = (torch.from_numpy(a).to(DEV) for a in (refined, before, truth, table))
  want_gray, want_rgb = inference.export_label_map(refined_dev, valid_hw, out_hw, table_dev)
  before_gray, _ = inference.export_label_map(before_dev, valid_hw, out_hw, table_dev)
  gray, rgb, scores = inference.export_scored_label_map(refined_dev, before_dev, valid_hw, out_hw, table_dev, truth_dev, ncls)
  assert torch.equal(gray, want_gray) and torch.equal(rgb, want_rgb)
  assert scores.dtype == torch.int64 and scores.numel() == 2 * 3 * ncls + 1 == _ffi.export_scores_bytes(ncls) // 8
  tables = torch.stack([metrics.iou_stats(want_gray, truth_dev, ncls), metrics.iou_stats(before_gray, truth_dev, ncls)])
  changed = int((want_gray != before_gray).sum())
  assert changed > 0 and int(tables[0, 0].sum()) == int((truth.astype(np.int64) < ncls).sum())
  assert torch.equal(scores[:-1].view(2, 3, ncls), tables) and int(scores[-1]) == changed
  for k, exported in enumerate((want_gray, before_gray)):
    assert np.array_equal(tables[k].cpu().numpy(), crf_ref.iou_counts(exported.cpu().numpy(), truth, ncls))
  # a second call adds into the same tensor
  again = inference.export_scored_label_map(refined_dev, before_dev, valid_hw, out_hw, table_dev, truth_dev, ncls, scores)
  assert again[2] is scores and torch.equal(again[0], want_gray) and torch.equal(again[1], want_rgb)
  assert torch.equal(scores[:-1].view(2, 3, ncls), 2 * tables) and int(scores[-1]) == 2 * changed
  # without the labels before the CRF: their table and the counter stay; without the ground truth: both tables stay
  start = torch.arange(2 * 3 * ncls + 1, dtype=torch.int64, device=DEV) + 5
  some = start.clone()
  gray, rgb, _ = inference.export_scored_label_map(refined_dev, None, valid_hw, out_hw, table_dev, truth_dev, ncls, some)
  assert torch.equal(gray, want_gray) and torch.equal(rgb, want_rgb)
  assert torch.equal(some[:3 * ncls], start[:3 * ncls] + tables[0].reshape(-1)) and torch.equal(some[3 * ncls:], start[3 * ncls:])
  some = start.clone()
  gray, rgb, _ = inference.export_scored_label_map(refined_dev, before_dev, valid_hw, out_hw, table_dev, None, ncls, some)
  assert torch.equal(gray, want_gray) and torch.equal(rgb, want_rgb)
  assert torch.equal(some[:-1], start[:-1]) and int(some[-1]) == int(start[-1]) + changed
  # a refusal touches nothing
  some = start.clone()
  with pytest.raises(_ffi.SpmlHipError, match='status -2'):
    inference.export_scored_label_map(refined_dev, before_dev, (pred_hw[0] + 1, pred_hw[1]), out_hw, table_dev, truth_dev,
                                      ncls, some, out=(gray.fill_(9), rgb.fill_(9)))
  torch.cuda.synchronize()
  assert torch.equal(some, start) and bool((gray == 9).all()) and bool((rgb == 9).all())


# ------------------------------------------------------------------------------------------------------------------
# the five programs with --crf on a list of four PNG files
FILES = [('a.png', (97, 129)), ('b.png', (129, 97)), ('sub/c.png', (129, 110)), ('d.png', (129, 129))]
CRF_OPTIONS = ['--crf', '--crf_iter_max', '2']
# the keys of the JSON line of the commit before `--crf` (a file list): a run without the option must keep them
PARENT_KEYS = {
    'inference_softmax': {'images', 'images_per_s', 'mIoU', 'pixel_acc', 'head_path', 'snapshot', 'save_dir', 'data_list', 'has_labels'},
    'inference_softmax_msc': {'images', 'images_per_s', 'mIoU', 'pixel_acc', 'views', 'head_path', 'combine_path', 'snapshot',
                              'save_dir', 'data_list', 'has_labels'},
    'inference': {'images', 'images_per_s', 'mIoU', 'pixel_acc', 'memory_prototypes', 'snapshot', 'semantic_memory_dir',
                  'save_dir', 'data_list', 'has_labels'},
    'inference_msc': {'images', 'images_per_s', 'mIoU', 'pixel_acc', 'views', 'combine_path', 'memory_prototypes', 'snapshot',
                      'semantic_memory_dir', 'save_dir', 'data_list', 'has_labels'},
    'pseudo_softmaxrw': {'images', 'images_per_s', 'mIoU', 'pixel_acc', 'scales', 'is_flip', 'combine', 'walk_steps', 'head_path',
                         'snapshot', 'save_dir', 'data_list', 'has_labels'}}
CRF_KEYS = {'crf_path', 'crf_share', 'mIoU_before_crf', 'changed_by_crf'}


def seeded_snapshot(root, name, cfg, head):
  """`torch.save` of freshly seeded models (no training), as the `knn` snapshot of tests/test_inference_io_gpu.py."""
  from spml_amd.config.default import config, update_config
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.models.predictions.softmax_classifier import softmax_classifier
  update_config(str(cfg))
  torch.manual_seed(9)
  snap = root / name
  os.makedirs(str(snap))
  prediction = (segsort if head == 'segsort' else softmax_classifier)(config).state_dict()
  torch.save({'embedding_model': resnet_101_deeplab(config).state_dict(), 'prediction_model': prediction},
             str(snap / 'model-{:d}.pth'.format(config.train.max_iteration - 1)))
  return str(snap)


@pytest.fixture(scope='module')
def work(tmp_path_factory):
  root = tmp_path_factory.mktemp('crf_lists')
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101')
          .replace('stride:\n    - 97\n    - 97', 'stride:\n    - 64\n    - 64')
          .replace('color_map_path: "misc/colormapvoc.mat"', 'color_map_path: ""'))
  assert 'image_size: 97' in yaml and yaml.count('- 64') == 2 and 'color_map_path: ""' in yaml
  knn_cfg, softmax_cfg = root / 'config_knn.yaml', root / 'config_softmax.yaml'
  knn_cfg.write_text(yaml)
  softmax_cfg.write_text(yaml.replace('prediction_types: segsort', 'prediction_types: softmax_classifier')
                         .replace('kmeans_iterations: 3', 'kmeans_iterations: 0'))
  stages = {'knn': (seeded_snapshot(root, 'knn', knn_cfg, 'segsort'), str(knn_cfg)),
            'softmax': (seeded_snapshot(root, 'softmax', softmax_cfg, 'softmax_classifier'), str(softmax_cfg))}
  data = root / 'data'
  rng = np.random.RandomState(78)
  lines, files = [], []
  for name, (h, w) in FILES:
    rgb = np.repeat(np.repeat(rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)), 8, 0), 8, 1)[:h, :w]
    rgb = np.clip(rgb + rng.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
    semantic = np.repeat(np.repeat(rng.choice(np.array([0, 3, 7, 255], np.uint8), (h // 16 + 1, w // 16 + 1)), 16, 0), 16, 1)[:h, :w]
    semantic = np.ascontiguousarray(semantic)
    for sub, array, mode in (('img', rgb, 'RGB'), ('lab', semantic, 'L')):
      path = data / sub / name
      os.makedirs(str(path.parent), exist_ok=True)
      Image.fromarray(array, mode=mode).save(str(path))
    lines.append('img/%s lab/%s lab/%s' % (name, name, name))
    files.append((os.path.basename(name), rgb, semantic))
  data_list = data / 'val.txt'
  data_list.write_text('\n'.join(lines) + '\n')
  assert all(max(hw) == 129 for _, hw in FILES) and len({hw for _, hw in FILES}) >= 2
  assert any(h > w for _, (h, w) in FILES) and any(w > h for _, (h, w) in FILES)
  return dict(stages, root=root, data=str(data), list=str(data_list), files=files)


def run(name, work, stage, save, capsys, *extra):
  snap, cfg = work[stage]
  capsys.readouterr()
  load_program(name).main(['--snapshot_dir', snap, '--cfg_path', cfg, '--save_dir', str(save), '--data_dir', work['data'],
                           '--data_list', work['list']] + list(extra))
  return json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])


@pytest.fixture(scope='module')
def banks(work, tmp_path_factory):
  """The memory banks of the two kNN programs, written by the memory-bank programs from the same list."""
  root = tmp_path_factory.mktemp('crf_lists_banks')
  snap, cfg = work['knn']
  out = {}
  for name, prog in (('inference', 'prototype'), ('inference_msc', 'prototype_msc')):
    load_program(prog).main(['--snapshot_dir', snap, '--cfg_path', cfg, '--save_dir', str(root / prog), '--data_dir',
                             work['data'], '--data_list', work['list']])
    out[name] = ['--semantic_memory_dir', str(root / prog / 'semantic_prototype')]
  return out


@pytest.mark.parametrize('name', CRF_PROGRAMS)
def test_program_with_crf_on_a_file_list(name, work, banks, tmp_path, capsys):
  stage = 'knn' if name in banks else 'softmax'
  extra = banks.get(name, [])
  plain = run(name, work, stage, tmp_path / 'plain', capsys, *extra)
  check_label_folders(tmp_path / 'plain', work, plain)
  assert set(plain) == PARENT_KEYS[name]                                   # nothing of the CRF without the option
  result = run(name, work, stage, tmp_path / 'crf', capsys, *(extra + CRF_OPTIONS))
  maps = check_label_folders(tmp_path / 'crf', work, result)               # sizes, colour == table[gray], the JSON mIoU
  assert set(result) >= PARENT_KEYS[name] | CRF_KEYS
  assert result['crf_path'].startswith('pairs_mfma_') and 0.0 < result['crf_share'] < 1.0
  assert 0.0 <= result['changed_by_crf'] <= 1.0 and 0.0 <= result['mIoU_before_crf'] <= 100.0
  if stage == 'knn':
    return
  # the labels before the CRF are the plain run's: the same score, and the share of pixels that differ between the two
  # runs' files is what the CRF changed
  assert result['mIoU_before_crf'] == plain['mIoU']
  differ = sum(int((np.array(Image.open(str(tmp_path / 'plain' / 'semantic_gray' / n))) != m).sum())
               for (n, _, _), m in zip(work['files'], maps))
  assert result['changed_by_crf'] == round(differ / float(sum(m.size for m in maps)), 4)
  if name != 'inference_softmax_msc':
    return
  # the written maps equal a direct call on the same bytes
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  snap, cfg = work[stage]
  args = parse_args('x', ['--snapshot_dir', snap, '--cfg_path', cfg] + CRF_OPTIONS[1:])
  embedding_model, prediction_model, _ = inference_cli.load_models(config, args, torch.device(DEV), 'softmax_classifier')
  _, crop_size, stride, _ = inference_cli.geometry(config)
  mean, std = config.network.pixel_means, config.network.pixel_stds
  crf = inference_cli.CrfStage(config, args).crf
  scales = load_program(name).SCALES
  for (fname, rgb, _), got in zip(work['files'], maps):
    rgb_dev = torch.from_numpy(rgb).to(DEV)
    views = inference.device_views(rgb_dev, scales, True, crop_size, mean, std)
    out = inference.predict_softmax_multiscale(embedding_model, prediction_model, views, rgb.shape[:2], crop_size, stride)
    prob = out['semantic_prob'] / torch.full((), float(len(views)), device=DEV)
    refined = inference.dense_crf_refine(inference.crf_guide(rgb_dev, mean, std), prob, crf)
    assert np.array_equal(refined['semantic_prediction'].cpu().numpy().astype(np.uint8), got), fname


# ------------------------------------------------------------------------------------------------------------------
# prog --crf against its *_crf* sibling on synthetic images
@pytest.mark.parametrize('name', CRF_PROGRAMS)
def test_crf_option_equals_the_sibling_on_synthetic_images(name, tmp_path, capsys, monkeypatch):
  head = 'segsort' if name in ('inference', 'inference_msc') else 'softmax_classifier'
  cfg = tiny_config(tmp_path, 2, head)
  snap = write_snapshot(tmp_path, cfg, head)
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  save = tmp_path / 'results'
  common = ['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic',
            '--crf_iter_max', '2']
  if head == 'segsort':
    common += ['--kmeans_num_clusters', '4,4', '--label_divisor', '2048']
  results, maps = [], []
  for prog, extra in ((SIBLING[name], []), (name, ['--crf'])):
    capsys.readouterr()
    load_program(prog).main(common + extra)
    results.append(json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]))
    maps.append([np.load(str(save / 'semantic_gray' / ('synthetic_%04d.npy' % i))) for i in range(2)])
    for i in range(2):
      os.remove(str(save / 'semantic_gray' / ('synthetic_%04d.npy' % i)))
  sibling, option = results
  assert all(a.dtype == np.uint8 and a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(*maps))
  assert CRF_KEYS <= set(option)
  for key in set(sibling) - {'images_per_s', 'crf_share'}:
    assert option[key] == sibling[key], key
