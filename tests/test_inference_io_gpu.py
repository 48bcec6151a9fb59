"""csrc/inference_io.hip on the GPU against the fp64 restatement (tests/inference_io_ref.py), at the shapes of
tests/inference_io_cases.py, and the programs end to end on a list of image files.

Measured on the MI355X over the view cases below: the largest |kernel - fp64| of a resized pixel is 5.604e-07
(`MEASURED_MAX_DEV`; values up to 2.64, about ten fp32 roundings per pixel).  IMAGE_BOUND is four times that."""
import importlib.util
import json
import os

import numpy as np
import PIL.Image as Image
import pytest
import torch

import inference_io_cases as cases
import inference_io_ref as ref
from spml_amd import _ffi, inference
from spml_amd.data import transforms
from spml_amd.utils.general import metrics, vis
from test_train_cli import ROOT, YAML, load_cli

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEASURED_MAX_DEV = 5.604e-07
IMAGE_BOUND = 4 * MEASURED_MAX_DEV
CEILING = 1e-5                  # the project's ceiling for an fp32 image chain


def device_source(hw):
  rgb, semantic = cases.source(hw)
  return rgb, semantic, torch.from_numpy(rgb).to(DEV), torch.from_numpy(semantic).to(DEV)


@pytest.mark.parametrize('with_labels', [False, True])
@pytest.mark.parametrize('hw,scales,is_flip,image_size,sizes', cases.VIEW_CASES)
def test_views_against_the_restatement(hw, scales, is_flip, image_size, sizes, with_labels):
  rgb, semantic, rgb_dev, sem_dev = device_source(hw)
  got = inference.device_views(rgb_dev, scales, is_flip, cases.CROP, cases.MEAN, cases.STD, image_size,
                               semantic_label=sem_dev if with_labels else None)
  views, labels = got if with_labels else (got, None)
  plan = transforms.plan_views(hw[0], hw[1], scales, is_flip, cases.CROP, image_size)
  assert [(v['new_h'], v['new_w']) for v in plan[::2 if is_flip else 1]] == sizes
  want = ref.views(rgb, semantic if with_labels else None, plan, cases.MEAN, cases.STD)
  assert len(views) == len(plan) and (labels is None or len(labels) == len(plan))
  exact = ref.normalise_f32(rgb, cases.MEAN, cases.STD).transpose(2, 0, 1)
  base = views[0][0].untyped_storage().data_ptr()
  worst = 0.0
  for k, (view, p, (want_image, want_label)) in enumerate(zip(views, plan, want)):
    image, valid_hw, flip = view
    new_h, new_w = p['new_h'], p['new_w']
    assert tuple(image.shape) == (1, 3, p['pad_h'], p['pad_w']) and image.dtype == torch.float32 and image.is_contiguous()
    assert valid_hw == (new_h, new_w) and flip == bool(p['flip'])
    assert image.untyped_storage().data_ptr() == base and image.data_ptr() == base + p['image_off']      # one allocation
    host = image[0].cpu().numpy()
    inside = np.zeros(host.shape, dtype=bool)
    inside[:, :new_h, :new_w] = True
    assert np.array_equal(host[~inside], np.zeros((int((~inside).sum()),), np.float32))       # the padding: exactly 0
    if (new_h, new_w) == tuple(hw):                                                            # scale 1: the byte itself
      assert np.array_equal(host[:, :new_h, :new_w], exact[:, :, ::-1] if flip else exact)
    dev = float(np.abs(host.astype(np.float64) - want_image).max())
    worst = max(worst, dev)
    print('view %d of %r (%d x %d, flip %d): max |kernel - fp64| = %.3e' % (k, hw, new_h, new_w, flip, dev))
    if with_labels:
      label = labels[k]
      assert label.dtype == torch.int64 and tuple(label.shape) == (new_h, new_w)
      assert np.array_equal(label.cpu().numpy(), want_label)                                   # bit for bit
  print('%r: worst %.3e (IMAGE_BOUND %.3e)' % (hw, worst, IMAGE_BOUND))
  assert IMAGE_BOUND < CEILING
  assert worst <= IMAGE_BOUND
  again = inference.device_views(rgb_dev, scales, is_flip, cases.CROP, cases.MEAN, cases.STD, image_size,
                                 semantic_label=sem_dev if with_labels else None)
  again = again[0] if with_labels else again
  assert all(torch.equal(a[0], b[0]) for a, b in zip(views, again))


def test_refused_view_records_touch_nothing():
  hw = (23, 37)
  _, _, rgb_dev, sem_dev = device_source(hw)
  plan = transforms.plan_views(hw[0], hw[1], cases.SCALES, True, cases.CROP)
  records = inference.view_records(plan)
  image_bytes, label_bytes = transforms.view_buffer_bytes(plan)
  mean, std = inference._normalisation(torch.device(DEV), cases.MEAN, cases.STD)
  images = torch.full((image_bytes // 4,), 7.0, device=DEV)
  labels = torch.full((label_bytes // 8,), 7, dtype=torch.int64, device=DEV)

  def call(r, images=images, labels=labels, semantic=sem_dev):
    params_dev = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).to(DEV)
    _ffi.image_views(rgb_dev, semantic, r, params_dev, mean, std, images, labels)
  for fields in (dict(pad_h=10), dict(new_w=0), dict(image_off=image_bytes), dict(label_off=int(records['label_off'][1]))):
    bad = records.copy()
    for key, value in fields.items():
      bad[key][0] = value
    with pytest.raises(_ffi.SpmlHipError, match='status -2'):
      call(bad)
  with pytest.raises(_ffi.SpmlHipError, match='status -2'):
    call(records, images=images[:-1])                                     # the last plane leaves the buffer
  torch.cuda.synchronize()
  assert bool((images == 7.0).all()) and bool((labels == 7).all())
  # an output that overlaps an input
  n = 3 * hw[0] * hw[1]
  shared = torch.zeros((image_bytes + 16,), dtype=torch.uint8, device=DEV)
  with pytest.raises(_ffi.SpmlHipError, match='status -1'):
    _ffi.image_views(shared[:n].view(hw[0], hw[1], 3), None, records,
                     torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).to(DEV), mean, std,
                     shared[:image_bytes].view(torch.float32), None)
  call(records)                                                           # and the records as planned run
  want = inference.device_views(rgb_dev, cases.SCALES, True, cases.CROP, cases.MEAN, cases.STD, semantic_label=sem_dev)
  for p, (view, _, _), label in zip(plan, *want):
    at, lat = p['image_off'] // 4, p['label_off'] // 8
    assert torch.equal(images[at:at + view.numel()], view.reshape(-1))
    assert torch.equal(labels[lat:lat + label.numel()], label.reshape(-1))


@pytest.mark.parametrize('pred_hw,valid_hw,out_hw', cases.EXPORT_CASES)
def test_export_against_the_restatement(pred_hw, valid_hw, out_hw):
  pred, table = cases.prediction(pred_hw, valid_hw), cases.color_map()
  assert set(np.unique(pred[:valid_hw[0], :valid_hw[1]])) == set(range(256))
  want_gray, want_rgb = ref.export(pred, valid_hw, out_hw, table)
  pred_dev, table_dev = torch.from_numpy(pred).to(DEV), torch.from_numpy(table).to(DEV)
  gray, rgb = inference.export_label_map(pred_dev, valid_hw, out_hw, table_dev)
  assert gray.dtype == torch.uint8 and tuple(gray.shape) == out_hw and tuple(rgb.shape) == out_hw + (3,)
  assert np.array_equal(gray.cpu().numpy(), want_gray) and np.array_equal(rgb.cpu().numpy(), want_rgb)
  if valid_hw == out_hw:
    assert np.array_equal(want_gray, pred[:valid_hw[0], :valid_hw[1]].astype(np.uint8))      # the identity
    assert set(np.unique(want_gray)) == set(range(256))
  again = inference.export_label_map(pred_dev, valid_hw, out_hw, table_dev)
  assert torch.equal(again[0], gray) and torch.equal(again[1], rgb)
  # into slices of one buffer, as the programs call it; a refusal touches nothing
  px = out_hw[0] * out_hw[1]
  out = torch.full((4 * px,), 9, dtype=torch.uint8, device=DEV)
  with pytest.raises(_ffi.SpmlHipError, match='status -2'):
    inference.export_label_map(pred_dev, (pred_hw[0] + 1, pred_hw[1]), out_hw, table_dev,
                               out=(out[:px].view(out_hw), out[px:].view(out_hw + (3,))))
  torch.cuda.synchronize()
  assert bool((out == 9).all())
  inference.export_label_map(pred_dev, valid_hw, out_hw, table_dev, out=(out[:px].view(out_hw), out[px:].view(out_hw + (3,))))
  assert torch.equal(out[:px].view(out_hw), gray) and torch.equal(out[px:].view(out_hw + (3,)), rgb)


# ------------------------------------------------------------------------------------------------------------------
# end to end: the programs on a list of four image files
FILES = [('a.png', (61, 83)), ('b.png', (83, 61)), ('sub/c.png', (70, 97)), ('d.png', (97, 97))]


def load_program(name):
  spec = importlib.util.spec_from_file_location('spml_%s_cli' % name, os.path.join(ROOT, 'pyscripts', 'inference', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def load_train_classifier():
  spec = importlib.util.spec_from_file_location('spml_train_classifier_cli', os.path.join(ROOT, 'pyscripts', 'train', 'train_classifier.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.fixture(scope='module')
def work(tmp_path_factory):
  """Classifier snapshot (stage 1 -> stage 2) made as tests/test_softmax_inference_gpu.py makes its own (129 x 129 images, 2 x 2
  windows), and the list of four PNG files with labels."""
  root = tmp_path_factory.mktemp('inference_io')
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101')
          .replace('stride:\n    - 97\n    - 97', 'stride:\n    - 64\n    - 64').replace('image_size: 97', 'image_size: 129')
          .replace('color_map_path: "misc/colormapvoc.mat"', 'color_map_path: ""'))
  assert 'image_size: 129' in yaml and yaml.count('- 64') == 2 and 'color_map_path: ""' in yaml
  stage1 = root / 'config_emb.yaml'
  stage1.write_text(yaml)
  snap1 = root / 'stage1'
  load_cli().main(['--snapshot_dir', str(snap1), '--cfg_path', str(stage1), '--data_list', 'synthetic'])
  cfg = root / 'config_classifier.yaml'
  cfg.write_text(yaml.replace('prediction_types: segsort', 'prediction_types: softmax_classifier')
                 .replace('kmeans_iterations: 3', 'kmeans_iterations: 0')
                 .replace('pretrained: ""', 'pretrained: "%s"' % str(snap1 / 'model-1.pth')))
  snap2 = root / 'stage2'
  load_train_classifier().main(['--snapshot_dir', str(snap2), '--cfg_path', str(cfg), '--data_list', 'synthetic'])
  # a snapshot with the kNN predictor, written as tests/test_knn_msc_gpu.py writes its own (train.py's holds the
  # SegsortSoftmax head, which the strict load of `segsort` refuses)
  from spml_amd.config.default import config, update_config
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  from spml_amd.models.predictions.segsort import segsort
  update_config(str(stage1))
  torch.manual_seed(9)
  snap3 = root / 'knn'
  os.makedirs(str(snap3))
  torch.save({'embedding_model': resnet_101_deeplab(config).state_dict(), 'prediction_model': segsort(config).state_dict()},
             str(snap3 / 'model-{:d}.pth'.format(config.train.max_iteration - 1)))
  data = root / 'data'
  rng = np.random.RandomState(77)
  lines, files = [], []
  for name, (h, w) in FILES:
    rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
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
  return {'root': root, 'knn': (str(snap3), str(stage1)), 'stage2': (str(snap2), str(cfg)), 'data': str(data),
          'list': str(data_list), 'files': files}


def run(name, work, stage, save, capsys, *extra):
  snap, cfg = work[stage]
  capsys.readouterr()
  load_program(name).main(['--snapshot_dir', snap, '--cfg_path', cfg, '--save_dir', str(save), '--data_dir', work['data'],
                           '--data_list', work['list']] + list(extra))
  return json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])


def check_label_folders(save, work, result):
  """Both PNG folders at the files' own sizes, colour == table[gray], the JSON mIoU == the score of the written files."""
  table, counts, maps = vis.voc_color_map(), None, []
  for name, rgb, semantic in work['files']:
    gray, color = Image.open(str(save / 'semantic_gray' / name)), Image.open(str(save / 'semantic_color' / name))
    assert gray.mode == 'L' and color.mode == 'RGB'
    gray, color = np.array(gray), np.array(color)
    assert gray.shape == semantic.shape and gray.dtype == np.uint8 and np.array_equal(color, table[gray])
    assert set(np.unique(gray)) <= set(range(21))
    counts = metrics.iou_stats(torch.from_numpy(gray).to(DEV), torch.from_numpy(semantic).to(DEV), 21, counts)
    maps.append(gray)
  assert sorted(os.listdir(str(save / 'semantic_gray'))) == sorted(n for n, _, _ in work['files'])
  score = metrics.mean_iou(counts)
  assert result['images'] == len(work['files']) and result['images_per_s'] > 0
  assert result['mIoU'] == round(score['mean_iou'], 4) and result['pixel_acc'] == round(score['pixel_acc'], 4)
  assert result['data_list'] == work['list'] and result['has_labels'] is True
  return maps


def models_of(work, stage, head):
  from spml_amd import inference_cli as cli
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  snap, cfg = work[stage]
  args = parse_args('x', ['--snapshot_dir', snap, '--cfg_path', cfg])
  device = torch.device(DEV)
  return config, cli.load_models(config, args, device, head)[:2], cli.geometry(config)


def test_softmax_programs_on_a_file_list(work, tmp_path, capsys):
  single = run('inference_softmax', work, 'stage2', tmp_path / 'single', capsys)
  single_maps = check_label_folders(tmp_path / 'single', work, single)
  msc = run('inference_softmax_msc', work, 'stage2', tmp_path / 'msc', capsys)
  msc_maps = check_label_folders(tmp_path / 'msc', work, msc)
  assert msc['views'] == 10
  # the label maps equal a direct call of the API function on device_views of the same bytes
  config, (embedding_model, prediction_model), (_, crop_size, stride, _) = models_of(work, 'stage2', 'softmax_classifier')
  mean, std, table = config.network.pixel_means, config.network.pixel_stds, torch.from_numpy(vis.voc_color_map()).to(DEV)
  scales = load_program('inference_softmax_msc').SCALES
  for (name, rgb, _), single_map, msc_map in zip(work['files'], single_maps, msc_maps):
    h, w = rgb.shape[:2]
    rgb_dev = torch.from_numpy(rgb).to(DEV)
    (image, valid_hw, _), = inference.device_views(rgb_dev, [1], False, crop_size, mean, std, image_size=config.test.image_size)
    assert max(valid_hw) in (128, 129)                      # (int(ratio * side) may leave the larger side one short)
    out = inference.predict_softmax_full_resolution(embedding_model, prediction_model, image, valid_hw, crop_size, stride)
    gray, _ = inference.export_label_map(out['semantic_prediction'], valid_hw, (h, w), table)
    assert np.array_equal(gray.cpu().numpy(), single_map), name
    views = inference.device_views(rgb_dev, scales, True, crop_size, mean, std)
    out = inference.predict_softmax_multiscale(embedding_model, prediction_model, views, (h, w), crop_size, stride)
    assert np.array_equal(out['semantic_prediction'].cpu().numpy().astype(np.uint8), msc_map), name
  # pseudo labels from the same list: the tags come from the files' labels, the PNG folders are written
  pseudo = run('pseudo_softmax', work, 'stage2', tmp_path / 'pseudo', capsys)
  check_label_folders(tmp_path / 'pseudo', work, pseudo)
  for name, _, semantic in work['files']:
    gray = np.array(Image.open(str(tmp_path / 'pseudo' / 'semantic_gray' / name)))
    assert set(np.unique(gray)) <= set(np.unique(semantic)) | {0, 255}                       # tagged classes (+ background / ignore)


def test_memory_bank_programs_on_a_file_list(work, tmp_path, capsys):
  from spml_amd.utils.segsort import others as segsort_others
  bank = run('prototype', work, 'knn', tmp_path / 'bank', capsys)
  assert bank['images'] == 4 and bank['views'] == 1 and bank['data_list'] == work['list']
  memory_dir = str(tmp_path / 'bank' / 'semantic_prototype')
  assert sorted(os.listdir(memory_dir)) == sorted(n.replace('.png', '.npy') for n, _, _ in work['files'])
  prototypes, labels = segsort_others.load_memory_banks(memory_dir)
  assert prototypes.shape[0] == sum(bank['prototypes_per_image']) == labels.shape[0]
  present = set(np.unique(np.concatenate([s.reshape(-1) for _, _, s in work['files']])))
  assert set(labels.unique().tolist()) <= present
  result = run('inference', work, 'knn', tmp_path / 'knn', capsys, '--semantic_memory_dir', memory_dir)
  check_label_folders(tmp_path / 'knn', work, result)
  assert result['semantic_memory_dir'] == memory_dir
  # without a bank a data list is refused
  with pytest.raises(SystemExit, match='semantic_memory_dir'):
    run('inference', work, 'knn', tmp_path / 'none', capsys)
  bank_msc = run('prototype_msc', work, 'knn', tmp_path / 'bank_msc', capsys)
  assert bank_msc['views'] == 3
  result = run('inference_msc', work, 'knn', tmp_path / 'knn_msc', capsys, '--semantic_memory_dir',
               str(tmp_path / 'bank_msc' / 'semantic_prototype'))
  check_label_folders(tmp_path / 'knn_msc', work, result)
  assert result['views'] == 10
