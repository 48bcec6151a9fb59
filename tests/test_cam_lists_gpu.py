"""The image-tag recipe on image files, on the GPU: `spml_cam_ingest_f32` against the fp64 four-tap expression
(tests/cam_ingest_ref.py), `pseudo_labels_cam` / `pseudo_labels_cam_crf` on a seeded network, `pseudo_softmaxrw.py
--cam_dir [--crf]` and `inference_msc.py --pseudo_tags` on a list of PNG files of different sizes, and `inference_msc.py
--pseudo_tags [--crf]` against `pseudo_inference_msc.py` / `pseudo_inference_crf_msc.py` on synthetic images.

The kernel's bound per case is `max |G - Y| <= 4 * max(max |R - Y|, 2^-24 * max |Y|)` (see cam_ingest_ref).  Measured on
an MI355X, in units of 2^-24 * max |Y| (the kernel sums and takes the power in fp64 and rounds once, so it stays within
one rounding of Y; the reference's own deviation R - Y in brackets):
  8x8x21 k0: 0.00 (0.00)    9x15x2 k1: 0.77 (3.19)    17x23x3 k2: 0.45 (1.26)
  41x16x21 k1: 0.69 (1.42)  33x40x21 k20: 0.58 (1.24)  97x129x21 k3: 0.57 (1.43)"""
import json
import os

import numpy as np
import PIL.Image as Image
import pytest
import torch

import cam_ingest_ref as ref
from spml_amd import _ffi, inference, inference_cli
from test_crf_lists_gpu import CRF_KEYS, seeded_snapshot
from test_dense_crf_gpu import reference_stage, tiny_config, write_snapshot
from test_inference_io_gpu import check_label_folders, load_program
from test_train_cli import YAML

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def deterministic_mode():
  """Label maps of two runs of a network are compared bit for bit below (a program against the API, a program against its
  sibling): without the mode the embedding's tap-group sums and the banks' segment sums depend on the arrival order."""
  was = _ffi.set_deterministic(True)
  yield
  _ffi.set_deterministic(was)


# ------------------------------------------------------------------------------------------------------------------
# the kernel
def ingest(case, planes, out=None):
  h, w, ncls, keys, _ = case
  return _ffi.cam_ingest(planes, keys, (h, w), ncls, ref.ALPHA, out=out)


@pytest.mark.parametrize('case', ref.CASES, ids=ref.IDS)
def test_kernel_against_the_fp64_four_tap_expression(case):
  h, w, ncls, keys, _ = case
  host = ref.planes_of(case)
  want = ref.four_tap(host, keys, (h, w), ncls)
  deviation = float(np.abs(ref.reference(host, keys, (h, w), ncls) - want).max())
  # the planes at a 16-byte, non-zero offset inside a larger buffer (where `ImageSource` puts them), the output full of NaN
  buffer = torch.full((host.size + 12,), float('nan'), dtype=torch.float32, device=DEV)
  planes = buffer[4:4 + host.size].view(len(keys), h, w)
  planes.copy_(torch.from_numpy(host.copy()))
  assert planes.data_ptr() % 16 == 0 and planes.data_ptr() != buffer.data_ptr()
  out = torch.full((ncls, h // 8, w // 8), float('nan'), dtype=torch.float32, device=DEV)
  got = ingest(case, planes if keys else None, out)
  assert got is out and _ffi.cam_ingest_path_name(len(keys), h, w, ncls) == 'cam_ingest'
  got = got.cpu().numpy()
  error, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
  print('%s: max |G - Y| = %.3e = %.2f units (reference %.2f units of 2^-24 max |Y|)'
        % (case[:4], error, error / (ref.U * scale), deviation / (ref.U * scale)))
  assert np.isfinite(got).all()
  assert error <= ref.bound(want, deviation)
  absent = [c for c in range(1, ncls) if c - 1 not in keys]
  assert (got[absent] == 0.0).all()                                      # written by the kernel: exactly zero
  if not keys:
    assert (got[0] == 1.0).all()
  # the order the planes are given in does not matter, nor does what the output held
  if len(keys) > 1:
    order = list(range(len(keys)))[::-1]
    again = _ffi.cam_ingest(planes[order].contiguous(), [keys[i] for i in order], (h, w), ncls, ref.ALPHA)
    assert np.array_equal(again.cpu().numpy(), got)


def test_kernel_on_one_class_and_other_powers():
  assert bool((_ffi.cam_ingest(None, [], (16, 24), 1, ref.ALPHA) == 1.0).all())
  case = ref.CASES[5]
  h, w, ncls, keys, _ = case
  host = ref.planes_of(case)
  planes = torch.from_numpy(host.copy()).to(DEV)
  for alpha in (0, 1, 7):
    want = ref.four_tap(host, keys, (h, w), ncls, alpha)
    got = _ffi.cam_ingest(planes, keys, (h, w), ncls, alpha).cpu().numpy()
    assert float(np.abs(got - want).max()) <= 4 * ref.U * float(np.abs(want).max()), alpha
  assert bool((_ffi.cam_ingest(planes, keys, (h, w), ncls, 0)[0] == 1.0).all())


def test_a_refusal_launches_nothing():
  case = ref.CASES[5]
  h, w, ncls, keys, _ = case
  planes = torch.from_numpy(ref.planes_of(case).copy()).to(DEV)
  out = torch.full((ncls, h // 8, w // 8), 9.0, dtype=torch.float32, device=DEV)
  for bad, alpha, status in (([7, 19, 20], 6, -1), ([7, 19, -1], 6, -1), ([7, 19, 7], 6, -1), (keys, -1, -1)):
    with pytest.raises(_ffi.SpmlHipError, match='status %d' % status):
      _ffi.cam_ingest(planes, bad, (h, w), ncls, alpha, out=out)
  with pytest.raises(_ffi.SpmlHipError, match='status -2'):            # more planes than foreground classes
    _ffi.cam_ingest(planes, [0, 1, 2], (h, w), 3, 6, out=torch.full((3, h // 8, w // 8), 9.0, device=DEV))
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.cam_ingest(planes[:, :7].contiguous(), keys, (7, w), ncls, 6)
  torch.cuda.synchronize()
  assert bool((out == 9.0).all())


# ------------------------------------------------------------------------------------------------------------------
# four PNG files of different sizes (one nested), their CAM files, one seeded snapshot for both programs
FILES = [('a.png', (97, 129)), ('b.png', (129, 97)), ('sub/c.png', (129, 110)), ('d.png', (104, 129))]
CRF_OPTIONS = ['--crf', '--crf_iter_max', '2']
CAM_KEYS = {'images', 'images_per_s', 'mIoU', 'pixel_acc', 'scales', 'is_flip', 'cam_dir', 'alpha', 'cam_path', 'walk_steps',
            'snapshot', 'save_dir', 'data_list', 'has_labels'}


@pytest.fixture(scope='module')
def work(tmp_path_factory):
  root = tmp_path_factory.mktemp('cam_lists')
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101')
          .replace('stride:\n    - 97\n    - 97', 'stride:\n    - 64\n    - 64')
          .replace('color_map_path: "misc/colormapvoc.mat"', 'color_map_path: ""'))
  assert 'image_size: 97' in yaml and yaml.count('- 64') == 2 and 'color_map_path: ""' in yaml
  cfg = root / 'config.yaml'
  cfg.write_text(yaml)
  snap = seeded_snapshot(root, 'knn', cfg, 'segsort')
  data, cams = root / 'data', root / 'cams'
  os.makedirs(str(cams))
  rng = np.random.RandomState(91)
  lines, bare, files, cam_files = [], [], [], []
  for index, (name, (h, w)) in enumerate(FILES):
    rgb = np.repeat(np.repeat(rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)), 8, 0), 8, 1)[:h, :w]
    rgb = np.clip(rgb + rng.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
    semantic = np.repeat(np.repeat(rng.choice(np.array([0, 3, 7, 255], np.uint8), (h // 16 + 1, w // 16 + 1)), 16, 0), 16, 1)[:h, :w]
    semantic = np.ascontiguousarray(semantic)
    for sub, array, mode in (('img', rgb, 'RGB'), ('lab', semantic, 'L')):
      path = data / sub / name
      os.makedirs(str(path.parent), exist_ok=True)
      Image.fromarray(array, mode=mode).save(str(path))
    lines.append('img/%s lab/%s lab/%s' % (name, name, name))
    bare.append('img/%s' % name)
    files.append((os.path.basename(name), rgb, semantic))
    # the CAM file of another model: noisy activations of the classes the image carries -- fp64 in one file, as a model's
    # own arrays may be, the keys out of order in another, and one file without entries
    cam = {}
    for c in ((7, 3), (3,), (), (3, 7))[index]:
      cam[c - 1] = (0.15 + 0.7 * (semantic == c) + 0.1 * rng.rand(h, w)).astype(np.float64 if index == 1 else np.float32)
    np.save(str(cams / os.path.basename(name).replace('.png', '.npy')), cam)
    cam_files.append(cam)
  (data / 'val.txt').write_text('\n'.join(lines) + '\n')
  (data / 'bare.txt').write_text('\n'.join(bare) + '\n')
  assert len({hw for _, hw in FILES}) == len(FILES) and any(h > w for _, (h, w) in FILES) and any(w > h for _, (h, w) in FILES)
  assert any(h % 8 for _, (h, w) in FILES) and any(w % 8 for _, (h, w) in FILES)
  return dict(snap=snap, cfg=str(cfg), root=root, data=str(data), list=str(data / 'val.txt'), bare=str(data / 'bare.txt'),
              cams=str(cams), files=files, cam_files=cam_files)


def run(name, work, save, capsys, *extra, data_list=None):
  capsys.readouterr()
  load_program(name).main(['--snapshot_dir', work['snap'], '--cfg_path', work['cfg'], '--save_dir', str(save), '--data_dir',
                           work['data'], '--data_list', data_list or work['list']] + list(extra))
  lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
  assert len(lines) == 1
  return json.loads(lines[0])


@pytest.fixture(scope='module')
def stage(work):
  """What the programs load, loaded again: (config, embedding network, segsort head, crop size, the CRF of CRF_OPTIONS)."""
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args('x', ['--snapshot_dir', work['snap'], '--cfg_path', work['cfg']] + CRF_OPTIONS[1:])
  embedding_model, prediction_model, _ = inference_cli.load_models(config, args, torch.device(DEV), 'segsort')
  return config, embedding_model, prediction_model, inference_cli.geometry(config)[1], inference_cli.CrfStage(config, args).crf


def cam_inputs(work, stage, index):
  """-> (views, image size, planes on the device, keys, the file's bytes on the device) of file `index`, as
  `ListImageSource` hands them to the program."""
  config, _, _, crop_size, _ = stage
  _, rgb, _ = work['files'][index]
  cam = work['cam_files'][index]
  rgb_dev = torch.from_numpy(rgb).to(DEV)
  views = inference.device_views(rgb_dev, [1], True, crop_size, config.network.pixel_means, config.network.pixel_stds)
  keys = list(cam.keys())
  planes = torch.from_numpy(np.stack([np.asarray(v, np.float32) for v in cam.values()])).to(DEV) if keys else None
  return views, rgb.shape[:2], planes, keys, rgb_dev


# ------------------------------------------------------------------------------------------------------------------
# the API
def test_pseudo_labels_cam_on_a_seeded_network(work, stage, monkeypatch):
  config, embedding_model, _, _, crf = stage
  views, (h, w), planes, keys, rgb_dev = cam_inputs(work, stage, 0)
  assert keys == [6, 2] and [v[2] for v in views] == [True, False]
  calls, plain_transition = [], _ffi.affinity_transition

  def recording_transition(units, scale, power):
    calls.append((units, scale, power))
    return plain_transition(units, scale, power)

  monkeypatch.setattr(_ffi, 'affinity_transition', recording_transition)
  out = inference.pseudo_labels_cam(embedding_model, views, (h, w), planes, keys, 21)
  monkeypatch.setattr(_ffi, 'affinity_transition', plain_transition)
  assert set(out) == {'cam', 'cam_rw', 'semantic_prediction', 'cam_path'} and out['cam_path'] == 'cam_ingest'
  assert tuple(out['cam'].shape) == tuple(out['cam_rw'].shape) == (21, h // 8, w // 8)
  assert tuple(out['semantic_prediction'].shape) == (h, w) and out['semantic_prediction'].dtype == torch.int64
  # the class maps meet the kernel's bound against the fp64 expression on the file's own planes
  host = planes.cpu().numpy()
  want = ref.four_tap(host, keys, (h, w), 21)
  deviation = float(np.abs(ref.reference(host, keys, (h, w), 21) - want).max())
  assert float(np.abs(out['cam'].cpu().numpy() - want).max()) <= ref.bound(want, deviation)
  # the walk is the shared one, over the affinity of the two views' unit embeddings, on the function's own class maps
  (units, scale, power), = calls
  assert units.shape[0] == 2 and units.shape[2] == (h // 8) * (w // 8) and (scale, power) == (5.0, 20)
  assert torch.equal(out['cam_rw'], inference._walk(_ffi.affinity_transition(units, 5.0, 20), out['cam'], 6))
  assert torch.equal(out['semantic_prediction'], _ffi.upsample_argmax(out['cam_rw'], h, w))
  assert set(torch.unique(out['semantic_prediction']).tolist()) <= {0, 3, 7}
  # with the CRF: the labels before it are the plain function's, the tail is the shared fused call
  guide = inference.crf_guide(rgb_dev, config.network.pixel_means, config.network.pixel_stds)
  refined = inference.pseudo_labels_cam_crf(embedding_model, views, (h, w), planes, keys, 21, guide, crf)
  assert set(refined) == {'cam', 'cam_rw', 'cam_path', 'semantic_prob', 'semantic_prediction',
                          'semantic_prediction_before_crf', 'crf_path'}
  assert torch.equal(refined['cam'], out['cam']) and tuple(refined['cam_rw'].shape) == tuple(out['cam_rw'].shape)
  assert torch.equal(refined['semantic_prediction_before_crf'], out['semantic_prediction'])
  tail = inference.random_walk_crf_refine(guide, refined['cam_rw'], crf)
  assert torch.equal(refined['semantic_prediction'], tail['semantic_prediction'])
  assert refined['crf_path'].startswith('pairs_mfma_')
  # a file without entries: background everywhere
  empty = inference.pseudo_labels_cam(embedding_model, views, (h, w), None, [], 21)
  assert bool((empty['cam'][0] == 1.0).all()) and not bool(empty['cam'][1:].any())
  assert not bool(empty['semantic_prediction'].any())
  # a key given twice or out of range is refused before the views go through the network
  class Untouched(object):
    def parameters(self):
      return iter(())

    def generate_embeddings(self, *args, **kwargs):
      raise AssertionError('the keys are checked before the network runs')
  for bad in ([6, 6], [6, 20]):
    with pytest.raises(_ffi.SpmlHipError, match='status -1'):
      inference.pseudo_labels_cam(Untouched(), views, (h, w), planes, bad, 21)
  # no CPU path for the planes, no image below 8 x 8
  with pytest.raises(_ffi.SpmlHipError):
    inference.pseudo_labels_cam(embedding_model, views, (h, w), planes.cpu(), keys, 21)
  with pytest.raises(ValueError):
    inference.pseudo_labels_cam(embedding_model, views, (7, w), planes, keys, 21)


# ------------------------------------------------------------------------------------------------------------------
# pseudo_softmaxrw.py --cam_dir
@pytest.mark.parametrize('crf', [False, True], ids=['plain', 'crf'])
def test_cam_walk_on_a_file_list(crf, work, stage, tmp_path, capsys):
  config, embedding_model, _, _, crf_model = stage
  result = run('pseudo_softmaxrw', work, tmp_path / 'out', capsys, '--cam_dir', work['cams'], *(CRF_OPTIONS if crf else []))
  maps = check_label_folders(tmp_path / 'out', work, result)             # sizes, colour == table[gray], the JSON mIoU
  assert set(result) == CAM_KEYS | (CRF_KEYS if crf else set())
  assert result['cam_dir'] == work['cams'] and result['alpha'] == 6 and result['walk_steps'] == 6
  assert result['cam_path'] == 'cam_ingest' and result['scales'] == [1] and result['is_flip'] is True
  assert 'combine' not in result and 'head_path' not in result
  before = []
  for index, got in enumerate(maps):                                     # the written labels are the API's for the same file
    views, hw, planes, keys, rgb_dev = cam_inputs(work, stage, index)
    if crf:
      guide = inference.crf_guide(rgb_dev, config.network.pixel_means, config.network.pixel_stds)
      out = inference.pseudo_labels_cam_crf(embedding_model, views, hw, planes, keys, 21, guide, crf_model)
      before.append(out['semantic_prediction_before_crf'])
    else:
      out = inference.pseudo_labels_cam(embedding_model, views, hw, planes, keys, 21)
    assert np.array_equal(out['semantic_prediction'].cpu().numpy().astype(np.uint8), got), FILES[index][0]
  assert not maps[2].any() and maps[0].any()                             # (c.png's CAM file has no entries)
  if crf:
    assert result['crf_path'].startswith('pairs_mfma_') and 0.0 < result['crf_share'] < 1.0
    differ = sum(int((b.cpu().numpy() != m).sum()) for b, m in zip(before, maps))
    assert result['changed_by_crf'] == round(differ / float(sum(m.size for m in maps)), 4)


def test_cam_walk_needs_no_label_columns_and_names_a_missing_file(work, stage, tmp_path, capsys):
  result = run('pseudo_softmaxrw', work, tmp_path / 'bare', capsys, '--cam_dir', work['cams'], data_list=work['bare'])
  assert result['images'] == len(FILES) and result['has_labels'] is False
  assert result['mIoU'] is None and result['pixel_acc'] is None and set(result) == CAM_KEYS
  for index, (name, (h, w)) in enumerate(FILES):
    name = os.path.basename(name)
    gray = np.array(Image.open(str(tmp_path / 'bare' / 'semantic_gray' / name)))
    views, hw, planes, keys, _ = cam_inputs(work, stage, index)
    out = inference.pseudo_labels_cam(stage[1], views, hw, planes, keys, 21)
    assert gray.shape == (h, w) and np.array_equal(out['semantic_prediction'].cpu().numpy().astype(np.uint8), gray), name
    assert np.array(Image.open(str(tmp_path / 'bare' / 'semantic_color' / name))).shape == (h, w, 3)
  # a directory without the files: the run ends with the first missing file's name
  os.makedirs(str(tmp_path / 'none'))
  with pytest.raises(SystemExit) as info:
    run('pseudo_softmaxrw', work, tmp_path / 'missing', capsys, '--cam_dir', str(tmp_path / 'none'))
  assert str(tmp_path / 'none' / 'a.npy') in str(info.value.code)
  # a plane of another shape
  np.save(str(tmp_path / 'none' / 'a.npy'), {2: np.zeros((129, 97), np.float32)})
  with pytest.raises(SystemExit) as info:
    run('pseudo_softmaxrw', work, tmp_path / 'shape', capsys, '--cam_dir', str(tmp_path / 'none'))
  assert str(tmp_path / 'none' / 'a.npy') in str(info.value.code) and '129 x 97' in str(info.value.code)


def test_cam_walk_on_synthetic_images_reads_the_names_of_pseudo_camrw_crf(tmp_path, capsys, monkeypatch):
  cfg = tiny_config(tmp_path, 21, 'segsort')
  snap = write_snapshot(tmp_path, cfg, 'segsort')
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  config, device, (emb, _, _), (ncls, crop, _, size), _ = reference_stage(cfg, snap, None)
  cams = tmp_path / 'cams'
  os.makedirs(str(cams))
  stand_in = load_program('pseudo_camrw_crf').synthetic_cams
  common = ['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--data_list', 'synthetic', '--cam_dir', str(cams)]
  with pytest.raises(SystemExit) as info:
    load_program('pseudo_softmaxrw').main(common + ['--save_dir', str(tmp_path / 'none')])
  assert str(cams / 'synthetic_0000.npy') in str(info.value.code)
  files = []
  for index in range(2):
    label = inference_cli.synthetic_image(index, size, ncls, device)[1]
    files.append({k: v.cpu().numpy() for k, v in stand_in(label, ncls).items()})
    np.save(str(cams / ('synthetic_%04d.npy' % index)), files[-1])
  capsys.readouterr()
  load_program('pseudo_softmaxrw').main(common + ['--save_dir', str(tmp_path / 'out')])
  result = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
  assert result['images'] == 2 and result['cam_dir'] == str(cams) and result['alpha'] == 6 and result['cam_path'] == 'cam_ingest'
  assert result['mIoU'] is not None and 'data_list' not in result and 'head_path' not in result
  for index, cam in enumerate(files):
    got = np.load(str(tmp_path / 'out' / 'semantic_gray' / ('synthetic_%04d.npy' % index)))
    image = inference_cli.synthetic_image(index, size, ncls, device)[0]
    views = inference.flip_scale_views(image, [1], True, crop)
    planes = torch.from_numpy(np.stack(list(cam.values()))).to(device) if cam else None
    out = inference.pseudo_labels_cam(emb, views, (size, size), planes, list(cam.keys()), ncls)
    assert got.dtype == np.uint8 and np.array_equal(out['semantic_prediction'].cpu().numpy().astype(np.uint8), got)


# ------------------------------------------------------------------------------------------------------------------
# inference_msc.py --pseudo_tags
@pytest.mark.parametrize('crf', [False, True], ids=['plain', 'crf'])
def test_pseudo_tags_equals_the_synthetic_only_program(crf, tmp_path, capsys, monkeypatch):
  cfg = tiny_config(tmp_path, 2, 'segsort')
  snap = write_snapshot(tmp_path, cfg, 'segsort')
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  save = tmp_path / 'results'
  common = ['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic',
            '--crf_iter_max', '2', '--kmeans_num_clusters', '4,4', '--label_divisor', '2048']
  sibling = 'pseudo_inference_crf_msc' if crf else 'pseudo_inference_msc'
  results, maps = [], []
  for prog, extra in ((sibling, []), ('inference_msc', ['--pseudo_tags'] + (['--crf'] if crf else []))):
    capsys.readouterr()
    load_program(prog).main(common + extra)
    results.append(json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]))
    maps.append([np.load(str(save / 'semantic_gray' / ('synthetic_%04d.npy' % i))) for i in range(2)])
    for i in range(2):
      os.remove(str(save / 'semantic_gray' / ('synthetic_%04d.npy' % i)))
  theirs, ours = results
  assert all(a.dtype == np.uint8 and a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(*maps))
  assert ours['views'] == 8 and ours['normalize_path'] == 'hip_tag_normalize'
  assert (CRF_KEYS <= set(ours)) == crf
  for key in set(theirs) - {'images_per_s', 'crf_share'}:                # mIoU, instance_mIoU and the paths among them
    assert ours[key] == theirs[key], key
  assert {'mIoU', 'pixel_acc', 'instance_mIoU', 'normalize_path', 'combine_path'} <= set(theirs)
  # without the option the program is what it was: ten views, no tag fields
  capsys.readouterr()
  load_program('inference_msc').main(common)
  plain = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
  assert plain['views'] == 10 and 'normalize_path' not in plain and 'instance_mIoU' not in plain


def test_pseudo_tags_on_a_file_list(work, stage, tmp_path, capsys):
  config, embedding_model, prediction_model, crop_size, _ = stage
  run('prototype_msc', work, tmp_path / 'bank', capsys)
  bank = ['--semantic_memory_dir', str(tmp_path / 'bank' / 'semantic_prototype')]
  result = run('inference_msc', work, tmp_path / 'out', capsys, '--pseudo_tags', *bank)
  maps = check_label_folders(tmp_path / 'out', work, result)
  assert result['views'] == 8 and result['normalize_path'] == 'hip_tag_normalize' and 'instance_mIoU' not in result
  # the written labels are the API's on the same bytes, with the tags of the file's own label map
  prototypes, prototype_labels = inference_cli.load_bank(bank[1], config, torch.device(DEV))
  stride = inference_cli.geometry(config)[2]
  prog = load_program('inference_msc')
  for (name, rgb, semantic), got in zip(work['files'], maps):
    views = inference.device_views(torch.from_numpy(rgb).to(DEV), prog.PSEUDO_SCALES, True, crop_size,
                                   config.network.pixel_means, config.network.pixel_stds)
    tags = inference.label_tags_from_map(torch.from_numpy(semantic).to(DEV), 21)
    out = inference.pseudo_labels_knn_multiscale(embedding_model, prediction_model, views, rgb.shape[:2], crop_size, stride,
                                                 prototypes, prototype_labels, 21, tags, floor=prog.PSEUDO_FLOOR)
    assert np.array_equal(out['semantic_prediction'].cpu().numpy().astype(np.uint8), got), name
  # a list without label columns has no tags to give
  with pytest.raises(SystemExit) as info:
    run('inference_msc', work, tmp_path / 'bare', capsys, '--pseudo_tags', *bank, data_list=work['bare'])
  assert 'no label columns' in str(info.value.code) and not os.path.exists(str(tmp_path / 'bare'))
