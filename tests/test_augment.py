"""The host side of file-list training (spml_amd/data) and the yardstick of its kernel (tests/augment_ref.py), without
a GPU: the restatement against the reference's own numpy stages (golden n13_augment) and against ATen for what cv2 does
there; the plan; the dataset classes; the sharding; the entry points."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_cases as cases
import augment_ref as ref
from spml_amd import _ffi
from spml_amd.data import batcher, transforms
from spml_amd.data.datasets import (DenseposeClassifierDataset, DenseposeDataset, ListDataset, ListTagClassifierDataset,
                                    ListTagDataset)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24            # unit round-off of fp32


@pytest.fixture(scope='module')
def gold():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'n13_augment.npz'))


# ------------------------------------------------------------------------------------------------------------------
# the restatement against the reference's own lines
@pytest.mark.parametrize('ci', range(4))
def test_restatement_equals_the_reference_numpy_stages(gold, ci):
  g = lambda k: gold['c%d_%s' % (ci, k)]
  image, label, crop = g('image'), g('label'), tuple(int(v) for v in g('crop'))
  mean = tuple(float(v) for v in gold['mean'])
  m_image, m_label = ref.mirror(image, label)
  assert np.array_equal(m_image, g('mirror_image')) and np.array_equal(m_label, g('mirror_label'))
  p_image, p_label = ref.resize_with_pad(image, crop, mean), ref.resize_with_pad(label, crop, 255)
  assert p_image.dtype == np.float32 and np.array_equal(p_image, g('pad_image'))
  assert np.array_equal(p_label, g('pad_label'))
  start_w, start_h, end_w, end_h = (int(v) for v in g('bbox'))
  assert (end_h - start_h, end_w - start_w) == crop
  c_image = ref.crop(p_image, start_h, start_w, crop)
  assert np.array_equal(c_image, g('crop_image'))
  assert np.array_equal(ref.crop(p_label, start_h, start_w, crop), g('crop_label'))
  gray = ref.grayscale(c_image)
  assert gray.dtype == np.float32 and np.array_equal(gray, g('gray'))
  assert np.array_equal(ref.tags(label[..., 0]), g('tags').astype(np.int64))


def test_blur_weights_equal_the_reference_lines(gold):
  for sigma, want in zip(gold['sigmas'], gold['weights']):
    assert np.array_equal(ref.blur_weights(float(sigma)), want)
    assert np.array_equal(transforms.blur_weights(float(sigma)), want)


def test_golden_covers_every_padding_case(gold):
  kinds = set()
  for ci in range(4):
    h, w = gold['c%d_image' % ci].shape[:2]
    ch, cw = gold['c%d_crop' % ci]
    kinds.add((int(np.sign(h - ch)), int(np.sign(w - cw))))
    sw, sh = gold['c%d_bbox' % ci][:2]
    assert 0 <= sh <= max(h, ch) - ch and 0 <= sw <= max(w, cw) - cw
  assert kinds == {(-1, -1), (1, -1), (1, 1), (0, 0)}
  assert any(gold['c%d_bbox' % ci][0] > 0 or gold['c%d_bbox' % ci][1] > 0 for ci in range(4))


# ------------------------------------------------------------------------------------------------------------------
# ... and against ATen on the CPU for the two resize modes and the blur
RESIZES = [((20, 27), (40, 54)), ((58, 74), (29, 37)), ((20, 27), (10, 13)), ((41, 23), (53, 29)),
           ((70, 90), (105, 135)), ((28, 35), (28, 35))]      # the sizes of tests/augment_cases.py: up, down, none


@pytest.mark.parametrize('src,dst', RESIZES)
def test_nearest_indices_equal_aten(src, dst):
  """`mode='nearest'` is floor(dst_index * scale), scale = in / out in fp32; cv2's INTER_NEAREST the same in double.
  At these sizes the two floors agree for every index -- asserted, not assumed."""
  planes = torch.arange(src[0] * src[1], dtype=torch.float32).view(1, 1, *src)
  got = F.interpolate(planes, size=dst, mode='nearest')[0, 0].long().numpy()
  want = ref.resize_nearest(np.arange(src[0] * src[1]).reshape(src), *dst)
  assert np.array_equal(got, want)


@pytest.mark.parametrize('src,dst', RESIZES)
def test_bilinear_within_fp32_of_aten(src, dst):
  """`mode='bilinear', align_corners=False` forms the same taps (scale * (dst + 0.5) - 0.5, negative coordinates
  clamped to 0, the last tap clamped) in fp32.  Its coordinate is off by at most 3 roundings of a number below the
  source side, so each axis's fraction by 3 u side (0 where the scale is a power of two: every coordinate is exact);
  the value, continuous in the fractions with slope at most 1 on data in [0, 1], by the sum of the two, plus 7 roundings
  of the interpolation itself."""
  rng = np.random.RandomState(7)
  image = rng.randint(0, 256, src + (3,)).astype(np.float64) / 255.0
  want = ref.resize_linear(image, *dst)
  got = F.interpolate(torch.from_numpy(image.transpose(2, 0, 1)[None]).float(), size=dst, mode='bilinear',
                      align_corners=False)[0].permute(1, 2, 0).double().numpy()
  exact = all(float(np.log2(s / d)).is_integer() for s, d in zip(src, dst))
  bound = 8 * U if exact else (3 * U * (src[0] + src[1]) + 8 * U)      # (+ 1 u: the fp32 cast of the fp64 input)
  dev = float(np.abs(got - want).max())
  print('bilinear %r -> %r: max |ATen fp32 - restatement fp64| = %.3e (bound %.3e)' % (src, dst, dev, bound))
  assert dev <= bound


@pytest.mark.parametrize('sigma', [0.1, 5.0])
@pytest.mark.parametrize('hw', [(29, 37), (5, 6)])
def test_blur_within_fp32_of_aten(sigma, hw):
  """conv2d over a reflect-padded image is the correlation with reflect-101 borders; 25 products and 24 additions in
  fp32 on weights that sum to 1 and data in [0, 1]: at most 26 u (+ 1 u for the fp32 cast of the input)."""
  rng = np.random.RandomState(11)
  image = rng.randint(0, 256, hw + (3,)).astype(np.float64) / 255.0
  weight = cases.weights(sigma)
  want = ref.filter2d(image, weight.astype(np.float64).reshape(5, 5))
  x = F.pad(torch.from_numpy(image.transpose(2, 0, 1)[None]).float(), (2, 2, 2, 2), mode='reflect')
  k = torch.from_numpy(weight).view(1, 1, 5, 5).expand(3, 1, 5, 5).contiguous()
  got = F.conv2d(x, k, groups=3)[0].permute(1, 2, 0).double().numpy()
  dev = float(np.abs(got - want).max())
  print('blur sigma %.1f on %r: max |ATen fp32 - restatement fp64| = %.3e (bound %.3e)' % (sigma, hw, dev, 27 * U))
  assert dev <= 27 * U


def test_restatement_of_a_whole_sample_composes_its_stages():
  """augment_one against the stages applied by hand, and the padding's labels and pixels."""
  c = cases.case('A', 0)
  rgb, sem, inst = c['samples'][1]
  p = c['plans'][1]                                       # 41 x 23 at 1.3, mirrored, grey
  image = ref.resize_linear(rgb[:, ::-1].astype(np.float64) / 255.0, p['new_h'], p['new_w'])
  image = ref.crop(ref.resize_with_pad(image, cases.CROP, cases.MEAN.astype(np.float64)), 11, 0, cases.CROP)
  image = (ref.grayscale(image) - cases.MEAN) / cases.STD
  assert np.array_equal(c['image'][1], image.transpose(2, 0, 1))
  assert np.all(c['sem'][1][:, p['new_w']:] == 255) and np.all(c['inst'][1][:, p['new_w']:] == 255)
  want = cases.DENSEPOSE[ref.resize_nearest(sem[:, ::-1], p['new_h'], p['new_w'])][11:11 + 29]
  assert np.array_equal(c['sem'][1][:, :p['new_w']], want)
  for name in cases.BATCHES:
    got = cases.case(name, 0)
    assert got['image'].shape == (len(got['plans']), 3) + got['crop'] and got['tags'].shape == (len(got['plans']), 256)
    assert all(got['tags'][:, v].all() for v in (0, 14, 254, 255))
    assert np.abs(got['image']).max() < 3.0


# ------------------------------------------------------------------------------------------------------------------
# the plan
KW = dict(size=(29, 37), random_mirror=True, random_scale=True, random_crop=True, scale_range=(0.5, 2.0),
          random_grayscale=True, random_blur=True)


def _same(a, b):
  return all(np.array_equal(a[k], b[k]) for k in a)


def test_plan_is_a_function_of_seed_epoch_index():
  one = transforms.plan_training(transforms.sample_rng(235, 3, 17), 40, 50, **KW)
  assert _same(one, transforms.plan_training(transforms.sample_rng(235, 3, 17), 40, 50, **KW))
  for other in ((236, 3, 17), (235, 4, 17), (235, 3, 18)):
    assert not _same(one, transforms.plan_training(transforms.sample_rng(*other), 40, 50, **KW))
  np.random.seed(1)                                     # global state plays no part
  assert _same(one, transforms.plan_training(transforms.sample_rng(235, 3, 17), 40, 50, **KW))


def test_every_draw_stays_inside_its_range():
  seen = {'flip': set(), 'gray': set(), 'blur': set()}
  ratios_h, n_gray, n_blur, n = [], 0, 0, 3000
  for seed in range(n):
    p = transforms.plan_training(transforms.sample_rng(seed, 0, 0), 40, 50, **KW)
    assert int(0.5 * 40) <= p['new_h'] <= int(2.0 * 40) and int(0.5 * 50) <= p['new_w'] <= int(2.0 * 50)
    assert 0 <= p['start_h'] <= max(p['new_h'], 29) - 29 and 0 <= p['start_w'] <= max(p['new_w'], 37) - 37
    if p['new_h'] <= 29:
      assert p['start_h'] == 0
    if p['new_w'] <= 37:
      assert p['start_w'] == 0
    for k in seen:
      seen[k].add(p[k])
    ratios_h.append(p['new_h'])
    n_gray, n_blur = n_gray + p['gray'], n_blur + p['blur']
    if p['blur']:
      w = p['weights'].astype(np.float64).reshape(5, 5)
      assert abs(w.sum() - 1) < 1e-6 and w[2, 2] == w.max() and np.allclose(w, w.T) and (w >= 0).all()
      # sigma in [0.1, 5]: the centre weight lies between the two extremes'
      assert ref.blur_weights(5.0)[2, 2] - 1e-6 <= w[2, 2] <= 1.0
    else:
      assert not p['weights'].any()
  assert all(v == {False, True} for v in seen.values())
  assert min(ratios_h) == 20 and max(ratios_h) >= 79
  assert 0.25 < n_gray / n < 0.35 and 0.45 < n_blur / n < 0.55      # 0.3 and 0.5 (a few sigma of 3000 draws)
  # padded == S: the start is 0; no scaling, no mirror: nothing is drawn for them
  for seed in range(200):
    p = transforms.plan_training(transforms.sample_rng(seed, 0, 0), 29, 37, size=(29, 37), random_mirror=False,
                                 random_scale=False, random_crop=True)
    assert (p['new_h'], p['new_w'], p['start_h'], p['start_w'], p['flip'], p['gray'], p['blur']) == (29, 37, 0, 0, False, False, False)


def test_draw_order_is_the_references():
  """mirror, ratio, start_h, start_w, grayscale, blur, sigma -- one uniform each, from one stream."""
  rng = transforms.sample_rng(5, 6, 7)
  u = [rng.uniform(0, 1.0)]
  ratio = rng.uniform(0.5, 2.0)
  new_h, new_w = int(ratio * 40), int(ratio * 50)
  sh = int(np.floor(rng.uniform(0, max(new_h, 29) - 29)))
  sw = int(np.floor(rng.uniform(0, max(new_w, 37) - 37)))
  gray = rng.uniform(0, 1.0) < 0.3
  blur = rng.uniform(0, 1.0) < 0.5
  p = transforms.plan_training(transforms.sample_rng(5, 6, 7), 40, 50, **KW)
  assert (p['flip'], p['new_h'], p['new_w'], p['start_h'], p['start_w'], p['gray'], p['blur']) == \
      (u[0] >= 0.5, new_h, new_w, sh, sw, gray, blur)
  if blur:
    assert np.array_equal(p['weights'], ref.blur_weights(rng.uniform(0.1, 5)).reshape(25).astype(np.float32))


def test_a_side_without_a_pixel_is_refused_by_name():
  with pytest.raises(ValueError, match='tiny.png'):
    transforms.plan_training(transforms.sample_rng(0, 0, 0), 1, 9, size=(5, 5), random_mirror=False, random_scale=True,
                             random_crop=True, scale_range=(0.5, 0.5), name='somewhere/tiny.png')
  with pytest.raises(ValueError, match='random_crop'):
    transforms.plan_training(transforms.sample_rng(0, 0, 0), 9, 9, size=(5, 5), random_mirror=False, random_scale=False,
                             random_crop=False)


# ------------------------------------------------------------------------------------------------------------------
# the dataset classes
def write_list(tmp_path, n=8, three=True):
  from PIL import Image
  rng = np.random.RandomState(3)
  lines, arrays = [], []
  (tmp_path / 'img').mkdir(exist_ok=True)
  for k in range(n):
    h, w = 11 + 3 * k, 17 + 2 * (k % 3)
    rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    sem = rng.choice(np.array([0, 2, 3, 14, 254, 255], np.uint8), (h, w))
    inst = rng.randint(0, 7, (h, w)).astype(np.uint8)
    Image.fromarray(rgb).save(str(tmp_path / 'img' / ('%d.png' % k)))
    Image.fromarray(sem).save(str(tmp_path / 'img' / ('%d_sem.png' % k)))
    Image.fromarray(inst).save(str(tmp_path / 'img' / ('%d_inst.png' % k)))
    lines.append('img/%d.png img/%d_sem.png img/%d_inst.png' % (k, k, k) if three else 'img/%d.png' % k)
    arrays.append((rgb, sem, inst))
  path = tmp_path / ('train.txt' if three else 'images.txt')
  path.write_text('\n'.join(lines) + '\n')
  return str(path), arrays


def test_list_parsing_and_decoding(tmp_path):
  path, arrays = write_list(tmp_path)
  ds = ListTagDataset(str(tmp_path), path, size=(29, 37), random_crop=True, random_scale=True, random_mirror=True,
                      training=True)
  assert len(ds) == 8
  assert ds.image_paths[3] == os.path.join(str(tmp_path), 'img/3.png')
  assert ds.semantic_label_paths[3].endswith('img/3_sem.png') and ds.instance_label_paths[3].endswith('img/3_inst.png')
  image, sem, inst, plan, idx = ds[5]
  assert idx == 5 and image.dtype == sem.dtype == inst.dtype == np.uint8
  assert np.array_equal(image, arrays[5][0]) and np.array_equal(sem, arrays[5][1]) and np.array_equal(inst, arrays[5][2])
  assert (plan['h'], plan['w']) == image.shape[:2]
  assert _same(plan, ds.get(5, 0)[3]) and not _same(plan, ds.get(5, 1)[3])
  only, _ = write_list(tmp_path, three=False)
  images = ListDataset(str(tmp_path), only, size=(29, 37), random_crop=True, training=True)
  assert len(images) == 8 and images.semantic_label_paths == [] and images.instance_label_paths == []
  assert images[2][1] is None and images[2][2] is None
  with pytest.raises(ValueError, match='three-column'):
    batcher.pack([images.get(0)], np.zeros(1 << 16, np.uint8))
  ds.eval()
  with pytest.raises(NotImplementedError):
    ds[0]


def test_the_five_classes(tmp_path):
  path, _ = write_list(tmp_path, n=2)
  args = dict(data_dir=str(tmp_path), data_list=path, img_mean=(0.1, 0.2, 0.3), img_std=(1, 2, 3), size=(29, 37),
              random_crop=True, random_scale=True, random_mirror=True, training=True)
  want = {ListDataset: ((0.5, 1.5), False, False), ListTagDataset: ((0.5, 1.5), True, False),
          ListTagClassifierDataset: ((0.5, 2.0), True, True), DenseposeDataset: ((0.5, 1.5), False, False),
          DenseposeClassifierDataset: ((0.5, 2.0), False, True)}
  for cls, (scale, tagged, classifier) in want.items():
    ds = cls(random_grayscale=True, random_blur=True, **args) if classifier else cls(**args)
    assert ds.scale_range == scale and ds.with_tags == tagged
    assert (ds.random_grayscale, ds.random_blur) == (classifier, classifier)
    remap = cases.DENSEPOSE if 'Densepose' in cls.__name__ else cases.IDENTITY
    assert ds.label_remap.dtype == np.uint8 and np.array_equal(ds.label_remap, remap)
    sides, flags = set(), set()
    for epoch in range(300):
      p = ds.plan(0, 100, 100, epoch)
      sides.add(p['new_h'])
      flags.add((p['gray'], p['blur']))
    assert min(sides) >= int(scale[0] * 100) and max(sides) <= int(scale[1] * 100)
    assert (max(sides) > 150) == (scale[1] == 2.0)
    assert flags == ({(False, False), (False, True), (True, False), (True, True)} if classifier else {(False, False)})
    if classifier:
      off = cls(**args)                                   # the two switches default to off, as in the reference
      assert (off.random_grayscale, off.random_blur) == (False, False)
  ds = ListTagDataset(**args)
  ds.scale_range = (0.5, 0.5)
  with pytest.raises(ValueError, match='0.png'):
    ds.plan(0, 1, 40)


def test_rank_sharding_partitions_the_permutation_and_wraps():
  n, b, world = 10, 3, 2
  per_rank = {r: [batcher.rank_positions(9, n, b, it, r, world) for it in range(4)] for r in range(world)}
  stream = []                                             # positions 0, 1, 2, ... of the endless sequence
  for it in range(4):
    for i in range(b):
      for r in range(world):
        stream.append(per_rank[r][it][i])
  assert len(stream) == 24
  for epoch in (0, 1):
    got = [idx for e, idx in stream if e == epoch]
    assert got == list(batcher.epoch_permutation(9, epoch, n))[:len(got)]
  assert sorted(idx for e, idx in stream if e == 0) == list(range(n))          # a partition of the epoch
  assert [e for e, _ in stream] == [0] * 10 + [1] * 10 + [2] * 4               # wraps: every batch is full
  assert all(len(batch) == b for r in per_rank for batch in per_rank[r])
  assert not np.array_equal(batcher.epoch_permutation(9, 0, n), batcher.epoch_permutation(9, 1, n))
  assert not np.array_equal(batcher.epoch_permutation(9, 0, n), batcher.epoch_permutation(10, 0, n))
  assert batcher.rank_positions(9, n, b, 2, 1, world) == per_rank[1][2]       # a resumed run continues the sequence
  assert batcher.rank_positions(9, n, 4, 0, 0, 1, shuffle=False) == [(0, 0), (0, 1), (0, 2), (0, 3)]


def test_pack_lays_the_batch_out_behind_its_records(tmp_path):
  c = cases.case('A', 0)
  buf, records = cases.packed(c)
  assert records.dtype == _ffi.AUGMENT_PARAMS and records.shape == (5,) and _ffi.AUGMENT_PARAMS.itemsize == 168
  for k, ((rgb, sem, inst), p) in enumerate(zip(c['samples'], c['plans'])):
    r = records[k]
    px = p['h'] * p['w']
    assert np.array_equal(buf[r['image_off']:r['image_off'] + 3 * px].reshape(rgb.shape), rgb)
    assert np.array_equal(buf[r['sem_off']:r['sem_off'] + px].reshape(sem.shape), sem)
    assert np.array_equal(buf[r['inst_off']:r['inst_off'] + px].reshape(inst.shape), inst)
    assert r['image_off'] >= 5 * 168 and r['image_off'] % 16 == 0
    assert (r['h'], r['w'], r['new_h'], r['new_w'], r['start_h'], r['start_w']) == \
        (p['h'], p['w'], p['new_h'], p['new_w'], p['start_h'], p['start_w'])
    assert (bool(r['flip']), bool(r['gray']), bool(r['blur'])) == (p['flip'], p['gray'], p['blur'])
    assert np.array_equal(r['weights'], p['weights'])
  assert batcher.MAX_THREADS == 16


# ------------------------------------------------------------------------------------------------------------------
# the library's host side
def test_path_name_of_a_record():
  c = cases.case('A', 0)
  buf, records = cases.packed(c)
  names = [_ffi.augment_path_name(records[k:k + 1], buf.size, cases.CROP) for k in range(5)]
  assert names == ['plain', 'plain', 'blur', 'blur', 'blur']

  def changed(k, **fields):
    r = records[k:k + 1].copy()
    for name, v in fields.items():
      r[name] = v
    return r
  bad = [changed(0, new_h=0), changed(0, new_w=0), changed(0, start_h=1), changed(0, start_w=-1),
         changed(2, start_h=77), changed(2, start_w=99), changed(1, h=0), changed(1, new_w=16385)]
  for r in bad:
    assert _ffi.augment_path_name(r, buf.size, cases.CROP) == 'unsupported'
  last = records[4:5]
  assert _ffi.augment_path_name(last, buf.size, cases.CROP) == 'blur'
  assert _ffi.augment_path_name(last, int(last['inst_off'][0]) + 28 * 35, cases.CROP) == 'blur'
  assert _ffi.augment_path_name(last, int(last['inst_off'][0]) + 28 * 35 - 1, cases.CROP) == 'unsupported'
  assert _ffi.augment_path_name(changed(4, image_off=-1), buf.size, cases.CROP) == 'unsupported'
  assert _ffi.augment_path_name(changed(4, sem_off=1 << 40), buf.size, cases.CROP) == 'unsupported'
  assert _ffi.augment_path_name(changed(2, start_h=76, start_w=98), buf.size, cases.CROP) == 'blur'
  assert _ffi.augment_path_name(records[2:3], buf.size, (2, 37)) == 'unsupported'       # blur on a crop side below 3
  assert _ffi.augment_path_name(records[0:1], buf.size, (2, 37)) == 'plain'
  assert _ffi.augment_path_name(records[0:1], buf.size, (0, 37)) == 'unsupported'
  assert _ffi.lib().spml_augment_params_bytes() == _ffi.AUGMENT_PARAMS.itemsize
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  for name in ('spml_augment_batch_u8', 'spml_augment_tags_u8', 'spml_augment_path_name', 'spml_augment_params_bytes'):
    assert name in hdr and name in _ffi.EXPORTS


def test_no_cpu_fallback():
  from spml_amd import ops
  c = cases.case('A', 0)
  buf, records = cases.packed(c)
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  with pytest.raises(_ffi.SpmlHipError):
    ops.augment_batch(t(buf), records, t(cases.MEAN), t(cases.STD), t(cases.DENSEPOSE), cases.CROP)
  with pytest.raises(_ffi.SpmlHipError):
    ops.augment_tags(t(buf), records)


# ------------------------------------------------------------------------------------------------------------------
# the programs
def load_program(name):
  spec = importlib.util.spec_from_file_location('spml_' + name, os.path.join(ROOT, 'pyscripts', 'train', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


PROGRAMS = ('train', 'train_classifier', 'train_densepose', 'train_densepose_classifier')


@pytest.mark.parametrize('name', PROGRAMS)
def test_programs_stop_without_a_gpu_and_take_synthetic(tmp_path, name):
  from test_train_cli import YAML
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML)
  mod = load_program(name)
  if not torch.cuda.is_available():
    for extra in ([], ['--data_list', 'synthetic'], ['--data_dir', str(tmp_path), '--data_list', str(tmp_path / 'l.txt')]):
      with pytest.raises(SystemExit, match='MI355X'):
        mod.main(['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg)] + extra)
  doc = mod.__doc__
  assert 'outside' not in doc and '--data_list' in doc


def test_data_list_resolution(tmp_path):
  config = types.SimpleNamespace(dataset=types.SimpleNamespace(data_dir='', train_data_list=''))
  args = lambda d, l: types.SimpleNamespace(data_dir=d, data_list=l)
  assert batcher.resolve_data_list(args(None, None), config) is None
  assert batcher.resolve_data_list(args('x', 'synthetic'), config) is None
  missing = str(tmp_path / 'nowhere.txt')
  with pytest.raises(SystemExit, match='nowhere.txt'):
    batcher.resolve_data_list(args('x', missing), config)
  path, _ = write_list(tmp_path, n=1)
  assert batcher.resolve_data_list(args('x', path), config) == ('x', path)
  config.dataset.data_dir, config.dataset.train_data_list = 'from_config', path
  assert batcher.resolve_data_list(args(None, None), config) == ('from_config', path)
  assert batcher.resolve_data_list(args(None, 'synthetic'), config) is None
