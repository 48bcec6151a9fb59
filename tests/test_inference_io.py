"""Inference from image lists, as far as it runs without a GPU: the view plan against the reference's own functions
(tests/golden/n14_inference_io.npz), the colour table, the restatement (tests/inference_io_ref.py) against ATen on the
CPU, `ListDataset.read`, the refusals of the programs, the naming of `ImageSource` and the record refusals of
csrc/inference_io.hip through its host-only path names."""
import importlib.util
import os
import types

import numpy as np
import PIL.Image as Image
import pytest
import torch
import torch.nn.functional as F

import augment_ref
import inference_io_cases as cases
import inference_io_ref as ref
from spml_amd import _ffi, inference, inference_cli
from spml_amd.data import transforms
from spml_amd.data.datasets import ListDataset
from spml_amd.utils.general import vis
from test_train_cli import ROOT, YAML

U = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'n14_inference_io.npz')


@pytest.fixture(scope='module')
def gold():
  return np.load(GOLD)


# ------------------------------------------------------------------------------------------------------------------
# the plan against the reference's own functions
def test_plan_views_sizes_equal_the_references_requests(gold):
  for (h, w, size), (new_h, new_w) in zip(gold['interp_cases'], gold['interp_sizes']):
    if new_h < 1 or new_w < 1:
      with pytest.raises(ValueError, match='some/file.jpg'):
        transforms.plan_views(h, w, [1], False, (9, 9), image_size=size, name='some/file.jpg')
      continue
    view, = transforms.plan_views(h, w, [1], False, (9, 9), image_size=size)
    assert (view['new_h'], view['new_w']) == (new_h, new_w), (h, w, size)
  assert [tuple(r) for r in gold['interp_cases']][0] == (23, 43, 23) and tuple(gold['interp_sizes'][0]) == (12, 22)
  for (h, w, scale), (new_h, new_w) in zip(gold['scale_cases'], gold['scale_sizes']):
    view, = transforms.plan_views(int(h), int(w), [float(scale)], False, (9, 9))
    assert (view['new_h'], view['new_w']) == (new_h, new_w), (h, w, scale)
  with pytest.raises(ValueError):
    transforms.plan_views(375, 500, [0.5, 1], False, (9, 9), image_size=320)
  with pytest.raises(ValueError, match='a.jpg'):
    transforms.plan_views(1, 9, [0.5], False, (9, 9), name='a.jpg')


def test_plan_views_differs_from_rounding_where_the_reference_truncates(gold):
  """`flip_scale_views` sizes with round(h * scale): 375 x 1.25 -> 469 there, 468 in the reference."""
  differ = 0
  for (h, w, scale), (new_h, new_w) in zip(gold['scale_cases'], gold['scale_sizes']):
    rounded = (max(int(round(h * scale)), 1), max(int(round(w * scale)), 1))
    differ += rounded != (new_h, new_w)
    if (h, w, scale) == (375, 500, 1.25):
      assert rounded == (469, 625) and (new_h, new_w) == (468, 625)
      image = torch.zeros(1, 3, 375, 500)
      assert inference.flip_scale_views(image, [1.25], False, (9, 9))[0][1] == (469, 625)
      assert transforms.plan_views(375, 500, [1.25], False, (9, 9))[0]['new_h'] == 468
  assert differ >= 3


@pytest.mark.parametrize('tag', ['msc', 'bank', 'small'])
def test_plan_views_order_flags_and_padding_equal_create_image_pyramid(gold, tag):
  h, w = (int(v) for v in gold[tag + '_hw'])
  crop = (33, 33) if tag != 'msc' else (513, 513)
  plan = transforms.plan_views(h, w, [float(s) for s in gold[tag + '_scales']], bool(gold[tag + '_is_flip']), crop)
  assert [(v['new_h'], v['new_w']) for v in plan] == [tuple(s) for s in gold[tag + '_sizes']]
  assert [(v['new_h'], v['new_w']) for v in plan] == [tuple(s) for s in gold[tag + '_label_sizes']]
  assert [v['flip'] for v in plan] == [bool(f) for f in gold[tag + '_flips']]
  # the recording resize wrote every pixel's column index: a flipped view starts with the RESIZED array's last column
  assert [v['new_w'] - 1 if v['flip'] else 0 for v in plan] == list(gold[tag + '_first_column'])
  # (the label arrays are uint8: their column index wraps at 256)
  assert [c % 256 for c in gold[tag + '_first_column']] == list(gold[tag + '_first_label_column'])
  image_at = label_at = 0
  for v in plan:
    assert (v['pad_h'], v['pad_w']) == (max(v['new_h'], crop[0]), max(v['new_w'], crop[1]))
    assert v['image_off'] % 16 == 0 and v['label_off'] % 16 == 0
    assert v['image_off'] >= image_at and v['label_off'] >= label_at               # packed in order, no overlap
    image_at, label_at = v['image_off'] + 12 * v['pad_h'] * v['pad_w'], v['label_off'] + 8 * v['new_h'] * v['new_w']
  assert transforms.view_buffer_bytes(plan) == (image_at, label_at)
  if tag == 'msc':                                  # the ten views of a 375 x 500 file: 36.8 MB of fp32
    assert len(plan) == 10 and round(image_at / 1e6, 1) == 36.8


def test_resize_with_pad_of_the_restatement_equals_the_references(gold):
  for ci in range(4):
    got = augment_ref.resize_with_pad(gold['pad%d_image' % ci], tuple(gold['pad%d_crop' % ci]), 0)
    assert np.array_equal(got, gold['pad%d_out' % ci])


def test_voc_color_map_equals_the_references_table(gold):
  table = vis.voc_color_map()
  assert table.dtype == np.uint8 and table.shape == (256, 3) and np.array_equal(table, gold['color_map'])
  assert [tuple(r) for r in table[:3]] == [(0, 0, 0), (128, 0, 0), (0, 128, 0)] and tuple(table[255]) == (224, 224, 192)


def test_load_color_map_takes_the_key_from_the_file_name(tmp_path):
  scipy_io = pytest.importorskip('scipy.io')
  table = np.linspace(0, 1, 15).reshape(5, 3)
  path = str(tmp_path / 'colormapvoc.mat')
  scipy_io.savemat(path, {'colormapvoc': table, 'other': np.zeros((2, 3))})
  got = vis.load_color_map(path)
  assert got.dtype == np.uint8 and np.array_equal(got, (table * 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------------
# the restatement's two resize modes against ATen on the CPU, at the sizes of the GPU tests
RESIZES = [(src, dst) for src, _, _, _, sizes in cases.VIEW_CASES for dst in sizes] + \
          [(valid, out) for _, valid, out in cases.EXPORT_CASES]


@pytest.mark.parametrize('src,dst', RESIZES)
def test_nearest_indices_equal_aten(src, dst):
  """`mode='nearest'` is floor(dst_index * scale), scale = in / out in fp32; cv2's INTER_NEAREST the same in double.
  At these sizes the two floors agree for every index -- asserted, not assumed."""
  planes = torch.arange(src[0] * src[1], dtype=torch.float32).view(1, 1, *src)
  got = F.interpolate(planes, size=dst, mode='nearest')[0, 0].long().numpy()
  assert np.array_equal(got, augment_ref.resize_nearest(np.arange(src[0] * src[1]).reshape(src), *dst))


@pytest.mark.parametrize('src,dst', RESIZES[:7])
def test_bilinear_within_fp32_of_aten(src, dst):
  """As tests/test_augment.py holds `resize_linear` to ATen, on the NORMALISED image: ATen's fp32 coordinate is off by
  at most 3 roundings of a number below the source side, so each axis's fraction by 3 u side; the value is continuous in
  the fractions with slope at most the data's span (4.8: (0 - 0.485) / 0.229 .. (1 - 0.406) / 0.225), plus 8 roundings of
  the interpolation and the input cast on values below 2.7."""
  rgb, _ = cases.source(src)
  image = ref.normalise(rgb, cases.MEAN, cases.STD)
  want = augment_ref.resize_linear(image, *dst)
  got = F.interpolate(torch.from_numpy(image.transpose(2, 0, 1)[None]).float(), size=dst, mode='bilinear',
                      align_corners=False)[0].permute(1, 2, 0).double().numpy()
  bound = 4.8 * 3 * U * (src[0] + src[1]) + 2.7 * 8 * U
  dev = float(np.abs(got - want).max())
  print('bilinear %r -> %r: max |ATen fp32 - restatement fp64| = %.3e (bound %.3e)' % (src, dst, dev, bound))
  assert dev <= bound
  if src == dst:
    assert np.array_equal(want, image)


def test_restatement_of_one_view_mirrors_the_resized_image_and_pads_with_zero():
  rgb, semantic = cases.source((23, 37))
  plain, flipped = ({'new_h': 11, 'new_w': 18, 'pad_h': 33, 'pad_w': 33, 'flip': f} for f in (0, 1))
  (image, label), (f_image, f_label) = ref.one_view(rgb, semantic, plain, cases.MEAN, cases.STD), \
      ref.one_view(rgb, semantic, flipped, cases.MEAN, cases.STD)
  assert image.shape == (3, 33, 33) and label.shape == (11, 18) and label.dtype == np.int64
  assert np.array_equal(f_image[:, :11, :18], image[:, :11, :18][:, :, ::-1]) and np.array_equal(f_label, label[:, ::-1])
  assert not image[:, 11:, :].any() and not image[:, :, 18:].any() and image[:, :11, :18].all()
  # a mirror of the RESIZED image is not a resize of the mirrored source where the scale is not exact
  other = augment_ref.resize_nearest(semantic[:, ::-1], 11, 18)
  assert not np.array_equal(other, f_label)


# ------------------------------------------------------------------------------------------------------------------
# the dataset, the programs' refusals, the names
def write_files(root, names, hw=(13, 17), labels=True, seed=0):
  """PNG / JPEG images (+ label PNGs) under `root`; -> (list path, per image (rgb, semantic))."""
  rng = np.random.RandomState(seed)
  lines, arrays = [], []
  for k, name in enumerate(names):
    h, w = hw[0] + k, hw[1] + 2 * k
    rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    semantic = rng.choice(np.array([0, 1, 2, 255], np.uint8), (h, w))
    os.makedirs(os.path.dirname(os.path.join(root, 'img', name)), exist_ok=True)
    os.makedirs(os.path.dirname(os.path.join(root, 'lab', name)), exist_ok=True)
    Image.fromarray(rgb, mode='RGB').save(os.path.join(root, 'img', name))
    stem = os.path.splitext(name)[0] + '.png'
    if labels:
      Image.fromarray(semantic, mode='L').save(os.path.join(root, 'lab', stem))
      lines.append('img/%s lab/%s lab/%s' % (name, stem, stem))
    else:
      lines.append('img/%s' % name)
    arrays.append((rgb, semantic))
  path = os.path.join(root, 'list.txt')
  with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
  return path, arrays


def test_list_dataset_read_in_both_modes(tmp_path):
  path, arrays = write_files(str(tmp_path), ['a.png', 'b.png'])
  ds = ListDataset(str(tmp_path), path, size=(9, 9), random_crop=True, training=True)
  for mode in (ds.train, ds.eval):
    mode()
    for k, (rgb, semantic) in enumerate(arrays):
      got = ds.read(k)
      assert got[0].dtype == np.uint8 and np.array_equal(got[0], rgb)
      assert np.array_equal(got[1], semantic) and np.array_equal(got[2], semantic)
  ds.eval()
  with pytest.raises(NotImplementedError):
    ds[0]
  bare, _ = write_files(str(tmp_path / 'bare'), ['a.png'], labels=False)
  rgb, semantic, instance = ListDataset(str(tmp_path / 'bare'), bare).read(0)
  assert rgb.shape == (13, 17, 3) and semantic is None and instance is None


def load_program(name):
  spec = importlib.util.spec_from_file_location('spml_%s_cli' % name,
                                                os.path.join(ROOT, 'pyscripts', 'inference', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


WIRED = [('inference_softmax', 'predict_softmax_full_resolution', False),
         ('inference_softmax_msc', 'predict_softmax_multiscale', False),
         ('inference', 'predict_full_resolution', False),
         ('inference_msc', 'predict_knn_multiscale', False),
         ('prototype', 'multiscale_prototypes', True),
         ('prototype_msc', 'multiscale_prototypes', True),
         ('pseudo_softmax', 'pseudo_labels_softmax', True),
         ('pseudo_softmaxrw', 'pseudo_labels_softmax', True)]
NOT_WIRED = ['inference_crf', 'inference_crf_msc', 'inference_softmax_crf', 'inference_softmax_crf_msc',
             'pseudo_inference_msc', 'pseudo_inference_crf_msc', 'pseudo_softmaxrw_crf', 'pseudo_camrw_crf',
             'pseudo_denseposerw_crf']


def common_args(tmp_path):
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  return ['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg)]


@pytest.mark.parametrize('name,api_function,needs_labels', WIRED)
def test_wired_programs_take_a_list_and_refuse_what_they_cannot_read(name, api_function, needs_labels, tmp_path):
  prog, common = load_program(name), common_args(tmp_path)
  # a list that does not exist: the first guard, named, before --save_dir and the GPU
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'train.txt'])
  assert str(info.value.code) == ("data list 'train.txt' does not exist (ListDataset reads 'image [semantic_label "
                                  "instance_label]' per line); use --data_list synthetic or call spml_amd.inference.%s on "
                                  'your own images' % api_function)
  bare, _ = write_files(str(tmp_path / 'bare'), ['a.png'], labels=False)
  full, _ = write_files(str(tmp_path / 'full'), ['a.png'])
  # a list without label columns: refused by the programs that need them, before --save_dir and the GPU
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_dir', str(tmp_path / 'bare'), '--data_list', bare])
  if needs_labels:
    assert 'no label columns' in str(info.value.code) and bare in str(info.value.code)
  else:
    assert str(info.value.code) == '--save_dir is required'
  # a list that can be read passes the first guard: the next one speaks
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_dir', str(tmp_path / 'full'), '--data_list', full])
  assert str(info.value.code) == '--save_dir is required'
  if not torch.cuda.is_available():
    with pytest.raises(SystemExit) as info:
      prog.main(common + ['--data_dir', str(tmp_path / 'full'), '--data_list', full, '--save_dir', str(tmp_path / 'o')])
    assert 'no CPU fallback' in str(info.value.code) and not os.path.exists(str(tmp_path / 'o'))


@pytest.mark.parametrize('name', NOT_WIRED)
def test_programs_not_wired_yet_keep_their_refusal(name, tmp_path):
  full, _ = write_files(str(tmp_path / 'full'), ['a.png'])
  with pytest.raises(SystemExit) as info:
    load_program(name).main(common_args(tmp_path) + ['--data_dir', str(tmp_path / 'full'), '--data_list', full])
  text = str(info.value.code)
  assert text.startswith('file-list data loading (ListDataset) is outside the scope of this repository; use --data_list '
                         'synthetic or call spml_amd.inference.') and text.endswith(' on your own images')


def test_every_inference_program_is_one_or_the_other():
  have = sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, 'pyscripts', 'inference')) if f.endswith('.py'))
  assert have == sorted([w[0] for w in WIRED] + NOT_WIRED) and len(have) == 17


def test_image_source_names():
  assert inference_cli.output_name('/data/VOC/JPEGImages/2007_000032.jpg') == '2007_000032.png'
  assert inference_cli.output_name('nested/dir/x.y.jpg') == 'x.y.png'
  assert inference_cli.output_name('scene/frame_01.png') == 'frame_01.png'
  assert inference_cli.output_name('a.jpeg') == 'a.jpeg'                 # only '.jpg' is replaced, as in the reference
  image = inference_cli.SourceImage(3, '2007_000032.png', (5, 7), [], None, None)
  assert inference_cli.ListImageSource.bank_name(None, image) == '2007_000032.npy'
  synthetic = inference_cli.SourceImage(3, 'synthetic_0003', (5, 7), [], None, None)
  assert inference_cli.SyntheticImageSource.bank_name(None, synthetic) == 'synthetic_0003.npy'
  args = lambda data_list: types.SimpleNamespace(data_list=data_list)
  assert not inference_cli.reads_file_list(args(None)) and not inference_cli.reads_file_list(args('synthetic'))
  assert inference_cli.reads_file_list(args('val.txt'))


def test_label_pngs_are_written_into_directories_made_on_the_way(tmp_path):
  gray = np.arange(35, dtype=np.uint8).reshape(5, 7)
  color = vis.voc_color_map()[gray]
  paths = str(tmp_path / 'o' / 'semantic_gray' / 'sub' / 'a.png'), str(tmp_path / 'o' / 'semantic_color' / 'sub' / 'a.png')
  inference_cli.write_label_pngs(paths[0], paths[1], gray, color)
  got_gray, got_color = Image.open(paths[0]), Image.open(paths[1])
  assert got_gray.mode == 'L' and got_color.mode == 'RGB'
  assert np.array_equal(np.array(got_gray), gray) and np.array_equal(np.array(got_color), color)


# ------------------------------------------------------------------------------------------------------------------
# the record refusals of the library (host-only: the expression the launch itself evaluates)
def records_of(hw, scales, flip, crop, image_size=0):
  plan = transforms.plan_views(hw[0], hw[1], scales, flip, crop, image_size)
  return inference.view_records(plan), transforms.view_buffer_bytes(plan)


def test_view_record_refusals():
  assert _ffi.lib().spml_view_params_bytes() == _ffi.VIEW_PARAMS.itemsize == 40
  for hw, scales, flip, size, _ in cases.VIEW_CASES:
    records, (image_bytes, label_bytes) = records_of(hw, scales, flip, cases.CROP, size)
    assert _ffi.image_views_path_name(records, hw, image_bytes) == 'views'
    assert _ffi.image_views_path_name(records, hw, image_bytes, label_bytes, True) == 'views+labels'
    # a buffer one element short of the last plane
    assert _ffi.image_views_path_name(records, hw, image_bytes - 4) == 'unsupported'
    assert _ffi.image_views_path_name(records, hw, image_bytes, label_bytes - 8, True) == 'unsupported'
  records, (image_bytes, label_bytes) = records_of((23, 37), cases.SCALES, True, cases.CROP)
  name = lambda r, hw=(23, 37), ib=image_bytes, lb=label_bytes, lab=True: _ffi.image_views_path_name(r, hw, ib, lb, lab)

  def changed(index, **fields):
    r = records.copy()
    for key, value in fields.items():
      r[key][index] = value
    return r
  assert name(records) == 'views+labels'
  for hw in ((0, 37), (23, 0), (16385, 37), (23, 16385)):
    assert name(records, hw=hw) == 'unsupported', hw
  assert name(records, hw=(16384, 16384)) == 'views+labels'
  for fields in (dict(new_h=0), dict(new_w=0), dict(new_h=-1), dict(new_h=16385, pad_h=16385), dict(pad_w=16385),
                 dict(pad_h=10), dict(pad_w=17),                                     # pad < new (view 0 is 11 x 18)
                 dict(image_off=-16), dict(label_off=-16), dict(image_off=2), dict(label_off=4),
                 dict(image_off=image_bytes), dict(label_off=label_bytes)):
    assert name(changed(0, **fields)) == 'unsupported', fields
  assert name(changed(0, label_off=-16), lab=False) == 'views'                       # (not read without labels)
  # two planes that overlap: view 1 moved onto view 0
  assert name(changed(1, image_off=int(records['image_off'][0]))) == 'unsupported'
  assert name(changed(1, label_off=int(records['label_off'][0]))) == 'unsupported'
  assert name(changed(1, image_off=int(records['image_off'][1]) - 16)) == 'unsupported'
  # V outside [1, 64]
  many = np.concatenate([records] * 11)[:65].copy()
  step, lstep = 12 * 40 * 64 + 16, 8 * 40 * 64 + 16
  for k in range(65):
    many['image_off'][k], many['label_off'][k] = k * step, k * lstep
  assert _ffi.image_views_path_name(many[:64].copy(), (23, 37), 65 * step, 65 * lstep, True) == 'views+labels'
  assert _ffi.image_views_path_name(many, (23, 37), 65 * step, 65 * lstep, True) == 'unsupported'
  assert _ffi.lib().spml_image_views_path_name(None, 0, 23, 37, 0, 0, 0) == b'unsupported'


def test_label_export_refusals():
  for pred, valid, out in cases.EXPORT_CASES:
    assert _ffi.label_export_path_name(pred, valid, out) == 'export'
  assert _ffi.label_export_path_name((16384, 16384), (16384, 16384), (16384, 16384)) == 'export'
  for pred, valid, out in [((0, 9), (1, 1), (5, 5)), ((9, 16385), (1, 1), (5, 5)), ((9, 9), (0, 9), (5, 5)),
                           ((9, 9), (10, 9), (5, 5)), ((9, 9), (9, 10), (5, 5)), ((9, 9), (9, 9), (0, 5)),
                           ((9, 9), (9, 9), (5, 16385)), ((9, 9), (9, 9), (-1, 5))]:
    assert _ffi.label_export_path_name(pred, valid, out) == 'unsupported', (pred, valid, out)


def test_no_cpu_path():
  with pytest.raises(_ffi.SpmlHipError):
    inference.device_views(torch.zeros((5, 7, 3), dtype=torch.uint8), [1], False, (9, 9), cases.MEAN, cases.STD)
  with pytest.raises(_ffi.SpmlHipError):
    inference.export_label_map(torch.zeros((5, 7), dtype=torch.int64), (5, 7), (5, 7), torch.zeros((256, 3), dtype=torch.uint8))
