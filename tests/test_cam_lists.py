"""The image-tag recipe on image files, as far as it runs without a GPU: the tap model of `spml_cam_ingest_f32` against
the reference's own lines (tests/cam_ingest_ref.py), the header / `_ffi` agreement and the host-side refusals of the entry,
the guards of `pseudo_softmaxrw.py --cam_dir` and `inference_msc.py --pseudo_tags`, and the CAM files `ImageSource` reads."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cam_ingest_ref as ref
from spml_amd import _ffi, inference, inference_cli
from test_inference_io import NOT_WIRED, WIRED, common_args, load_program, write_files
from test_train_cli import ROOT


# ------------------------------------------------------------------------------------------------------------------
# the yardstick
@pytest.mark.parametrize('case', ref.CASES, ids=ref.IDS)
def test_reference_lines_are_the_four_tap_mean(case):
  """`F.interpolate(scale_factor=1/8)` takes the given factor: source coordinate 8 d + 3.5, weights 1/2, 1/2 in both axes,
  at every size -- also where h % 8 != 0, where `size=(h // 8, w // 8)` would give another coordinate."""
  h, w, ncls, keys, _ = case
  planes = ref.planes_of(case)
  want, got = ref.four_tap(planes, keys, (h, w), ncls), ref.reference(planes, keys, (h, w), ncls)
  assert got.dtype == np.float32 and got.shape == want.shape == (ncls, h // 8, w // 8)
  dev, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
  print('%s: max |R - Y| = %.3e = %.2f units of 2^-24 max |Y| (max |Y| = %.4f)' % (case[:4], dev, dev / (ref.U * scale), scale))
  assert dev <= 4 * ref.U * scale
  absent = [c for c in range(1, ncls) if c - 1 not in keys]
  assert not want[absent].any() and not got[absent].any()
  if not keys:
    assert (want[0] == 1.0).all() and (got[0] == 1.0).all()
  if case[4] < 0:                                     # every class present, negative activations: a background above 1
    assert len(keys) == ncls - 1 and float(want[0].max()) > 1.0


def test_an_absent_class_puts_a_zero_into_the_maximum():
  """The background of :111 runs over the zero planes too: with negative activations and a class missing the maximum is
  0, with every class present it is the (negative) activation."""
  plane = np.full((1, 8, 8), -0.5, np.float32)
  assert np.allclose(ref.four_tap(plane, [0], (8, 8), 2)[0], 1.5 ** 6)
  assert np.allclose(ref.four_tap(plane, [0], (8, 8), 3)[0], 1.0)
  assert np.array_equal(ref.reference(plane, [0], (8, 8), 3)[0], np.ones((1, 1), np.float32))
  assert np.array_equal(ref.four_tap(np.zeros((0, 16, 24), np.float32), [], (16, 24), 1), np.ones((1, 2, 3)))


# ------------------------------------------------------------------------------------------------------------------
# the entry points: header, wrapper table, refusals (decided on the host before any launch)
def declared(name):
  text = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  result, params = re.search(r'([a-z_ ]+\*?)\s*\b%s\s*\(([^)]*)\)\s*;' % name, text).groups()
  return result.strip(), [p.strip() for p in params.split(',')]


def test_header_and_ffi_agree_on_the_two_symbols():
  kinds = lambda params: [ctypes.c_void_p if '*' in p else ctypes.c_int for p in params]
  result, params = declared('spml_cam_ingest_f32')
  assert result == 'int' and [p.split()[-1].lstrip('*') for p in params] == \
      ['planes', 'classes', 'K', 'h', 'w', 'ncls', 'alpha', 'out', 'stream']
  assert _ffi._SIGNATURES['spml_cam_ingest_f32'] == (ctypes.c_int, kinds(params))
  result, params = declared('spml_cam_ingest_path_name')
  assert result == 'const char*' and [p.split()[-1] for p in params] == ['K', 'h', 'w', 'ncls']
  assert _ffi._SIGNATURES['spml_cam_ingest_path_name'] == (ctypes.c_char_p, kinds(params))
  assert {'spml_cam_ingest_f32', 'spml_cam_ingest_path_name'} <= set(_ffi.EXPORTS)
  header = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  assert 'pseudo_camrw_crf.py:108-111' in header and ':151-152' in header
  assert _ffi.ABI_VERSION == 8 == _ffi.lib().spml_abi_version()          # additive: the version stays


def test_path_name_and_refusals():
  for h, w, ncls, keys, _ in ref.CASES:
    assert _ffi.cam_ingest_path_name(len(keys), h, w, ncls) == 'cam_ingest'
  assert _ffi.cam_ingest_path_name(3, 375, 500, 21) == 'cam_ingest' and _ffi.cam_ingest_path_name(0, 8, 8, 1) == 'cam_ingest'
  assert _ffi.cam_ingest_path_name(255, 16384, 16384, 256) == 'cam_ingest'
  for k, h, w, ncls in [(0, 7, 8, 21), (0, 8, 7, 21), (21, 16, 16, 21), (1, 16, 16, 1), (-1, 16, 16, 21), (0, 16, 16, 0),
                        (0, 16, 16, 257), (0, 16385, 16, 21), (0, 16, 16385, 21)]:
    assert _ffi.cam_ingest_path_name(k, h, w, ncls) == 'unsupported', (k, h, w, ncls)

  if torch.cuda.is_available():
    return          # (the raw host addresses below must never reach a launch: tests/test_cam_lists_gpu.py refuses on device buffers)
  lib = _ffi.lib()
  arena = (ctypes.c_ubyte * (1 << 16))()                 # host memory: nothing below reaches a launch
  base = (ctypes.addressof(arena) + 63) // 64 * 64
  planes, out = base, base + (1 << 15)                   # 3 * 16 * 16 * 4 = 3072 bytes of planes, 21 * 2 * 2 * 4 of output

  def call(planes=planes, keys=(2, 7, 19), k=None, hw=(16, 16), ncls=21, alpha=6, out=out):
    host = (ctypes.c_int * max(len(keys), 1))(*keys)
    return lib.spml_cam_ingest_f32(ctypes.c_void_p(planes), host, len(keys) if k is None else k, hw[0], hw[1], ncls, alpha,
                                   ctypes.c_void_p(out), None)
  for kw in (dict(hw=(7, 16)), dict(hw=(16, 7)), dict(hw=(16385, 16)), dict(keys=(0, 1, 2), ncls=3), dict(ncls=0),
             dict(ncls=257), dict(keys=(), k=-1)):
    assert call(**kw) == -2, kw                          # SPML_ERR_UNSUPPORTED
  for kw in (dict(keys=(2, 20, 19)), dict(keys=(2, -1, 19)), dict(keys=(2, 7, 2)), dict(keys=(1,), ncls=2), dict(alpha=-1),
             dict(out=None), dict(planes=None), dict(planes=planes + 2), dict(out=out + 1), dict(out=planes),
             dict(out=planes + 3068), dict(planes=out + 4 * 83)):
    assert call(**kw) == -1, kw                          # SPML_ERR_INVALID_ARG
  assert lib.spml_cam_ingest_f32(ctypes.c_void_p(planes), None, 3, 16, 16, 21, 6, ctypes.c_void_p(out), None) == -1


def test_no_cpu_path_and_the_smallest_image():
  views = [(torch.zeros(1, 3, 16, 16), (16, 16), False)]
  planes = torch.zeros(1, 16, 16)
  with pytest.raises(_ffi.SpmlHipError):
    inference.pseudo_labels_cam(None, views, (16, 16), planes, [3], 21)
  with pytest.raises(_ffi.SpmlHipError):
    inference.pseudo_labels_cam_crf(None, views, (16, 16), planes, [3], 21, torch.zeros(16, 16, 3, dtype=torch.uint8), None)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.cam_ingest(planes, [3], (16, 16), 21, 6)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.cam_ingest(torch.zeros(0, 16, 16), [], (16, 16), 21, 6, out=torch.zeros(21, 2, 2))
  for hw in ((7, 16), (16, 7)):
    small = [(torch.zeros(1, 3, 16, 16), hw, False)]
    with pytest.raises(ValueError, match='smaller than 8 x 8'):
      inference.pseudo_labels_cam(None, small, hw, None, [], 21)
    with pytest.raises(ValueError, match='smaller than 8 x 8'):
      inference.pseudo_labels_cam_crf(None, small, hw, None, [], 21, torch.zeros(hw + (3,), dtype=torch.uint8), None)
  with pytest.raises(ValueError, match='un-padded image'):
    inference.pseudo_labels_cam_crf(None, views, (16, 16), None, [], 21, torch.zeros(16, 17, 3, dtype=torch.uint8), None)


# ------------------------------------------------------------------------------------------------------------------
# the two options
def test_cam_dir_runs_the_guards_in_the_shared_order(tmp_path):
  prog, common = load_program('pseudo_softmaxrw'), common_args(tmp_path) + ['--cam_dir', str(tmp_path / 'cams')]
  assert prog.ALPHA == 6 and prog.WALK_STEPS == 6 and tuple(prog.SCALES) == (1,)
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'train.txt'])
  assert str(info.value.code).startswith("data list 'train.txt' does not exist")
  bare, _ = write_files(str(tmp_path / 'bare'), ['a.png'], labels=False)
  full, _ = write_files(str(tmp_path / 'full'), ['a.png'])
  for root, path in (('bare', bare), ('full', full)):     # the CAM walk never reads the label map: a bare list passes
    listed = common + ['--data_dir', str(tmp_path / root), '--data_list', path]
    with pytest.raises(SystemExit) as info:
      prog.main(listed)
    assert str(info.value.code) == '--save_dir is required'
    if not torch.cuda.is_available():
      with pytest.raises(SystemExit) as info:
        prog.main(listed + ['--save_dir', str(tmp_path / 'o')])
      assert 'no CPU fallback' in str(info.value.code) and not os.path.exists(str(tmp_path / 'o'))
  # without the option the program needs the label columns, as before; its two relatives do not take the CAM route
  with pytest.raises(SystemExit) as info:
    prog.main(common_args(tmp_path) + ['--data_dir', str(tmp_path / 'bare'), '--data_list', bare])
  assert 'no label columns' in str(info.value.code)
  with pytest.raises(SystemExit) as info:
    load_program('pseudo_softmax').main(common + ['--data_dir', str(tmp_path / 'bare'), '--data_list', bare])
  assert 'no label columns' in str(info.value.code)
  with pytest.raises(SystemExit) as info:
    load_program('pseudo_softmaxrw_crf').main(common + ['--data_dir', str(tmp_path / 'full'), '--data_list', full])
  assert str(info.value.code).startswith('file-list data loading (ListDataset) is outside the scope')


def test_pseudo_tags_is_on_inference_msc_alone_and_runs_the_guards_in_the_shared_order(tmp_path):
  for name in [w[0] for w in WIRED] + NOT_WIRED:
    if name == 'inference_msc':
      continue
    with pytest.raises(SystemExit) as info:
      load_program(name).main(common_args(tmp_path) + ['--pseudo_tags'])
    assert info.value.code == 2, name                     # argparse: unrecognized arguments: --pseudo_tags
  prog = load_program('inference_msc')
  assert prog.PSEUDO_SCALES == load_program('pseudo_inference_msc').SCALES == [0.5, 1, 1.5, 2]
  assert prog.PSEUDO_FLOOR == load_program('pseudo_inference_msc').FLOOR == 0.15
  bare, _ = write_files(str(tmp_path / 'bare'), ['a.png'], labels=False)
  full, _ = write_files(str(tmp_path / 'full'), ['a.png'])
  for extra in ([], ['--crf']):
    common = common_args(tmp_path) + ['--pseudo_tags'] + extra
    with pytest.raises(SystemExit) as info:
      prog.main(common + ['--data_list', 'train.txt'])
    assert str(info.value.code).startswith("data list 'train.txt' does not exist")
    # the tags come from the label map: a bare list is refused before --save_dir and the GPU are looked at
    with pytest.raises(SystemExit) as info:
      prog.main(common + ['--data_dir', str(tmp_path / 'bare'), '--data_list', bare, '--save_dir', str(tmp_path / 'o')])
    assert 'no label columns' in str(info.value.code) and bare in str(info.value.code)
    assert not os.path.exists(str(tmp_path / 'o'))
    listed = common + ['--data_dir', str(tmp_path / 'full'), '--data_list', full]
    with pytest.raises(SystemExit) as info:
      prog.main(listed)
    assert str(info.value.code) == '--save_dir is required'
    if not torch.cuda.is_available():
      with pytest.raises(SystemExit) as info:
        prog.main(listed + ['--save_dir', str(tmp_path / 'o')])
      assert 'no CPU fallback' in str(info.value.code) and not os.path.exists(str(tmp_path / 'o'))
  # without the option a bare list still passes the first guard
  with pytest.raises(SystemExit) as info:
    prog.main(common_args(tmp_path) + ['--data_dir', str(tmp_path / 'bare'), '--data_list', bare])
  assert str(info.value.code) == '--save_dir is required'


# ------------------------------------------------------------------------------------------------------------------
# the CAM files
def test_cam_file_is_read_in_the_dicts_order_as_fp32(tmp_path):
  rng = np.random.RandomState(3)
  cams = {19: rng.rand(13, 17), 2: rng.rand(13, 17).astype(np.float32), 7: rng.rand(13, 17).astype(np.float16)}
  np.save(str(tmp_path / 'a.npy'), cams)
  keys, planes = inference_cli.read_cam_file(str(tmp_path), 'a.npy', (13, 17), 21)
  assert keys.dtype == np.int32 and list(keys) == [19, 2, 7]
  assert len(planes) == 3 and all(p.dtype == np.float32 and p.shape == (13, 17) and p.flags['C_CONTIGUOUS'] for p in planes)
  for plane, value in zip(planes, cams.values()):
    assert np.array_equal(plane, value.astype(np.float32))
  np.save(str(tmp_path / 'empty.npy'), {})
  keys, planes = inference_cli.read_cam_file(str(tmp_path), 'empty.npy', (13, 17), 21)
  assert keys.shape == (0,) and planes == []


def test_bad_cam_files_end_the_run_with_a_message_that_names_the_file(tmp_path):
  with pytest.raises(SystemExit) as info:
    inference_cli.read_cam_file(str(tmp_path), '2007_000032.npy', (13, 17), 21)
  assert str(tmp_path / '2007_000032.npy') in str(info.value.code) and 'does not exist' in str(info.value.code)
  np.save(str(tmp_path / 'shape.npy'), {3: np.zeros((13, 17), np.float32), 5: np.zeros((17, 13), np.float32)})
  with pytest.raises(SystemExit) as info:
    inference_cli.read_cam_file(str(tmp_path), 'shape.npy', (13, 17), 21)
  text = str(info.value.code)
  assert str(tmp_path / 'shape.npy') in text and 'key 5' in text and '17 x 13' in text and '13 x 17' in text
  for key in (20, -1):
    np.save(str(tmp_path / 'key.npy'), {key: np.zeros((13, 17), np.float32)})
    with pytest.raises(SystemExit) as info:
      inference_cli.read_cam_file(str(tmp_path), 'key.npy', (13, 17), 21)
    assert str(tmp_path / 'key.npy') in str(info.value.code) and 'key %d' % key in str(info.value.code)
  np.save(str(tmp_path / 'last.npy'), {19: np.zeros((13, 17), np.float32)})
  assert list(inference_cli.read_cam_file(str(tmp_path), 'last.npy', (13, 17), 21)[0]) == [19]
