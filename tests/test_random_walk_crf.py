"""The random-walk + dense-CRF pseudo labels as far as they run without a GPU: the new C-ABI symbol, the
guards of the two programs, the CAM helpers against the reference's lines, the refusals of CPU tensors and the test inputs
of tests/random_walk_crf_ref.py with their label caps."""
import os
import re

import numpy as np
import pytest
import torch

import dense_crf_ref
import random_walk_crf_ref as ref
from spml_amd import _ffi, inference
from spml_amd.models.crf import DenseCRF
from test_inference_cli import load_program, test_every_program_runs_the_guards_in_one_order as run_the_guards
from test_train_cli import ROOT, YAML

SYMBOL = 'spml_dense_crf_infer_upsampled_f32'


def test_header_declares_the_symbol_and_the_ffi_lists_it():
  header = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  declaration = re.search(r'^int %s\(([^;]*)\);' % SYMBOL, header, flags=re.M)
  assert declaration is not None
  arguments = [a.strip() for a in declaration.group(1).replace('\n', ' ').split(',')]
  assert arguments == ['const float* lowres', 'int ncls', 'int oh', 'int ow', 'int h', 'int w', 'int iter_max',
                       'float pos_w', 'float bi_w', 'float* q', 'int64_t* labels', 'int64_t* labels_before',
                       'float* prob_up', 'void* ws', 'size_t ws_bytes', 'void* stream']
  assert 'pseudo_softmaxrw_crf.py:172-185' in header and header.count('spml/models/crf.py:23-41') >= 5
  assert '#define SPML_ABI_VERSION 8' in header
  assert SYMBOL in _ffi.EXPORTS and len(_ffi._SIGNATURES[SYMBOL][1]) == len(arguments)
  assert hasattr(_ffi.lib(), SYMBOL)                          # the built library exports it


@pytest.mark.parametrize('name,api_function', [('pseudo_softmaxrw_crf', 'pseudo_labels_softmax_crf'),
                                               ('pseudo_camrw_crf', 'random_walk_crf_refine')])
def test_both_programs_run_the_guards_in_the_shared_order(name, api_function, tmp_path):
  run_the_guards(name, api_function, tmp_path)
  prog = load_program(name)
  assert prog.WALK_STEPS == 6
  if name == 'pseudo_softmaxrw_crf':
    assert (tuple(prog.SCALES), prog.COMBINE) == ((1,), 'prob_mean')
  else:
    assert prog.ALPHA == 6
  # the six --crf_* options are read before any guard refuses the call
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  with pytest.raises(SystemExit) as info:
    prog.main(['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--data_list', 'synthetic', '--crf_iter_max',
               '2', '--crf_pos_xy_std', '1', '--crf_pos_w', '3', '--crf_bi_xy_std', '67', '--crf_bi_rgb_std', '3',
               '--crf_bi_w', '4'])
  assert str(info.value.code) == '--save_dir is required'


def cam_case(h, w, seed):
  """CAMs of classes 3, 8 and 20 (entries 2, 7, 19) in [0, 1]; the top-left quarter carries no activation at all."""
  rng = np.random.RandomState(seed)
  cam = {k: rng.rand(h, w).astype(np.float32) for k in (2, 7, 19)}
  for v in cam.values():
    v[:h // 2, :w // 2] = 0.0
  return cam


def test_cam_with_background_is_the_reference_lines():
  h, w = 37, 53
  cam = cam_case(h, w, 5)
  want = ref.reference_cam_full(cam, (h, w), 6)
  got = inference.cam_with_background({k: torch.from_numpy(v) for k, v in cam.items()}, (h, w), 21, 6)
  assert got.dtype == torch.float32 and tuple(got.shape) == (21, h, w)
  np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=0)
  for k, v in cam.items():                                    # entry k is class k + 1, bit for bit
    assert np.array_equal(got[k + 1].numpy(), v)
  absent = [c for c in range(1, 21) if c - 1 not in cam]
  assert not got[absent].any()
  assert np.array_equal(got[0, :h // 2, :w // 2].numpy(), np.ones((h // 2, w // 2), np.float32))   # no activation: exactly 1
  assert float(got[0].min()) >= 0.0 and float(got[0, h // 2:, w // 2:].max()) < 1.0
  # numpy maps are taken as they are, and another alpha is another power
  from_numpy = inference.cam_with_background(cam, (h, w), 21, 6)
  assert torch.equal(from_numpy, got)
  np.testing.assert_allclose(inference.cam_with_background(cam, (h, w), 21, 2).numpy(),
                             ref.reference_cam_full(cam, (h, w), 2), rtol=1e-6, atol=0)


@pytest.mark.parametrize('hw', [(37, 53), (64, 80), (65, 65)])
def test_downsampled_cam_is_the_reference_line(hw):
  full = ref.reference_cam_full(cam_case(hw[0], hw[1], 6), hw, 6)
  want = ref.reference_cam_down(full)
  got = inference.downsampled_cam(torch.from_numpy(full))
  assert tuple(got.shape) == (21, hw[0] // 8, hw[1] // 8) == tuple(want.shape)
  np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6, atol=0)


def test_no_cpu_fallback():
  crf = DenseCRF(**dense_crf_ref.DEFAULTS)
  image, low = ref.walked_map(16, 24, 2, 1)
  image_t, low_t = torch.from_numpy(image), torch.from_numpy(low)
  with pytest.raises(_ffi.SpmlHipError):
    crf.refine_upsampled(image_t, low_t)
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_upsampled(torch.zeros(16, dtype=torch.uint8), low_t, (16, 24))
  with pytest.raises(_ffi.SpmlHipError):
    inference.random_walk_crf_refine(image_t, low_t, crf)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.dense_crf_infer_upsampled(low_t, (16, 24), 1, 3.0, 4.0, torch.zeros(16, dtype=torch.uint8))


@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_walked_map_is_what_the_walk_hands_over(shape):
  h, w, c = shape
  image, low = ref.walked_map(h, w, c, ref.SEED)
  assert image.dtype == np.uint8 and image.shape == (h, w, 3)
  assert low.dtype == np.float32 and low.shape == (c, max(h // 8, 1), max(w // 8, 1))
  assert np.array_equal(image, dense_crf_ref.blocky(h, w, c, ref.SEED)[0])
  live = c - 1 if c > 2 else c
  assert np.array_equal(low[:live].reshape(live, -1).max(1), np.ones(live, np.float32)) and low.min() >= 0.0
  if c > 2:
    assert not low[c - 1].any()
  up = ref.upsampled(low, (h, w))
  assert up.dtype == np.float32 and up.shape == (c, h, w) and up.min() >= 0.0 and up.max() <= 1.0


@pytest.mark.parametrize('parameters', ['defaults', 'alternative'])
@pytest.mark.parametrize('shape', [(1, 300, 4), (16, 24, 2)], ids=lambda s: '%dx%dx%d' % s)
def test_label_caps_hold_on_the_two_smallest_comparing_shapes(shape, parameters):
  """The yardstick alone, so the caps are also checked without a GPU: the share of pixels under the margin stays under
  the cap, and the CRF changes labels."""
  _, _, up, want = ref.yardstick(shape, parameters)
  keep, left_out = ref.under_margin(want)
  print('%s %s: %.4f of the pixels under the margin' % (shape, parameters, left_out))
  assert ref.label_cap(shape) == 0.02 and left_out <= 0.02
  assert abs(want.sum(0) - 1).max() < 1e-12
  assert (want.argmax(0) != up.argmax(0)).any(), 'the CRF changed no label'
  assert ref.label_cap((8, 8, 3)) is None and ref.label_cap((17, 129, 64)) == 0.20
