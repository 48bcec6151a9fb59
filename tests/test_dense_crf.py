"""The dense CRF as far as it runs without a GPU: the fp64 oracle (tests/dense_crf_ref.py) against closed forms, the
device-side restatement of the reference's image de-normalisation against the numpy lines themselves, the refusals of
CPU tensors, the host-only size and route queries of the C-ABI and the guards of the three `*_crf*` programs."""
import numpy as np
import pytest
import torch

import dense_crf_ref as ref
from spml_amd import _ffi, inference
from spml_amd.models.crf import DenseCRF
from test_inference_cli import load_program
from test_train_cli import YAML


def single_pixel_recursion(prob, weight, iterations):
  """N = 1: both kernels and both norms are 1, Q <- softmax(-U + weight * Q)."""
  logp = np.log(np.clip(prob.astype(np.float64), 1e-5, 1.0))
  q = np.exp(logp) / np.exp(logp).sum()
  for _ in range(iterations):
    x = logp + weight * q
    q = np.exp(x - x.max()) / np.exp(x - x.max()).sum()
  return q


def test_oracle_single_pixel_closed_form():
  prob = np.array([0.2, 0.5, 0.3], np.float32).reshape(3, 1, 1)
  image = np.array([[[10, 200, 30]]], np.uint8)
  for params in (ref.DEFAULTS, ref.ALTERNATIVE):
    got = ref.dense_crf(image, prob, **params)
    want = single_pixel_recursion(prob.reshape(3), params['pos_w'] + params['bi_w'], params['iter_max'])
    assert got.shape == (3, 1, 1) and got.dtype == np.float64
    np.testing.assert_allclose(got.reshape(3), want, rtol=0, atol=1e-14)
    assert abs(got.sum() - 1.0) < 1e-14


def test_oracle_far_apart_pixels_of_different_colour_decouple():
  """Black and white are 3 * 255^2 / (2 * 3^2) = 10837 apart in the bilateral exponent, and one position is 100 standard
  deviations at pos_xy_std = 0.01 (exponent -5000): both kernels are the identity in fp64, both norms 1, and every pixel
  follows the single-pixel recursion on its own."""
  image = np.zeros((1, 21, 3), np.uint8)
  image[0, 20] = 255
  prob = np.full((2, 1, 21), 0.5, np.float32)
  prob[:, 0, 0] = (0.3, 0.7)
  prob[:, 0, 20] = (0.9, 0.1)
  k1, k2 = ref.kernels(image[:, [0, 20]], 0.01, 67, 3)
  assert np.array_equal(k1, np.eye(2)) and np.array_equal(k2, np.eye(2))
  got = ref.dense_crf(image[:, [0, 20]], prob[:, :, [0, 20]], iter_max=10, pos_w=3, pos_xy_std=0.01, bi_w=4, bi_xy_std=67,
                      bi_rgb_std=3)
  for col, p in ((0, (0.3, 0.7)), (1, (0.9, 0.1))):
    np.testing.assert_allclose(got[:, 0, col], single_pixel_recursion(np.array(p, np.float32), 7, 10), rtol=0, atol=1e-14)
  # under the bilateral kernel alone the white pixel does not see the twenty black ones, which do see each other
  alone = ref.dense_crf(image, prob, iter_max=5, pos_w=0, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
  np.testing.assert_allclose(alone[:, 0, 20], single_pixel_recursion(np.array((0.9, 0.1), np.float32), 4, 5), rtol=0,
                             atol=1e-14)
  assert abs(alone[0, 0, 0] - single_pixel_recursion(np.array((0.3, 0.7), np.float32), 4, 5)[0]) > 1e-3


def test_oracle_without_iterations_returns_the_clipped_renormalised_input():
  rng = np.random.RandomState(3)
  prob = rng.rand(4, 3, 5).astype(np.float32) * 1.5          # not normalised, values above 1
  prob[1, 0, 0] = 0.0
  prob[:, 2, 2] = 0.0                                        # a pixel of zeros only: uniform after the clip
  image = rng.randint(0, 256, size=(3, 5, 3)).astype(np.uint8)
  got = ref.dense_crf(image, prob, **dict(ref.DEFAULTS, iter_max=0))
  clipped = np.clip(prob.astype(np.float64), 1e-5, 1.0)
  np.testing.assert_allclose(got, clipped / clipped.sum(0, keepdims=True), rtol=0, atol=1e-15)
  np.testing.assert_allclose(got[:, 2, 2], 0.25, rtol=0, atol=1e-15)


def test_oracle_messages_are_symmetrically_normalised():
  """One iteration by hand on 2 x 2 pixels, from the definition: n = 1 / sqrt(K 1 + 1e-20), M = n * (K (n Q))."""
  rng = np.random.RandomState(5)
  image = rng.randint(0, 256, size=(2, 2, 3)).astype(np.uint8)
  prob = rng.rand(3, 2, 2).astype(np.float32)
  k1, k2 = ref.kernels(image, 1, 67, 3)
  assert np.allclose(np.diag(k1), 1) and np.allclose(np.diag(k2), 1) and np.array_equal(k1, k1.T)
  assert abs(k1[0, 1] - np.exp(-0.5)) < 1e-15 and abs(k1[0, 3] - np.exp(-1.0)) < 1e-15      # (x, y) in pixels
  logp = np.log(np.clip(prob.astype(np.float64), 1e-5, 1)).reshape(3, 4)
  q = np.exp(logp) / np.exp(logp).sum(0)
  x = logp.copy()
  for weight, k in ((3, k1), (4, k2)):
    n = 1 / np.sqrt(k.sum(1) + 1e-20)
    for i in range(4):
      x[:, i] += weight * n[i] * sum(k[i, j] * n[j] * q[:, j] for j in range(4))
  want = np.exp(x - x.max(0)) / np.exp(x - x.max(0)).sum(0)
  got = ref.dense_crf(image, prob, **dict(ref.DEFAULTS, iter_max=1))
  np.testing.assert_allclose(got.reshape(3, 4), want, rtol=0, atol=1e-14)


def reference_denormalize(image_chw, pixel_means, pixel_stds):
  """pyscripts/inference/inference_softmax_crf_msc.py:159-164 of twke18/SPML, the lines themselves."""
  image = image_chw.astype(np.float32)
  image = image.transpose(1, 2, 0)
  image *= np.reshape(pixel_stds, (1, 1, 3))
  image += np.reshape(pixel_means, (1, 1, 3))
  image = image * 255
  image = image.astype(np.uint8)
  return image


def denormalize_case(h, w, seed):
  """A normalised image whose de-normalised values sit on and next to the integers (the truncation is sensitive to the
  last bit there) and, in the second half, anywhere in 0..255."""
  from spml_amd.config.default import config
  means, stds = config.network.pixel_means, config.network.pixel_stds
  rng = np.random.RandomState(seed)
  u8 = rng.randint(0, 256, size=(3, h, w))
  x = (u8 / 255.0 - np.reshape(means, (3, 1, 1))) / np.reshape(stds, (3, 1, 1))
  x[:, h // 2:] = ((rng.rand(3, h - h // 2, w) * 254.9 + 0.05) / 255.0 - np.reshape(means, (3, 1, 1))) / \
      np.reshape(stds, (3, 1, 1))
  return x.astype(np.float32), means, stds


def test_denormalized_uint8_is_the_reference_lines_on_every_pixel():
  x, means, stds = denormalize_case(37, 53, 11)
  want = reference_denormalize(x.copy(), means, stds)
  got = inference.denormalized_uint8(torch.from_numpy(x), means, stds)
  assert got.dtype == torch.uint8 and tuple(got.shape) == (37, 53, 3) and got.is_contiguous()
  assert np.array_equal(got.numpy(), want)
  assert torch.equal(inference.denormalized_uint8(torch.from_numpy(x)[None], means, stds), got)
  # the float64 steps matter: all-float32 arithmetic differs from the reference on some pixel of this image
  f32 = ((torch.from_numpy(x).permute(1, 2, 0) * torch.tensor(stds, dtype=torch.float32) +
          torch.tensor(means, dtype=torch.float32)) * 255).to(torch.uint8)
  assert not np.array_equal(f32.numpy(), want)
  with pytest.raises(ValueError):
    inference.denormalized_uint8(torch.zeros(4, 5, 5), means, stds)


def test_no_cpu_fallback():
  crf = DenseCRF(**ref.DEFAULTS)
  image, prob = ref.blocky(7, 5, 2, 1)
  with pytest.raises(_ffi.SpmlHipError):
    crf(torch.from_numpy(image), torch.from_numpy(prob))
  with pytest.raises(_ffi.SpmlHipError):
    inference.dense_crf_refine(torch.from_numpy(image), torch.from_numpy(prob), crf)
  with pytest.raises(_ffi.SpmlHipError):
    crf.prepare(torch.from_numpy(image), 2)
  if not torch.cuda.is_available():
    with pytest.raises(_ffi.SpmlHipError):
      crf(image, prob)                                       # the numpy route goes through the GPU as well


def test_workspace_query_is_host_only():
  lib = _ffi.lib()
  for h, w, c in ref.SHAPES + [(375, 500, 21), (2048, 2048, 64)]:
    n = h * w
    got = lib.spml_dense_crf_workspace_bytes(h, w, c)
    assert got > 7 * n * c * 4 and got % 256 == 0, (h, w, c)     # five class maps and two split-f16 operand images
  assert lib.spml_dense_crf_workspace_bytes(33, 47, 32) < lib.spml_dense_crf_workspace_bytes(33, 47, 33)
  for bad in ((0, 5, 3), (5, 0, 3), (5, 5, 0), (-1, 5, 3), (2049, 5, 3), (5, 2049, 3), (5, 5, 65)):
    assert lib.spml_dense_crf_workspace_bytes(*bad) == 0, bad
  with pytest.raises(_ffi.SpmlHipError, match='64 classes'):
    _ffi.dense_crf_workspace(5, 5, 65, 'cpu')


def test_path_name_of_every_gpu_test_shape():
  for h, w, c in ref.SHAPES:
    columns = 32 if c <= 32 else 64
    assert _ffi.dense_crf_path_name(h, w, c, 1) == 'pairs_mfma_f16x2_c%d+separable_r6' % columns
    assert _ffi.dense_crf_path_name(h, w, c, 3) == 'pairs_mfma_f16x2_c%d+separable_r18' % columns
    assert DenseCRF(**ref.ALTERNATIVE).path_name(h, w, c) == 'pairs_mfma_f16x2_c%d+separable_r18' % columns
  assert _ffi.dense_crf_path_name(375, 500, 21, 1) == 'pairs_mfma_f16x2_c32+separable_r6'
  assert _ffi.dense_crf_path_name(8, 8, 32, 0.5) == 'pairs_mfma_f16x2_c32+separable_r3'
  assert _ffi.dense_crf_path_name(8, 8, 33, 1000) == 'pairs_mfma_f16x2_c64+separable_r2047'
  assert _ffi.dense_crf_path_name(17, 129, 65, 1) == 'unsupported'
  assert _ffi.dense_crf_path_name(2049, 8, 3, 1) == 'unsupported'
  assert _ffi.dense_crf_path_name(8, 8, 3, 0) == 'unsupported'


@pytest.mark.parametrize('name', ['inference_softmax_crf', 'inference_softmax_crf_msc', 'pseudo_inference_crf_msc'])
def test_crf_programs_run_the_guards_in_the_shared_order(name, tmp_path):
  prog = load_program(name)
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  common = ['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--crf_iter_max', '3']
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'train.txt'])
  assert 'ListDataset' in str(info.value.code) and 'spml_amd.inference.dense_crf_refine ' in str(info.value.code)
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'synthetic'])
  assert str(info.value.code) == '--save_dir is required'
  if torch.cuda.is_available():
    return
  import os
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'synthetic', '--save_dir', str(tmp_path / 'o')])
  assert info.value.code not in (0, None) and 'no CPU fallback' in str(info.value.code)
  assert not os.path.exists(str(tmp_path / 'o'))


def test_pair_kernels_do_not_spill_and_hold_no_hand_issued_instruction():
  """csrc/dense_crf.hip compiled with the product flags: no scratch in any kernel, and no inline assembly -- every MFMA
  comes from the compiler's builtin, so the compiler sees every dependency and pads the wait states itself (nothing for
  tools/check_asm_hazards.py to re-derive).  The three instantiations of the pair kernel carry the MFMAs the design
  counts per tile of j: two for the exponents, then per k step two (norms) or three per 32 class columns."""
  import os
  import re
  import subprocess
  import tempfile
  from spml_amd import _build
  with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, 'crf.s')
    cmd = [_build._hipcc()] + _build.FLAGS + ['-DSPML_BUILD_EXPERIMENT=0', '-S', '--cuda-device-only',
                                              os.path.join(_build.CSRC, 'dense_crf.hip'), '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
  assert 'scratch_' not in text and ';;#ASMSTART' not in text
  assert set(re.findall(r'\.vgpr_spill_count:\s+(\d+)', text)) == {'0'}
  assert set(re.findall(r'\.private_segment_fixed_size:\s+(\d+)', text)) == {'0'}
  kernels = dict(re.findall(r'^(_ZN4spml\S*crf_pairs\S*):[^\n]*\n(.*?)s_endpgm', text, flags=re.S | re.M))
  counts = sorted(body.count('v_mfma_f32_32x32x16_f16') for body in kernels.values())
  assert counts == [2 + 2 * 2, 2 + 2 * 3, 2 + 2 * 3 * 2], counts
  assert all(body.count('v_exp_f32') >= 16 for body in kernels.values())
