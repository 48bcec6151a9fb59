"""The kNN label inference with the dense CRF as far as it runs without a GPU: the two new C-ABI symbols, the
guards of the three programs, the framework route against the reference's lines, the refusals of CPU tensors and the
test inputs of tests/knn_crf_ref.py with their label caps."""
import os
import re

import numpy as np
import pytest
import torch

import dense_crf_ref
import knn_crf_ref as ref
from spml_amd import _ffi, inference
from spml_amd.models.crf import DenseCRF
from test_inference_cli import load_program, test_every_program_runs_the_guards_in_one_order as run_the_guards
from test_train_cli import ROOT, YAML

SIZE_SYMBOL = 'spml_dense_crf_votes_workspace_bytes'
SYMBOL = 'spml_dense_crf_infer_votes_f32'
PROGRAMS = [('inference', 'predict_full_resolution'), ('inference_crf', 'predict_knn_full_resolution_crf'),
            ('inference_crf_msc', 'predict_knn_multiscale')]


def declared_arguments(header, result, symbol):
  declaration = re.search(r'^%s %s\(([^;]*)\);' % (result, symbol), header, flags=re.M)
  assert declaration is not None, symbol
  return [' '.join(a.split()) for a in declaration.group(1).split(',')]


def test_header_declares_both_symbols_and_the_ffi_lists_them():
  header = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  assert declared_arguments(header, 'size_t', SIZE_SYMBOL) == ['int m', 'int ncls']
  arguments = declared_arguments(header, 'int', SYMBOL)
  assert arguments == ['const int64_t* clu', 'const int64_t* topk', 'int m', 'int k', 'int ncls', 'int h', 'int w',
                       'int iter_max', 'float pos_w', 'float bi_w', 'float* q', 'int64_t* labels',
                       'int64_t* labels_before', 'float* prob', 'void* table_ws', 'size_t table_ws_bytes', 'void* ws',
                       'size_t ws_bytes', 'void* stream']
  comment = header[header.index(' * ' + SYMBOL):]
  comment = comment[:comment.index('\n * spml_dense_crf_path_name')]
  assert 'inference_crf.py:237-254' in comment and 'spml/models/crf.py:23-41' in comment
  assert '#define SPML_ABI_VERSION 8' in header
  for symbol, count in ((SIZE_SYMBOL, 2), (SYMBOL, len(arguments))):
    assert symbol in _ffi.EXPORTS and len(_ffi._SIGNATURES[symbol][1]) == count
    assert hasattr(_ffi.lib(), symbol)                        # the built library exports it


def test_table_size_is_zero_outside_the_limits():
  size = _ffi.lib().spml_dense_crf_votes_workspace_bytes
  assert size(1, 1) == (3 * 32 + 4) * 4 and size(144, 21) == 144 * (3 * 32 + 4) * 4
  assert size(4096, 64) == 4096 * (3 * 64 + 4) * 4 and size(7, 33) == 7 * (3 * 64 + 4) * 4
  assert size(7, 32) % 16 == 0 and size(7, 33) % 16 == 0      # rows are read as float4s
  assert [size(0, 21), size(-1, 21), size(4097, 21), size(12, 0), size(12, 65)] == [0] * 5


@pytest.mark.parametrize('name,api_function', PROGRAMS)
def test_the_three_programs_run_the_guards_in_the_shared_order(name, api_function, tmp_path):
  run_the_guards(name, api_function, tmp_path)
  prog = load_program(name)
  if name == 'inference_crf_msc':
    assert list(prog.SCALES) == [0.5, 0.75, 1, 1.25, 1.5]
  if name == 'inference':
    return
  # the six --crf_* options are read before any guard refuses the call
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  with pytest.raises(SystemExit) as info:
    prog.main(['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--data_list', 'synthetic', '--crf_iter_max',
               '2', '--crf_pos_xy_std', '1', '--crf_pos_w', '3', '--crf_bi_xy_std', '67', '--crf_bi_rgb_std', '3',
               '--crf_bi_w', '4'])
  assert str(info.value.code) == '--save_dir is required'


@pytest.mark.parametrize('shape', [(7, 5, 2), (33, 47, 5), (17, 129, 64)], ids=lambda s: '%dx%dx%d' % s)
def test_framework_segment_votes_on_the_cpu_is_the_reference_lines_bit_for_bit(shape):
  h, w, c = shape
  _, clu, topk = ref.votes_case(h, w, c, ref.SEED)
  want = ref.vote_map(clu, topk, c, (h, w))
  got = inference.framework_segment_votes(torch.from_numpy(clu), torch.from_numpy(topk), c, (h, w))
  assert got.dtype == torch.float32 and tuple(got.shape) == (c, h, w) and got.is_contiguous()
  assert np.array_equal(got.numpy(), want)
  assert np.abs(got.numpy().astype(np.float64).sum(0) - 1).max() <= 20 * 2.0 ** -25  # at most 20 rounded twentieths
  # an id map handed over as [h, w] is the same map
  assert torch.equal(inference.framework_segment_votes(torch.from_numpy(clu).view(h, w), torch.from_numpy(topk), c, (h, w)),
                     got)


def test_no_cpu_fallback():
  crf = DenseCRF(**dense_crf_ref.DEFAULTS)
  image, clu, topk = (torch.from_numpy(a) for a in ref.votes_case(16, 24, 2, 1))
  ws = torch.zeros(16, dtype=torch.uint8)
  with pytest.raises(_ffi.SpmlHipError):
    crf.refine_votes(image, clu, topk, 2)
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_votes(ws, clu, topk, 2, (16, 24))
  with pytest.raises(_ffi.SpmlHipError):
    inference.knn_votes_crf_refine(image, clu, topk, 2, crf)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.dense_crf_infer_votes(clu, topk, 2, (16, 24), 1, 3.0, 4.0, ws)


@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_votes_case_is_what_the_retrieval_hands_over(shape):
  h, w, c = shape
  image, clu, topk = ref.votes_case(h, w, c, ref.SEED)
  m = min(4, h) * min(6, w)
  assert image.dtype == np.uint8 and np.array_equal(image, dense_crf_ref.blocky(h, w, c, ref.SEED)[0])
  assert clu.dtype == np.int64 and clu.shape == (h * w,) and sorted(set(clu.tolist())) == list(range(m))
  assert topk.dtype == np.int64 and topk.shape == (m, 20)
  live = c - 1 if c > 2 else c
  assert topk.min() >= 0 and topk.max() < live
  counts = (topk[:, :, None] == np.arange(c)).sum(1)
  top = np.sort(counts, axis=1)
  assert (top[:, -1] >= 11).all() and (c == 1 or (top[:, -1] > top[:, -2]).all())    # no row has a tied maximum
  votes = ref.vote_map(clu, topk, c, (h, w))
  assert votes.dtype == np.float32 and votes.shape == (c, h, w)
  assert np.array_equal(votes[:, 0, 0], counts[clu[0]].astype(np.float32) / np.float32(20))
  if c > 2:
    assert not votes[c - 1].any()


@pytest.mark.parametrize('parameters', ['defaults', 'alternative'])
@pytest.mark.parametrize('shape', [(16, 24, 2), (33, 47, 5)], ids=lambda s: '%dx%dx%d' % s)
def test_label_caps_hold_on_the_two_smallest_comparing_shapes(shape, parameters):
  """The yardstick alone, so the caps are also checked without a GPU: the share of pixels under the margin stays under
  the cap, the marginals are distributions, and the CRF changes labels."""
  _, _, _, votes, want = ref.yardstick(shape, parameters)
  keep, left_out = ref.under_margin(want)
  print('%s %s: %.4f of the pixels under the margin' % (shape, parameters, left_out))
  assert ref.LABEL_CAP == 0.02 and left_out <= 0.02
  assert abs(want.sum(0) - 1).max() < 1e-12
  assert (want.argmax(0) != votes.argmax(0)).any(), 'the CRF changed no label'
