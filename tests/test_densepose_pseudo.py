"""The DensePose pseudo labels as far as they run without a GPU: the fp64 restatement of
tests/densepose_pseudo_ref.py against the golden of the reference's own lines, the framework route on the CPU, the
path-name table at the limits, the new C-ABI symbols, the program's guards, the refusals of CPU tensors and the seeded
test inputs."""
import os
import re

import numpy as np
import pytest
import torch

import densepose_pseudo_ref as ref
from spml_amd import _ffi, inference, inference_cli
from test_inference_cli import load_program, test_every_program_runs_the_guards_in_one_order as run_the_guards
from test_train_cli import ROOT, YAML

# fp32 rounding of values in [0, 1]: the reference's row passes three fp32 divisions and a sum of at most 15 terms, the
# resampled map four products and three sums more -- about twenty roundings of 2^-24 each
F32_CHAIN = 20 * 2.0 ** -24
# the walk: seven fp32 products with 35-term sums over a column-stochastic matrix, values in [0, 1]
WALK_CHAIN = 7 * 35 * 2.0 ** -24


@pytest.mark.parametrize('ci', [0, 1])
def test_restatement_reproduces_the_golden(ci):
  g = ref.golden_cases()[ci]
  counts, probs, acc = ref.segment_cam(g['nn_index'], g['nn_value'], g['proto_label'], ref.THRESHOLD, g['cluster_index'],
                                       g['num_segments'], g['ncls'], g['half_hw'], g['out_hw'])
  # the one-hot rows the reference's retrieval returned are the classes the restatement reads off the stored indices
  classes = ref.pixel_classes(g['nn_index'], g['nn_value'], g['proto_label'], ref.THRESHOLD, g['ncls'])
  assert (classes >= 0).all() and np.array_equal(np.eye(g['ncls'], dtype=np.uint8)[classes], g['s_tags'])
  assert counts.sum() == classes.size and (counts.sum(1) > 0).all()        # dense ids: no empty segment in the golden
  assert np.abs(probs - g['s_probs']).max() <= F32_CHAIN
  assert np.abs(acc - g['semantic_probs']).max() <= F32_CHAIN
  cam = ref.normalized_cam(acc, g['tags'])
  assert not np.isnan(cam).any() and np.abs(cam - g['cam_full_arr']).max() <= 2 * F32_CHAIN
  assert np.array_equal(cam.reshape(g['ncls'], -1).max(1) == 1.0, g['tags'])
  cam_rw = ref.walked(g['cam_full_arr'], g['trans'], int(g['cfg'][7]))
  assert np.abs(cam_rw - g['cam_rw']).max() <= WALK_CHAIN
  assert np.abs(cam_rw - g['cam_full_arr']).max() > 1e-3                   # the walk moves the maps


def test_golden_geometry():
  a, b = ref.golden_cases()
  assert (a['half_hw'], a['out_hw']) == ((20, 28), (5, 7)) and (b['half_hw'], b['out_hw']) == ((21, 30), (5, 7))
  for g in (a, b):
    assert g['ncls'] == 15 and g['tags'].sum() == 3 and g['trans'].shape == (35, 35)
    lab = g['semantic_label']
    assert (lab == 255).any() and (lab == 254).any() and 0.05 < (lab < 15).mean() < 0.15
    assert os.path.getsize(ref.GOLDEN) < 600 * 1024


@pytest.mark.parametrize('ci', [0, 1])
def test_framework_route_on_the_cpu_equals_the_golden(ci):
  g = ref.golden_cases()[ci]
  t = {k: torch.from_numpy(np.array(g[k])) for k in ('nn_index', 'nn_value', 'proto_label', 'cluster_index')}
  got = inference.framework_densepose_segment_cam(t['nn_index'], t['nn_value'], t['proto_label'], ref.THRESHOLD,
                                                  t['cluster_index'], g['ncls'], g['half_hw'], g['out_hw'])
  assert got.dtype == torch.float32 and tuple(got.shape) == (g['ncls'],) + g['out_hw']
  assert np.array_equal(got.numpy(), g['semantic_probs'])                  # the reference's own ops: bit for bit


def test_framework_route_pins_what_the_reference_leaves_undefined():
  """A label above `ncls` is no class and a row without a counted pixel is zeros, as the kernel has it."""
  shape = ref.SHAPES[2]
  half_hw, out_hw, s, ncls = shape
  c, counts, probs, acc = ref.yardstick(shape)
  assert (counts.sum(1) == 0).any() and (c['proto_label'] == 254).any()
  t = {k: torch.from_numpy(np.array(v)) for k, v in c.items()}
  got = inference.framework_densepose_segment_cam(t['nn_index'], t['nn_value'], t['proto_label'], ref.THRESHOLD,
                                                  t['cluster_index'], ncls, half_hw, out_hw)
  assert not torch.isnan(got).any() and np.abs(got.numpy() - acc).max() <= F32_CHAIN


@pytest.mark.parametrize('shape', ref.SHAPES, ids=ref.shape_id)
def test_seeded_cases_have_classless_pixels_and_empty_segments(shape):
  (h2, w2), (oh, ow), s, ncls = shape
  for seed in ref.SEEDS:
    c, counts, probs, acc = ref.yardstick(shape, seed)
    n = h2 * w2
    assert all(c[k].shape == (n,) for k in ('nn_index', 'nn_value', 'cluster_index'))
    assert c['cluster_index'].min() >= 0 and c['cluster_index'].max() < s and c['nn_index'].max() < len(c['proto_label'])
    classes = ref.pixel_classes(c['nn_index'], c['nn_value'], c['proto_label'], ref.THRESHOLD, ncls)
    assert (classes < 0).any() and (classes >= 0).any()
    pixels = np.bincount(c['cluster_index'], minlength=s)
    assert s == 1 or (pixels == 0).any()                     # a segment id without a pixel
    assert s == 1 or ((pixels > 0) & (counts.sum(1) == 0)).any()          # a segment without a tagged pixel
    assert counts.sum() == (classes >= 0).sum() and acc.shape == (ncls, oh, ow)
    rows = probs.sum(1)
    assert np.all((np.abs(rows - 1) < 1e-12) | (rows == 0)) and not np.isnan(acc).any()
    assert acc.min() >= 0 and acc.max() <= 1 + 1e-12 and acc.max() > 0


def test_path_name_table_at_the_limits():
  name = _ffi.segment_tag_cam_path_name
  assert name(16, 1, 15) == 'lds_table' and name(630, 37, 15) == 'lds_table'
  assert name(512, 300, 21) == 'lds_table' and name(561, 64, 64) == 'lds_table'
  assert name(561, 128, 64) == 'lds_table' and name(561, 129, 64) == 'global_table'       # 8192 entries and one row more
  assert name(1551, 4096, 15) == 'global_table' and name(1551, 4096, 64) == 'global_table'
  assert name(561, 64, 65) == 'unsupported' and name(1551, 4097, 15) == 'unsupported'
  assert name(2 ** 31, 64, 15) == 'unsupported' and name(2 ** 31 - 1, 64, 15) == 'lds_table'
  assert name(0, 64, 15) == 'invalid' and name(16, 0, 15) == 'invalid' and name(16, 1, 0) == 'invalid'
  assert (_ffi.MAX_SEGMENT_TAG_CAM_CLASSES, _ffi.MAX_SEGMENT_TAG_CAM_SEGMENTS) == (64, 4096)
  size = _ffi.lib().spml_segment_tag_cam_workspace_bytes
  assert size(4096, 64) == 4096 * 64 * 8 and size(1, 1) == 8
  assert size(4097, 64) == 0 and size(4096, 65) == 0 and size(0, 15) == 0
  # every case of the GPU tests names its route
  routes = [name(h2 * w2, s, ncls) for (h2, w2), _, s, ncls in ref.SHAPES]
  assert routes == ['lds_table'] * 5 + ['global_table']


def test_header_declares_the_symbols_and_the_ffi_lists_them():
  header = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  declaration = re.search(r'^int spml_segment_tag_cam_f32\(([^;]*)\);', header, flags=re.M)
  assert declaration is not None
  arguments = [a.strip() for a in declaration.group(1).replace('\n', ' ').split(',')]
  assert arguments == ['const int64_t* nn_index', 'const float* nn_value', 'const int64_t* proto_label', 'int64_t M',
                       'float threshold', 'const int64_t* cluster_index', 'int S', 'int ncls', 'int h2', 'int w2',
                       'int oh', 'int ow', 'float* acc', 'int* counts', 'float* probs', 'void* ws', 'size_t ws_bytes',
                       'void* stream']
  assert 'pseudo_denseposerw_crf.py:159-182' in header and 'counts nowhere' in header
  for symbol in ('spml_segment_tag_cam_f32', 'spml_segment_tag_cam_workspace_bytes', 'spml_segment_tag_cam_path_name'):
    assert symbol in _ffi.EXPORTS and hasattr(_ffi.lib(), symbol)
  assert len(_ffi._SIGNATURES['spml_segment_tag_cam_f32'][1]) == len(arguments)


def test_program_runs_the_guards_in_the_shared_order(tmp_path):
  run_the_guards('pseudo_denseposerw_crf', 'pseudo_labels_densepose_crf', tmp_path)
  prog = load_program('pseudo_denseposerw_crf')
  assert prog.WALK_STEPS == 6 and prog.BACKGROUND_THRESHOLD is None
  # the --crf_* options, --kmeans_num_clusters and --label_divisor are read before any guard refuses the call
  from spml_amd.config.default import config
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  with pytest.raises(SystemExit) as info:
    prog.main(['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--data_list', 'synthetic', '--crf_iter_max',
               '2', '--crf_pos_xy_std', '1', '--crf_pos_w', '3', '--crf_bi_xy_std', '67', '--crf_bi_rgb_std', '3',
               '--crf_bi_w', '4', '--kmeans_num_clusters', '3,4', '--label_divisor', '1024'])
  assert str(info.value.code) == '--save_dir is required'
  assert list(config.network.kmeans_num_clusters) == [3, 4] and config.network.label_divisor == 1024


def test_the_program_builds_the_densepose_embedder():
  from spml_amd.models.embeddings import resnet_deeplab, resnet_pspnet, resnet_pspnet_densepose
  plain, densepose = inference_cli.embedding_makers(), inference_cli.embedding_makers(densepose=True)
  assert plain == {'panoptic_pspnet_101': resnet_pspnet.resnet_101_pspnet,
                   'panoptic_deeplab_101': resnet_deeplab.resnet_101_deeplab}
  assert densepose == {'panoptic_pspnet_101': resnet_pspnet_densepose.resnet_101_pspnet,
                       'panoptic_deeplab_101': resnet_deeplab.resnet_101_deeplab}
  source = open(os.path.join(ROOT, 'pyscripts', 'inference', 'pseudo_denseposerw_crf.py')).read()
  assert 'densepose=True' in source


def test_no_cpu_fallback():
  c = {k: torch.from_numpy(np.array(v)) for k, v in ref.case(ref.SHAPES[1]).items()}
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    _ffi.segment_tag_cam(c['nn_index'], c['nn_value'], c['proto_label'], -1.0, c['cluster_index'], 5, 1, (8, 8), (2, 2))
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    inference.densepose_segment_cam({}, torch.zeros(15, dtype=torch.bool), (8, 8), (2, 2), 15, 2048)
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    inference.pseudo_labels_densepose_crf(None, torch.zeros(1, 3, 16, 16), (16, 16), torch.zeros(16, 16),
                                          torch.zeros(16, 16), None, torch.zeros(16, 16, 3, dtype=torch.uint8), None)
