"""Tag-recipe kNN pseudo labels, the parts that need no GPU: the fixture (tests/golden/n11_pseudo_knn_msc.npz, exec'd from
pyscripts/inference/pseudo_inference_crf_msc.py:138-141 / :172-241 / :252-263 / :275 by tools/gen_golden.py) against a
plain-torch restatement of the tail, the conditions the fixture was picked for, the header's declarations, the limits
the workspace query states, the argument errors of `pseudo_labels_knn_multiscale` and the program's refusals.  The GPU
side is tests/test_pseudo_knn_msc_gpu.py."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_knn_msc import LOW_CAP, LOW_MARGIN, restated_view_tail

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [0.5, 1, 1.5, 2]
FLOOR = float(np.float32(0.15))        # np.maximum(<fp32 array>, 0.15) compares with 0.15 rounded to fp32 (:260)


def restated_tag_tail(total, num_views, tags, dtype=torch.float32):
  """pseudo_inference_crf_msc.py:254-263 and :275 in plain torch ops, in `dtype`, on the SUM of the views' vote maps
  `[ncls,h,w]`: the mean, per class the maximum over the image, the floor, 1 for the untagged classes, the division,
  the arg-max.  -> (prob, divisor, labels)."""
  mean = total.to(dtype) / torch.tensor(float(num_views), dtype=dtype)
  peak = mean.reshape(mean.shape[0], -1).max(dim=1).values
  divisor = torch.where(tags, torch.maximum(peak, torch.tensor(FLOOR, dtype=dtype)), torch.ones((), dtype=dtype))
  prob = mean / divisor.view(-1, 1, 1)
  return prob, divisor, torch.argmax(prob, 0)


def n11_case(g, ci):
  """(cfg dict, views) of fixture case `ci`; views = list of dicts with the padded `image` [1,3,Hp,Wp] (rebuilt from the
  stored image by `flip_scale_views`, the function the program feeds the model with), `crop_hw`, `flip`, and the
  reference's own `cluster_index` [rh * rw], per-segment `topk` [m, 20] and vote map `votes` [ncls,h,w], in the stored
  order: per scale the flipped view first."""
  from spml_amd import inference
  t = 'c%d_' % ci
  c, ncls, h, w, ch, cw, sh, sw, ky, kx = [int(v) for v in g[t + 'cfg']]
  cfg = dict(c=c, ncls=ncls, image=(h, w), crop=(ch, cw), stride=(sh, sw), grid=[ky, kx])
  assert g[t + 'scales'].tolist() == SCALES
  built = inference.flip_scale_views(g[t + 'image'], SCALES, True, (ch, cw))
  rows = g[t + 'views'].tolist()
  assert len(built) == len(rows) == 8
  views = []
  for vi, ((si, pad_h, pad_w, rh, rw, flip, m), (image, crop_hw, is_flip)) in enumerate(zip(rows, built)):
    assert tuple(image.shape) == (1, 3, pad_h, pad_w) and crop_hw == (rh, rw) and is_flip == bool(flip) and si == vi // 2
    clu, topk = g[t + 'cluster_index%d' % vi], g[t + 'topk%d' % vi]
    assert clu.dtype == torch.int16 and tuple(clu.shape) == (rh * rw,) and int(clu.max()) + 1 == m
    assert topk.dtype == torch.uint8 and tuple(topk.shape) == (m, 20) and int(topk.max()) < ncls
    views.append(dict(image=image, crop_hw=(rh, rw), flip=bool(flip), cluster_index=clu.long(), topk=topk.long(),
                      votes=g[t + 'votes%d' % vi]))
  return cfg, views


def restated_sum(views, cfg, dtype=torch.float32):
  """The vote maps of all views (tests/test_knn_msc.py's restatement of the per-view tail), added in view order."""
  total = None
  for v in views:
    votes = restated_view_tail(v['cluster_index'], v['topk'], cfg['ncls'], v['crop_hw'], v['flip'], cfg['image'], dtype)
    total = votes if total is None else total + votes
  return total


def sure_pixels(g, ci):
  t = 'c%d_' % ci
  return g[t + 'margin'] >= LOW_MARGIN * g[t + 'semantic_prob'].abs().max()


def ulp_distance(got, want):
  """max |got - want| in units of the fp32 spacing at `want`."""
  ulp = (torch.nextafter(want.abs(), torch.full_like(want, float('inf'))) - want.abs()).double()
  return ((got.double() - want.double()).abs() / ulp).max().item()


@pytest.mark.parametrize('ci', [0, 1])
def test_fixture_is_reproduced_by_plain_torch(ci):
  g = load_golden('n11_pseudo_knn_msc')
  cfg, views = n11_case(g, ci)
  t = 'c%d_' % ci
  ref, tags = g[t + 'semantic_prob'], g[t + 'label_tags']
  assert tuple(ref.shape) == (cfg['ncls'],) + cfg['image'] and ref.dtype == torch.float32 and tags.dtype == torch.bool
  assert g[t + 'semantic_pred'].dtype == torch.uint8 and tuple(g[t + 'semantic_pred'].shape) == cfg['image']
  for v in views:
    got = restated_view_tail(v['cluster_index'], v['topk'], cfg['ncls'], v['crop_hw'], v['flip'], cfg['image'])
    assert torch.equal(got, v['votes'])
  prob, divisor, pred = restated_tag_tail(restated_sum(views, cfg), len(views), tags)
  assert torch.equal(divisor, g[t + 'divisor'])                                  # bit-equal
  dist = ulp_distance(prob, ref)
  print('case %d: %d views, restated semantic_prob %.2f ulp from the stored one' % (ci, len(views), dist))
  assert dist <= 1.0
  sure = sure_pixels(g, ci)
  assert torch.equal(pred[sure], g[t + 'semantic_pred'].long()[sure])
  # the tags are the classes of the stored label map (:138-141)
  present = g[t + 'label_map'].unique()
  want_tags = torch.zeros(cfg['ncls'], dtype=torch.bool)
  want_tags[present[present < cfg['ncls']].long()] = True
  assert torch.equal(tags, want_tags)


def test_fixture_covers_the_cases_it_is_meant_to():
  g = load_golden('n11_pseudo_knn_msc')
  cfg, views = n11_case(g, 0)                                 # (a) image = crop: the scale-1 views are not padded
  assert cfg['image'] == cfg['crop'] and cfg['ncls'] == 5
  assert all(tuple(v['image'].shape[-2:]) == v['crop_hw'] == cfg['image'] for v in views[2:4])
  cfg, views = n11_case(g, 1)                                 # (b) odd width, a padded 0.5 view, several windows at scale 2
  (h, w), (ch, cw) = cfg['image'], cfg['crop']
  assert w % 2 == 1
  half, double = views[0], views[6]
  assert tuple(half['image'].shape[-2:]) == (ch, cw) != half['crop_hw'] and half['crop_hw'][0] < ch
  assert double['crop_hw'] == (2 * h, 2 * w)
  assert double['crop_hw'][0] > ch + cfg['stride'][0] and double['crop_hw'][1] > cw + cfg['stride'][1]
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'n11_pseudo_knn_msc.npz')) <= 600 * 1024


@pytest.mark.parametrize('ci', [0, 1])
def test_stored_margin_cap_and_normalisation_branches(ci):
  """The stored margin is the normalised map's own, at most 1 % of the pixels fall under it, and every branch of the
  normalisation is met by the stored data: a tagged class at or above the floor, a tagged class with votes under it, an
  untagged class that has votes and wins pixels; at least 3 classes win and the normalisation moves at least 5 % of the
  labels away from the plain arg-max of the mean."""
  g = load_golden('n11_pseudo_knn_msc')
  t = 'c%d_' % ci
  ref, mean, tags, pred = g[t + 'semantic_prob'], g[t + 'mean_prob'], g[t + 'label_tags'], g[t + 'semantic_pred'].long()
  top2 = ref.topk(2, dim=0).values
  assert torch.equal(top2[0] - top2[1], g[t + 'margin'])
  assert torch.equal(torch.argmax(ref, 0), pred)
  low = (~sure_pixels(g, ci)).float().mean().item()
  print('case %d: low-margin share %.4f' % (ci, low))
  assert low <= LOW_CAP
  peak = mean.reshape(mean.shape[0], -1).max(dim=1).values
  floor = torch.tensor(FLOOR)
  assert torch.equal(g[t + 'divisor'], torch.where(tags, torch.maximum(peak, floor), torch.ones(())))
  assert torch.equal(ref, mean / g[t + 'divisor'].view(-1, 1, 1))
  wins = torch.bincount(pred.reshape(-1), minlength=mean.shape[0])
  assert (tags & (peak >= floor)).any()
  assert (tags & (peak < floor) & (peak > 0)).any()
  assert ((~tags) & (peak > 0) & (wins > 0)).any()
  assert int((wins > 0).sum()) >= 3
  moved = (pred != torch.argmax(mean, 0)).float().mean().item()
  print('case %d: the normalisation moves %.3f of the labels' % (ci, moved))
  assert moved >= 0.05


def test_header_declares_both_entries_and_the_version_stays_8():
  from spml_amd import _ffi
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  assert int(re.search(r'#define SPML_ABI_VERSION (\d+)', hdr).group(1)) == 8 == _ffi.ABI_VERSION
  decl = re.search(r'int spml_tag_normalize_argmax_f32\(([^)]*)\);', hdr)
  assert decl is not None and 'spml_tag_normalize_argmax_f32' in _ffi.EXPORTS
  args = [' '.join(a.split()) for a in decl.group(1).split(',')]
  assert args == ['const float* acc', 'int ncls', 'int64_t n', 'int num_views', 'const unsigned char* tags', 'float floor',
                  'int64_t* labels', 'float* prob', 'float* divisor', 'void* ws', 'size_t ws_bytes', 'void* stream']
  res, argtypes = _ffi._SIGNATURES['spml_tag_normalize_argmax_f32']
  want = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
  assert res is ctypes.c_int and len(argtypes) == len(args)
  for a, ty in zip(args, argtypes):
    assert ty is (ctypes.c_void_p if '*' in a else want[a.split()[0]]), a
  size = re.search(r'size_t spml_tag_normalize_workspace_bytes\(([^)]*)\);', hdr)
  assert size is not None and [a.strip() for a in size.group(1).split(',')] == ['int ncls', 'int64_t n']
  assert 'spml_tag_normalize_workspace_bytes' in _ffi.EXPORTS
  assert _ffi._SIGNATURES['spml_tag_normalize_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64])
  assert 'pseudo_inference_crf_msc.py:252-263,275' in hdr      # the declaration cites the reference lines


def test_workspace_query_states_the_limits():
  """A host function: 1 .. 64 classes and at least one pixel are inside (a few floats per class), everything else gives
  0 bytes."""
  from spml_amd import _build, _ffi
  _build.build(verbose=False)
  lib = _ffi.lib()
  assert _ffi.MAX_TAG_NORMALIZE_CLASSES == 64
  assert lib.spml_tag_normalize_workspace_bytes(1, 1) == 4
  assert lib.spml_tag_normalize_workspace_bytes(21, 375 * 500) == 21 * 16 * 4       # at most 16 parts per class plane
  assert lib.spml_tag_normalize_workspace_bytes(64, 1 << 30) == 64 * 16 * 4
  for ncls, n in ((0, 100), (65, 100), (21, 0), (-1, 100), (21, -5), (21, (1 << 30) + 1)):
    assert lib.spml_tag_normalize_workspace_bytes(ncls, n) == 0


def test_pseudo_labels_knn_multiscale_argument_errors():
  from spml_amd import _ffi, inference
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.train import voc12_scribble_config
  model = segsort(voc12_scribble_config())
  conv = torch.nn.Conv2d(3, 16, 5, padding=2)
  bank, bank_lab = torch.zeros(30, 16), torch.zeros(30, dtype=torch.long)
  tags = torch.ones(5, dtype=torch.bool)
  call = lambda views, tags: inference.pseudo_labels_knn_multiscale(conv, model, views, (8, 8), (8, 8), (5, 5), bank,
                                                                    bank_lab, 5, tags)
  with pytest.raises(ValueError):
    call([], tags)
  views = inference.flip_scale_views(torch.zeros(1, 3, 8, 8), [1], True, (8, 8))
  with pytest.raises(_ffi.SpmlHipError):                      # CPU tags (and CPU views)
    call(views, tags)
  if torch.cuda.is_available():
    with pytest.raises(_ffi.SpmlHipError):                    # CPU views with device tags
      call(views, tags.cuda())
    with pytest.raises(_ffi.SpmlHipError):                    # device views with CPU tags
      call([(v.cuda(), hw, f) for v, hw, f in views], tags)
  with pytest.raises(_ffi.SpmlHipError):                      # the wrapper of the kernel refuses CPU tensors as well
    _ffi.tag_normalize_argmax(torch.zeros(5, 8, 8), 2, tags)


def test_framework_tail_is_the_restatement():
  """`framework_tag_normalize_argmax` (the path above 64 classes and the GPU tests' yardstick) on the CPU against the
  restatement kept here, on the sum of fixture case 1: bit for bit."""
  from spml_amd import inference
  g = load_golden('n11_pseudo_knn_msc')
  cfg, views = n11_case(g, 1)
  total, tags = restated_sum(views, cfg), g['c1_label_tags']
  before = total.clone()
  labels, prob, divisor = inference.framework_tag_normalize_argmax(total, len(views), tags, FLOOR, want_prob=True)
  want_prob, want_divisor, want_labels = restated_tag_tail(total, len(views), tags)
  assert torch.equal(prob, want_prob) and torch.equal(divisor, want_divisor) and torch.equal(labels, want_labels)
  assert torch.equal(total, before)
  assert inference.framework_tag_normalize_argmax(total, len(views), tags)[1] is None


def load_program():
  spec = importlib.util.spec_from_file_location(
      'spml_pseudo_inference_msc_cli', os.path.join(ROOT, 'pyscripts', 'inference', 'pseudo_inference_msc.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_program_refuses_a_file_list_and_a_machine_without_a_gpu(tmp_path):
  from test_train_cli import YAML
  prog = load_program()
  assert prog.SCALES == SCALES and prog.FLOOR == 0.15
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  common = ['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--save_dir', str(tmp_path / 'o'),
            '--semantic_memory_dir', str(tmp_path / 'bank'), '--kmeans_num_clusters', '3,5', '--label_divisor', '2048']
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'val.txt'])
  assert info.value.code not in (0, None) and 'ListDataset' in str(info.value.code)
  from spml_amd.config.default import config
  assert config.network.kmeans_num_clusters == [3, 5]         # the reference's own arguments are taken
  if torch.cuda.is_available():
    return
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'synthetic'])
  assert info.value.code not in (0, None) and 'no CPU fallback' in str(info.value.code)
