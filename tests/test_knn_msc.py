"""Multi-scale + flip kNN inference, the parts that need no GPU: the fixture (tests/golden/n9_knn_msc.npz, exec'd from
pyscripts/inference/inference_msc.py:157-226 / :237-242 by tools/gen_golden.py) against a plain-torch restatement of the
per-view tail, the low-margin cap, the argument errors of `predict_knn_multiscale`, the header's declarations and the
command-line entry point's refusals."""
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW_MARGIN = 2e-4        # labels are compared where top-1 minus top-2 >= LOW_MARGIN * max|semantic_prob| (the N7 rule,
LOW_CAP = 0.01           # tests/pseudo_label_ref.py) and at most this share of the pixels may fall below


def restated_votes(topk, ncls, dtype=torch.float32):
  """inference_msc.py:223-225 per SEGMENT: one-hot of the retrieved labels `[m, k]` over the classes, mean over k.  A
  label outside [0, ncls) matches no class (the reference's one_hot would fail on it)."""
  onehot = (topk.long().unsqueeze(-1) == torch.arange(ncls).view(1, 1, -1)).to(dtype)
  return torch.mean(onehot, dim=1)


def restated_view_tail(clu, topk, ncls, crop_hw, flip, out_hw, dtype=torch.float32):
  """inference_msc.py:223-234 in plain torch ops, in `dtype`: votes per segment, gathered by the segment id of every
  pixel, bilinear resize to `out_hw` (`F.interpolate`, the half-pixel mapping of `cv2.resize(..., INTER_LINEAR)`), flip of
  the RESULT.  -> vote map [ncls,h,w]."""
  rh, rw = crop_hw
  votes = restated_votes(topk, ncls, dtype)[clu.long().reshape(-1)].view(rh, rw, ncls).permute(2, 0, 1).unsqueeze(0)
  votes = F.interpolate(votes, size=tuple(out_hw), mode='bilinear', align_corners=False)[0]
  return torch.flip(votes, dims=[2]) if flip else votes


def n9_case(g, ci):
  """(cfg dict, views) of fixture case `ci`; views = list of dicts with the padded `image` [1,3,Hp,Wp] (rebuilt from the
  stored un-flipped scaled image: flip and zero-padding are exact), `crop_hw`, `flip`, and the reference's own
  `cluster_index` [rh * rw], per-segment `topk` [m, 20] and vote map `votes` [ncls,h,w], in the stored order: per scale
  the flipped view first."""
  t = 'c%d_' % ci
  c, ncls, h, w, ch, cw, sh, sw, ky, kx = [int(v) for v in g[t + 'cfg']]
  cfg = dict(c=c, ncls=ncls, image=(h, w), crop=(ch, cw), stride=(sh, sw), grid=[ky, kx])
  views = []
  for vi, (si, pad_h, pad_w, rh, rw, flip, m) in enumerate(g[t + 'views'].tolist()):
    scaled = g[t + 'scaled%d' % si]
    assert tuple(scaled.shape) == (1, 3, rh, rw) and pad_h == max(rh, ch) and pad_w == max(rw, cw)
    image = torch.zeros(1, 3, pad_h, pad_w)
    image[:, :, :rh, :rw] = torch.flip(scaled, dims=[3]) if flip else scaled
    clu, topk = g[t + 'cluster_index%d' % vi], g[t + 'topk%d' % vi]
    assert clu.dtype == torch.int16 and tuple(clu.shape) == (rh * rw,) and int(clu.max()) + 1 == m
    assert topk.dtype == torch.uint8 and tuple(topk.shape) == (m, 20) and int(topk.max()) < ncls
    views.append(dict(image=image, crop_hw=(rh, rw), flip=bool(flip), cluster_index=clu.long(), topk=topk.long(),
                      votes=g[t + 'votes%d' % vi]))
  return cfg, views


def sure_pixels(g, ci):
  t = 'c%d_' % ci
  return g[t + 'margin'] >= LOW_MARGIN * g[t + 'semantic_prob'].abs().max()


def restated_multiscale(views, cfg, dtype=torch.float32):
  """The tails of all views and inference_msc.py:237-242: sum in view order, mean, arg-max."""
  total = None
  for v in views:
    votes = restated_view_tail(v['cluster_index'], v['topk'], cfg['ncls'], v['crop_hw'], v['flip'], cfg['image'], dtype)
    total = votes if total is None else total + votes
  prob = total / len(views)
  return prob, torch.argmax(prob, 0)


@pytest.mark.parametrize('ci', [0, 1])
def test_fixture_is_reproduced_by_plain_torch(ci):
  g = load_golden('n9_knn_msc')
  cfg, views = n9_case(g, ci)
  t = 'c%d_' % ci
  ref = g[t + 'semantic_prob']
  assert tuple(ref.shape) == (cfg['ncls'],) + cfg['image'] and ref.dtype == torch.float32
  assert g[t + 'semantic_pred'].dtype == torch.uint8 and tuple(g[t + 'semantic_pred'].shape) == cfg['image']
  assert [v['flip'] for v in views] == [True, False] * (len(views) // 2)          # per scale the flipped view first
  for v in views:
    got = restated_view_tail(v['cluster_index'], v['topk'], cfg['ncls'], v['crop_hw'], v['flip'], cfg['image'])
    assert torch.equal(got, v['votes'])
    assert (got.sum(0) - 1.0).abs().max().item() <= 1e-5                        # every pixel's votes sum to one
  prob, pred = restated_multiscale(views, cfg)
  err = (prob - ref).abs().max().item()
  print('case %d: %d views, max prob %.4f, restatement error %.3e' % (ci, len(views), ref.max().item(), err))
  assert torch.allclose(prob, ref, rtol=1e-6, atol=1e-7)
  sure = sure_pixels(g, ci)
  assert torch.equal(pred[sure], g[t + 'semantic_pred'].long()[sure])


def test_fixture_covers_the_cases_it_is_meant_to():
  g = load_golden('n9_knn_msc')
  cfg, views = n9_case(g, 0)                                 # (a) one scale, a flip pair, no padding
  assert len(views) == 2 and all(tuple(v['image'].shape[-2:]) == v['crop_hw'] == cfg['image'] for v in views)
  cfg, views = n9_case(g, 1)                                 # (b) two scales, padding, two windows on an axis, odd width
  assert len(views) == 4 and cfg['image'][1] % 2 == 1
  (h, w), (ch, cw) = cfg['image'], cfg['crop']
  up, down = views[0], views[2]
  assert up['crop_hw'][0] < h and up['crop_hw'][1] < w and down['crop_hw'][0] > h and down['crop_hw'][1] > w
  assert tuple(up['image'].shape[-2:]) != up['crop_hw']      # a padded view ...
  assert ch < up['image'].shape[-1] <= ch + cfg['stride'][1]  # ... with two windows along x
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'n9_knn_msc.npz')) < 600 * 1024


@pytest.mark.parametrize('ci', [0, 1])
def test_stored_margin_is_the_means_own_and_the_cap_holds(ci):
  g = load_golden('n9_knn_msc')
  t = 'c%d_' % ci
  ref = g[t + 'semantic_prob']
  top2 = ref.topk(2, dim=0).values
  assert torch.equal(top2[0] - top2[1], g[t + 'margin'])
  assert torch.equal(torch.argmax(ref, 0), g[t + 'semantic_pred'].long())
  low = (~sure_pixels(g, ci)).float().mean().item()
  print('case %d: low-margin share %.4f' % (ci, low))
  assert low <= LOW_CAP
  assert g[t + 'semantic_pred'].unique().numel() >= 3


def test_predict_knn_multiscale_argument_errors():
  from spml_amd import _ffi, inference
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.train import voc12_scribble_config
  model = segsort(voc12_scribble_config())
  conv = torch.nn.Conv2d(3, 16, 5, padding=2)
  bank, bank_lab = torch.zeros(30, 16), torch.zeros(30, dtype=torch.long)
  with pytest.raises(ValueError):
    inference.predict_knn_multiscale(conv, model, [], (8, 8), (8, 8), (5, 5), bank, bank_lab, 5)
  views = inference.flip_scale_views(torch.zeros(1, 3, 8, 8), [1], True, (8, 8))
  with pytest.raises(_ffi.SpmlHipError):                      # CPU tensors
    inference.predict_knn_multiscale(conv, model, views, (8, 8), (8, 8), (5, 5), bank, bank_lab, 5)
  with pytest.raises(ValueError):                             # a 3-D view
    inference.predict_knn_multiscale(conv, model, [(torch.zeros(3, 8, 8), (8, 8), False)], (8, 8), (8, 8), (5, 5), bank,
                                     bank_lab, 5)


def test_header_declares_both_entries_and_the_version_stays_8():
  from spml_amd import _ffi
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  assert int(re.search(r'#define SPML_ABI_VERSION (\d+)', hdr).group(1)) == 8 == _ffi.ABI_VERSION
  decl = re.search(r'int spml_view_votes_accumulate_f32\(([^)]*)\);', hdr)
  assert decl is not None and 'spml_view_votes_accumulate_f32' in _ffi.EXPORTS
  args = [' '.join(a.split()) for a in decl.group(1).split(',')]
  assert args == ['const int64_t* clu', 'int rh', 'int rw', 'const int64_t* topk', 'int m', 'int k', 'int ncls',
                  'int flip', 'int h', 'int w', 'float* acc', 'void* ws', 'size_t ws_bytes', 'void* stream']
  res, argtypes = _ffi._SIGNATURES['spml_view_votes_accumulate_f32']
  assert len(argtypes) == len(args)
  import ctypes
  want = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}
  for a, ty in zip(args, argtypes):
    assert ty is (ctypes.c_void_p if '*' in a else want[a.split()[0]]), a
  assert res is ctypes.c_int
  size = re.search(r'size_t spml_view_votes_workspace_bytes\(([^)]*)\);', hdr)
  assert size is not None and [a.strip() for a in size.group(1).split(',')] == ['int m', 'int ncls']
  assert _ffi._SIGNATURES['spml_view_votes_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
  assert 'inference_msc.py:223-234' in hdr                    # the declaration cites the reference lines


def test_workspace_query_states_the_limits():
  """A host function: 64 classes and 4096 segments are inside, the next value of either is outside (0 bytes); the
  largest k-means here gives 144 segments."""
  from spml_amd import _build, _ffi
  _build.build(verbose=False)
  lib = _ffi.lib()
  assert _ffi.MAX_VIEW_VOTES_CLASSES == 64 and _ffi.MAX_VIEW_VOTES_SEGMENTS >= 144
  top = _ffi.MAX_VIEW_VOTES_SEGMENTS
  assert lib.spml_view_votes_workspace_bytes(144, 21) == 144 * 24 * 4       # rows padded to 8, 16, 24, 32 or 64 classes
  assert lib.spml_view_votes_workspace_bytes(top, 64) == top * 64 * 4
  assert lib.spml_view_votes_workspace_bytes(1, 1) == 8 * 4
  for m, ncls in ((top + 1, 21), (144, 65), (0, 21), (144, 0), (-1, 21)):
    assert lib.spml_view_votes_workspace_bytes(m, ncls) == 0


def load_program():
  spec = importlib.util.spec_from_file_location('spml_inference_msc_cli',
                                                os.path.join(ROOT, 'pyscripts', 'inference', 'inference_msc.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_program_refuses_a_file_list_and_a_machine_without_a_gpu(tmp_path):
  from test_train_cli import YAML
  prog = load_program()
  assert prog.SCALES == [0.5, 0.75, 1, 1.25, 1.5]
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
