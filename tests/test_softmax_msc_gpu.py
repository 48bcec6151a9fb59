"""Multi-scale + flip softmax inference on the GPU: the view kernel of csrc/msc_inference.hip alone against the
reference's torch ops, then `predict_softmax_multiscale` against the fixture exec'd from the reference's own lines
(tests/golden/n8_softmax_msc.npz; tests/test_softmax_msc.py keeps that fixture honest on the CPU), its framework path
above 64 classes and the command-line entry point.  Measured figures: profiles/softmax_msc.md."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from spml_amd import _ffi, inference
from spml_amd.models.predictions import softmax_classifier as sc
from test_softmax_inference import make_classifier
from test_softmax_msc import LOGIT_BOUND, n8_case, prob_bound, restated_multiscale, restated_view_tail

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (ncls, (Hp, Wp), (rh, rw), (h, w), flip)
KERNEL_CASES = [
    (5, (32, 32), (22, 30), (44, 60), 1),
    (21, (51, 62), (51, 62), (41, 50), 0),
    (33, (40, 70), (37, 23), (19, 45), 1),        # down on one axis, up on the other, odd w
    (64, (9, 9), (1, 1), (7, 5), 1),              # a one-pixel source
    (1, (8, 8), (8, 8), (8, 8), 0),               # every output is exactly 1
    (8, (20, 130), (20, 130), (20, 130), 1)]      # scale 1: the weights are exactly 0 and 1


class StubEmbedder(torch.nn.Module):
  """Stand-in for the embedding network (as in test_softmax_inference_gpu.py): the fixture's 5x5 conv."""

  def __init__(self, conv):
    super().__init__()
    self.conv = conv

  def generate_embeddings(self, datas, targets=None, resize_as_input=False):
    return {'embedding': self.conv(datas['image'])}


def device_inputs(ncls, pad, seed):
  """Inputs made on the device: canvas of logit size, non-uniform small integer counts, a non-zero accumulator."""
  gen = torch.Generator(device=DEV).manual_seed(seed)
  canvas = 4.0 * torch.randn((ncls,) + pad, generator=gen, device=DEV)
  cnt_y = torch.randint(1, 4, (pad[0],), generator=gen, device=DEV).float()
  cnt_x = torch.randint(1, 5, (pad[1],), generator=gen, device=DEV).float()
  return canvas, cnt_y, cnt_x, gen


@functools.lru_cache(maxsize=None)
def kernel_case(index):
  """One kernel case, computed once: the kernel's result after one and after two calls, the reference's fp32 CPU ops
  (`restated_view_tail`, owned by the tests) and the fp64 restatement of the same ops, all from identical device-made inputs copied to the CPU."""
  ncls, pad, crop, out_hw, flip = KERNEL_CASES[index]
  canvas, cnt_y, cnt_x, gen = device_inputs(ncls, pad, 500 + index)
  start = torch.rand((ncls,) + out_hw, generator=gen, device=DEV)
  acc = start.clone()
  assert _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, crop, flip, acc) is acc
  once = acc.cpu()
  _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, crop, flip, acc)
  twice = acc.cpu()
  refs = {}
  for dtype in (torch.float32, torch.float64):
    ref = start.cpu().to(dtype)
    for _ in range(2):
      ref = ref + restated_view_tail(canvas.cpu().to(dtype), cnt_y.cpu().to(dtype), cnt_x.cpu().to(dtype), crop, flip,
                                     out_hw)
    refs[dtype] = ref
  return dict(start=start.cpu(), once=once, twice=twice, ref32=refs[torch.float32], ref64=refs[torch.float64])


@pytest.mark.parametrize('index', range(len(KERNEL_CASES)))
def test_view_kernel_matches_the_reference_ops(index):
  """Yardstick: the reference's ops in fp64.  Bound: 4 x the error of the reference's own fp32 CPU ops against that
  fp64 restatement on this very case -- both are fp32 chains of the same length; the factor covers a different `exp`, a
  different division and fma contraction.  Measured: profiles/softmax_msc.md."""
  case = kernel_case(index)
  ref_err = (case['ref32'].double() - case['ref64']).abs().max().item()
  err = (case['twice'].double() - case['ref64']).abs().max().item()
  print('view kernel %r: max error %.3e, fp32 CPU ops %.3e (both against fp64)' % (KERNEL_CASES[index], err, ref_err))
  assert torch.isfinite(case['twice']).all()
  assert not torch.equal(case['once'], case['start']) and not torch.equal(case['twice'], case['once'])
  assert err <= 4 * ref_err
  if KERNEL_CASES[index][0] == 1:                              # one class: every probability is exactly 1
    assert torch.equal(case['once'], case['start'] + 1.0) and torch.equal(case['twice'], case['start'] + 1.0 + 1.0)


@pytest.mark.parametrize('index', [0, 2])
def test_padding_does_not_leak(index):
  """NaN everywhere outside the rh x rw region: every output stays finite and is bit for bit what finite padding gives
  (an `i1` clamped to Hp - 1 instead of rh - 1 would read the padding at the bottom / right border)."""
  ncls, pad, (rh, rw), out_hw, flip = KERNEL_CASES[index]
  canvas, cnt_y, cnt_x, _ = device_inputs(ncls, pad, 600 + index)
  poisoned = torch.full_like(canvas, float('nan'))
  poisoned[:, :rh, :rw] = canvas[:, :rh, :rw]
  want = _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, (rh, rw), flip, torch.zeros((ncls,) + out_hw, device=DEV))
  got = _ffi.view_probs_accumulate(poisoned, cnt_y, cnt_x, (rh, rw), flip, torch.zeros((ncls,) + out_hw, device=DEV))
  assert torch.isfinite(got).all()
  assert torch.equal(got, want)


def ulp_distance(got, want):
  """max |got - want| in units of the fp32 spacing at `want`."""
  want = want.cpu()
  ulp = (torch.nextafter(want, torch.full_like(want, float('inf'))) - want).double()
  return ((got.cpu().double() - want.double()).abs() / ulp).max().item()


def test_constant_canvas_gives_one_softmax_vector():
  """A canvas constant over the pixels, counts that divide exactly (powers of two) and a 2 x up-sampling (weights 1/4 and
  3/4, logits that are multiples of 1/8: every product and sum of the interpolation is exact): every pixel is the softmax
  of one vector, within 2 ulp of a device `torch.softmax`."""
  ncls, pad, crop, out_hw = 5, (24, 40), (17, 29), (34, 58)
  gen = torch.Generator(device=DEV).manual_seed(7)
  logits = torch.randint(-24, 25, (ncls,), generator=gen, device=DEV).float() / 8.0
  cnt_y = 2.0 ** torch.randint(0, 3, (pad[0],), generator=gen, device=DEV).float()
  cnt_x = 2.0 ** torch.randint(0, 2, (pad[1],), generator=gen, device=DEV).float()
  canvas = (logits.view(-1, 1, 1) * cnt_y.view(1, -1, 1) * cnt_x.view(1, 1, -1)).contiguous()
  want = torch.softmax(logits, dim=0).view(-1, 1, 1).expand((ncls,) + out_hw)
  for flip in (0, 1):
    got = _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, crop, flip, torch.zeros((ncls,) + out_hw, device=DEV))
    assert torch.equal(got, got[:, :1, :1].expand_as(got))          # the same vector at every pixel
    dist = ulp_distance(got, want)
    print('constant canvas, flip %d: %.2f ulp from torch.softmax' % (flip, dist))
    assert dist <= 2.0


def test_scale_one_flip_is_the_mirrored_softmax():
  """Scale 1: the weights are exactly 0 and 1, so the result is `softmax(canvas / counts)` mirrored, within 2 ulp of the
  device's own ops."""
  ncls, pad, crop, out_hw, flip = KERNEL_CASES[5]
  assert pad == crop == out_hw and flip == 1
  canvas, cnt_y, cnt_x, _ = device_inputs(ncls, pad, 700)
  got = _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, crop, flip, torch.zeros((ncls,) + out_hw, device=DEV))
  want = torch.flip(torch.softmax(canvas / (cnt_y.view(-1, 1) * cnt_x.view(1, -1)), dim=0), dims=[2])
  dist = ulp_distance(got, want)
  print('scale 1, flipped: %.2f ulp from softmax(canvas / counts) mirrored' % dist)
  assert dist <= 2.0


def test_two_calls_are_bit_identical():
  ncls, pad, crop, out_hw, flip = KERNEL_CASES[2]
  canvas, cnt_y, cnt_x, gen = device_inputs(ncls, pad, 800)
  start = torch.rand((ncls,) + out_hw, generator=gen, device=DEV)
  first = _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, crop, flip, start.clone())
  was = _ffi.set_deterministic(True)
  try:
    second = _ffi.view_probs_accumulate(canvas, cnt_y, cnt_x, crop, flip, start.clone())
  finally:
    _ffi.set_deterministic(was)
  assert torch.equal(first, second)


def test_argument_errors():
  zeros = lambda *shape: torch.zeros(shape, device=DEV)
  with pytest.raises(_ffi.SpmlHipError):                                # 65 classes
    _ffi.view_probs_accumulate(zeros(65, 8, 8), zeros(8) + 1, zeros(8) + 1, (8, 8), 0, zeros(65, 4, 4))
  with pytest.raises(_ffi.SpmlHipError):                                # rh > Hp
    _ffi.view_probs_accumulate(zeros(3, 8, 8), zeros(8) + 1, zeros(8) + 1, (9, 8), 0, zeros(3, 4, 4))
  with pytest.raises(_ffi.SpmlHipError):                                # acc of another class count
    _ffi.view_probs_accumulate(zeros(3, 8, 8), zeros(8) + 1, zeros(8) + 1, (8, 8), 0, zeros(4, 4, 4))
  with pytest.raises(_ffi.SpmlHipError):                                # acc without the class axis
    _ffi.view_probs_accumulate(zeros(3, 8, 8), zeros(8) + 1, zeros(8) + 1, (8, 8), 0, zeros(4, 4))
  with pytest.raises(_ffi.SpmlHipError):                                # counts of the crop's size, not the plane's
    _ffi.view_probs_accumulate(zeros(3, 8, 8), zeros(6) + 1, zeros(8) + 1, (6, 8), 0, zeros(3, 4, 4))
  canvas = zeros(3, 8, 8)
  with pytest.raises(_ffi.SpmlHipError):                                # acc aliases canvas
    _ffi.view_probs_accumulate(canvas, zeros(8) + 1, zeros(8) + 1, (8, 8), 0, canvas)
  with pytest.raises(_ffi.SpmlHipError):                                # CPU tensors
    _ffi.view_probs_accumulate(torch.zeros(3, 8, 8), torch.ones(8), torch.ones(8), (8, 8), 0, torch.zeros(3, 4, 4))


def check_against(out, want_prob, want_pred, margin, bound, image_hw):
  prob = out['semantic_prob'].cpu()
  assert tuple(prob.shape) == tuple(want_prob.shape)
  err = (prob - want_prob).abs().max().item()
  sure = margin >= 2 * bound
  low = (~sure).float().mean().item()
  print('max|d prob| %.3e against B %.3e; %.2f %% of the pixels below the margin 2 B' % (err, bound, 100 * low))
  assert err <= bound
  assert low < 0.01
  pred = out['semantic_prediction'].cpu()
  assert pred.dtype == torch.int64 and tuple(pred.shape) == tuple(image_hw)
  assert torch.equal(pred[sure], want_pred.long()[sure])


@pytest.mark.parametrize('ci', [0, 1])
def test_multiscale_matches_reference_lines(ci):
  """max|d semantic_prob| <= B = 0.5 * n_views * 1e-4 * max|logit| (the project's logit bound per view, a softmax moves
  a probability by at most half of the logit error, the views' errors add up); labels exact on every pixel whose stored
  margin is at least 2 B, and fewer than 1 % of the pixels are outside that set."""
  g = load_golden('n8_softmax_msc')
  cfg, views, conv, state = n8_case(g, ci)
  model = make_classifier(cfg['c'], cfg['ncls'], state).to(DEV)
  out = inference.predict_softmax_multiscale(StubEmbedder(conv).to(DEV), model,
                                             [(v.to(DEV), hw, flip) for v, hw, flip in views], cfg['image'],
                                             cfg['crop'], cfg['stride'])
  assert out['head_path'] == sc.HIP_HEAD_PATH and out['combine_path'] == inference.HIP_VIEW_PROBS_PATH == 'hip_view_probs'
  t = 'c%d_' % ci
  check_against(out, g[t + 'semantic_prob'], g[t + 'semantic_pred'], g[t + 'margin'], prob_bound(g, ci), cfg['image'])


@pytest.mark.parametrize('c', [16, 48])
def test_hip_head_pads_its_hidden_channels(c):
  """2C = 32 or 96 hidden channels are no multiple of the convolution's 64-channel tile: the HIP head runs them padded
  with zero channels (fixture case 0 has C = 16).  Against the module's own framework ops on the device, at the project's
  logit bound 1e-4 * max|logit|."""
  gen = torch.Generator().manual_seed(c)
  torch.manual_seed(c)
  model = make_classifier(c, 7)
  with torch.no_grad():
    model.semantic_classifier[1].running_mean.copy_(0.05 * torch.randn(2 * c, generator=gen))
    model.semantic_classifier[1].running_var.copy_(0.02 + 0.05 * torch.rand(2 * c, generator=gen))
  model = model.to(DEV)
  emb = torch.randn(1, c, 19, 23, generator=gen).to(DEV)
  canvas = torch.zeros(1, 7, 25, 30, device=DEV)
  assert model.accumulate_logits(emb, canvas, 6, 7) == sc.HIP_HEAD_PATH
  with torch.no_grad():
    want = model._logits(emb)
  scale = want.abs().max().item()
  err = (canvas[..., 6:, 7:] - want).abs().max().item()
  print('padded head C=%d: max|d logit| %.3e = %.3e of max|logit| %.4f' % (c, err, err / scale, scale))
  assert err <= LOGIT_BOUND * scale
  assert canvas[..., :6, :].abs().max().item() == 0.0 and canvas[..., :7].abs().max().item() == 0.0


def test_more_than_64_classes_take_the_framework_tail():
  """A 70-class head: `combine_path` (and `head_path`) name the framework ops, and the result meets the bounds of the
  test above against the CPU restatement, with its own max|logit| and margins: |d prob| <= B, labels exact where the
  margin is at least 2 B, fewer than 1 % of the pixels below it.  The input is chosen as the fixture's generator chooses
  its seeds: a 70-way map has more close calls than the fixture's, so the last weight is x 10, and seeds are tried from 70
  until the low-margin share of the CPU restatement is under the cap with headroom (70: 1.17 %, 71: 0.90 %, 72: 0.63 %,
  28 classes win)."""
  gen = torch.Generator().manual_seed(72)
  torch.manual_seed(72)
  cfg = dict(c=16, ncls=70, image=(30, 37), crop=(24, 24), stride=(15, 15))
  conv = torch.nn.Conv2d(3, 16, 5, padding=2)
  model = make_classifier(16, 70)
  with torch.no_grad():
    model.semantic_classifier[1].running_mean.copy_(0.05 * torch.randn(32, generator=gen))
    model.semantic_classifier[1].running_var.copy_(0.02 + 0.05 * torch.rand(32, generator=gen))
    model.semantic_classifier[4].weight.mul_(10.0)
  base = torch.randn(1, 3, 6, 7, generator=gen)
  image = torch.nn.functional.interpolate(base, size=cfg['image'], mode='bilinear', align_corners=False)
  views = inference.flip_scale_views(image, [0.75, 1.25], True, cfg['crop'])
  stats = {}
  want, want_pred = restated_multiscale(views, conv, model.state_dict(), cfg, stats=stats)
  bound = 0.5 * len(views) * LOGIT_BOUND * stats['max_abs_logit']
  top2 = want.topk(2, dim=0).values
  out = inference.predict_softmax_multiscale(StubEmbedder(conv).to(DEV), model.to(DEV),
                                             [(v.to(DEV), hw, flip) for v, hw, flip in views], cfg['image'],
                                             cfg['crop'], cfg['stride'])
  assert out['head_path'] == sc.FRAMEWORK_HEAD_PATH
  assert out['combine_path'] == inference.FRAMEWORK_VIEW_PROBS_PATH == 'framework_view_probs'
  check_against(out, want, want_pred, top2[0] - top2[1], bound, cfg['image'])


def test_multiscale_entry_point_reads_a_classifier_snapshot(tmp_path, capsys):
  """pyscripts/inference/inference_softmax_msc.py on a snapshot written by pyscripts/train/train_classifier.py (stage 1
  -> stage 2 -> ten views per 129 x 129 image -> label maps + one JSON line), on the pattern of
  test_inference_entry_point_reads_a_classifier_snapshot."""
  import importlib.util
  import json
  import os
  from test_train_cli import ROOT, YAML, load_cli
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101')
          .replace('stride:\n    - 97\n    - 97', 'stride:\n    - 64\n    - 64').replace('image_size: 97', 'image_size: 129'))
  assert 'image_size: 129' in yaml and yaml.count('- 64') == 2
  stage1 = tmp_path / 'config_emb.yaml'
  stage1.write_text(yaml)
  snap1 = tmp_path / 'stage1'
  load_cli().main(['--snapshot_dir', str(snap1), '--cfg_path', str(stage1), '--data_list', 'synthetic'])

  def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod

  cfg = tmp_path / 'config_classifier.yaml'
  cfg.write_text(yaml.replace('prediction_types: segsort', 'prediction_types: softmax_classifier')
                 .replace('kmeans_iterations: 3', 'kmeans_iterations: 0')
                 .replace('pretrained: ""', 'pretrained: "%s"' % str(snap1 / 'model-1.pth')))
  snap2 = tmp_path / 'stage2'
  load('spml_train_classifier_cli', ('pyscripts', 'train', 'train_classifier.py')).main(
      ['--snapshot_dir', str(snap2), '--cfg_path', str(cfg), '--data_list', 'synthetic'])
  capsys.readouterr()
  save = tmp_path / 'results'
  load('spml_inference_softmax_msc_cli', ('pyscripts', 'inference', 'inference_softmax_msc.py')).main(
      ['--snapshot_dir', str(snap2), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic'])
  line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
  result = json.loads(line)
  assert result['images'] >= 1 and result['images_per_s'] > 0 and 0.0 <= result['mIoU'] <= 100.0
  assert result['views'] == 10
  assert result['head_path'] == sc.HIP_HEAD_PATH and result['combine_path'] == 'hip_view_probs'
  maps = sorted(os.listdir(str(save / 'semantic_gray')))
  assert len(maps) == result['images'] and maps[0].endswith('.npy')
  label = np.load(str(save / 'semantic_gray' / maps[0]))
  assert label.dtype == np.uint8 and label.shape == (129, 129) and label.max() < 21
