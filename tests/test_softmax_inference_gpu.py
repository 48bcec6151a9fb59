"""Full-resolution softmax inference on the GPU: the four kernels of csrc/softmax_head.hip one by one against torch,
then `predict_softmax_full_resolution` against the fixture exec'd from the reference's own lines
(tests/golden/n6_softmax_inference.npz; tests/test_softmax_inference.py keeps that fixture honest on the CPU)."""
import numpy as np
import pytest
import torch

from bn_act_ref import decode_hl8
from conftest import load_golden
from spml_amd import _ffi, inference
from spml_amd.models.predictions import softmax_classifier as sc
from spml_amd.utils.general import metrics
from test_softmax_inference import LOW_MARGIN, make_classifier, n6_case, restated_inference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


class StubEmbedder(torch.nn.Module):
  """Stand-in for the embedding network (the TinyEmbedder pattern of test_inference_gpu.py): the fixture's 5x5 conv."""

  def __init__(self, conv):
    super().__init__()
    self.conv = conv

  def generate_embeddings(self, datas, targets=None, resize_as_input=False):
    return {'embedding': self.conv(datas['image'])}


@pytest.mark.parametrize('n,c,h,w', [(2, 32, 7, 11), (1, 64, 9, 15), (3, 16, 8, 8), (1, 208, 5, 13)])
def test_unit_hl8_round_trip(n, c, h, w):
  """h + l against x / |x| in float64 at 2^-22 relative, the width of the format (two 11-bit significands).  The low
  half is an f16 of the scaled value (S = 2^13), whose smallest step is 2^-24: an element below 2^-16 of the unit
  row cannot keep 22 relative bits, so the format's absolute floor 2^-25 / S = 2^-38 is added to the bound."""
  gen = torch.Generator().manual_seed(100 + c)
  x = torch.randn(n, c, h, w, generator=gen) * (0.1 + 3.0 * torch.rand(n, 1, h, w, generator=gen))
  x[0, :, 1, 2] = 0.0                                              # a zero-norm pixel: zeros, not NaN (outside the contract)
  got = _ffi.unit_hl8_from_nchw(x.to(DEV))
  assert got.rows == n * h * w and got.channels == c and float(got.bound.item()) == 1.0
  dec = decode_hl8(got).cpu().view(n, h, w, c).permute(0, 3, 1, 2)
  xd = x.double()
  want = xd / xd.norm(dim=1, keepdim=True)
  assert torch.equal(dec[0, :, 1, 2], torch.zeros(c, dtype=torch.float64))
  want[0, :, 1, 2] = 0.0
  err = (dec - want).abs()
  rel = (err / want.abs().clamp_min(2.0 ** -16)).max().item()
  print('unit hl8 C=%d: max relative error %.3e (2^-22 = %.3e)' % (c, rel, 2.0 ** -22))
  assert bool((err <= 2.0 ** -22 * want.abs() + 2.0 ** -38).all())
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.unit_hl8_from_nchw(torch.zeros(1, 24, 4, 4, device=DEV))      # C % 16 != 0


@pytest.mark.parametrize('ncls,ch,h,w', [(21, 128, 13, 17), (40, 64, 9, 33), (64, 32, 6, 7), (5, 64, 31, 3),
                                         (7, 160, 5, 9),           # more than 128 hidden channels: no tile fetched ahead
                                         (21, 64, 300, 301),       # more tiles than waves in flight: several per wave
                                         (33, 64, 270, 263)])      # ... with two class tiles
def test_class_head_accumulate_is_exact_on_integers(ncls, ch, h, w):
  """Small integers: every product and partial sum is exact in fp32, so the result is bit for bit the integer one
  whatever the summation order.  Asymmetric operands, a window that ends at the canvas's bottom-right corner."""
  gen = torch.Generator().manual_seed(ncls + ch)
  hidden = torch.randint(-4, 5, (h * w, ch), generator=gen)
  weight = torch.randint(-3, 4, (ncls, ch), generator=gen)
  bias = torch.randint(-9, 10, (ncls,), generator=gen)
  hp, wp = h + 7, w + 13
  canvas = torch.randint(-50, 51, (ncls, hp, wp), generator=gen)
  want = canvas.clone()
  want[:, 7:, 13:] += (hidden @ weight.t() + bias).t().reshape(ncls, h, w)
  dev_canvas = canvas.float().to(DEV)
  _ffi.class_head_accumulate(hidden.float().to(DEV), weight.float().to(DEV), bias.float().to(DEV), dev_canvas, 7, 13, h, w)
  assert torch.equal(dev_canvas.cpu(), want.float())


def test_class_head_accumulate_windows_on_every_border_and_overlapping():
  """Random operands, five windows: the four corners of the canvas (every border touched) and one in the middle over
  what the others wrote.  Bound: an fp32 fma chain of Ch terms plus the bias and the canvas additions is within
  (Ch + 8) * 2^-24 of the sum of the magnitudes (the standard running-error bound), per element."""
  gen = torch.Generator().manual_seed(77)
  ncls, ch, h, w, hp, wp = 21, 128, 15, 18, 24, 28
  weight = torch.randn(ncls, ch, generator=gen) * 0.2
  bias = torch.randn(ncls, generator=gen)
  canvas = torch.zeros(ncls, hp, wp, device=DEV)
  want = torch.zeros(ncls, hp, wp, dtype=torch.float64)
  mags = torch.zeros(ncls, hp, wp, dtype=torch.float64)
  for sh, sw in [(0, 0), (hp - h, wp - w), (0, wp - w), (hp - h, 0), (5, 6)]:
    hidden = torch.relu(torch.randn(h * w, ch, generator=gen))
    _ffi.class_head_accumulate(hidden.to(DEV), weight.to(DEV), bias.to(DEV), canvas, sh, sw, h, w)
    want[:, sh:sh + h, sw:sw + w] += (hidden.double() @ weight.double().t() + bias.double()).t().reshape(ncls, h, w)
    mags[:, sh:sh + h, sw:sw + w] += (hidden.double().abs() @ weight.double().abs().t() +
                                      bias.double().abs()).t().reshape(ncls, h, w)
  err = (canvas.cpu().double() - want).abs()
  print('class head: max error %.3e, max bound %.3e' % (err.max().item(), ((ch + 8) * 2.0 ** -24 * mags).max().item()))
  assert bool((err <= (ch + 8) * 2.0 ** -24 * mags).all())
  with pytest.raises(_ffi.SpmlHipError):                               # window outside the canvas
    _ffi.class_head_accumulate(hidden.to(DEV), weight.to(DEV), bias.to(DEV), canvas, hp - h + 1, 0, h, w)
  with pytest.raises(_ffi.SpmlHipError):                               # Ch % 32 != 0
    _ffi.class_head_accumulate(torch.zeros(4, 48, device=DEV), torch.zeros(3, 48, device=DEV),
                               torch.zeros(3, device=DEV), torch.zeros(3, 2, 2, device=DEV), 0, 0, 2, 2)


def test_argmax_channels_ties_and_region():
  gen = torch.Generator().manual_seed(5)
  canvas = torch.randint(0, 3, (7, 19, 23), generator=gen).float()        # three values over seven classes: ties everywhere
  got = _ffi.argmax_channels(canvas.to(DEV), 17, 20)
  top = canvas.max(0).values
  lowest = torch.where(canvas == top, torch.arange(7).view(7, 1, 1), torch.tensor(99)).min(0).values
  assert got.dtype == torch.int64 and tuple(got.shape) == (17, 20)
  assert torch.equal(got.cpu(), lowest[:17, :20])
  assert torch.equal(got.cpu(), torch.argmax(canvas, 0)[:17, :20])
  canvas[4, 2, 3] = float('nan')                                           # outside the contract: as torch.argmax, no fault
  assert int(_ffi.argmax_channels(canvas.to(DEV), 19, 23)[2, 3]) == 4 == int(torch.argmax(canvas, 0)[2, 3])


def test_iou_counts_match_the_reference_vectors_and_accumulate():
  g = load_golden('n6_softmax_inference')
  ncls = int(g['iou_num_classes'])
  pred, target = g['iou_pred'].to(DEV), g['iou_target'].to(DEV)
  counts = metrics.iou_stats(pred, target, ncls)
  assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), g['iou_counts'])
  again = metrics.iou_stats(pred, target, ncls, counts)
  assert again is counts and torch.equal(counts.cpu(), 2 * g['iou_counts'])
  big = torch.randint(0, 21, (513 * 513,), generator=torch.Generator().manual_seed(1))
  big_t = torch.where(big % 7 == 0, torch.tensor(255), (big * 5 + 3) % 21)
  c2 = metrics.iou_stats(big.to(DEV), big_t.to(DEV), 21).cpu()
  valid = big_t < 21
  assert torch.equal(c2[0], torch.bincount(big_t[valid], minlength=21))
  assert torch.equal(c2[1], torch.bincount(big[valid], minlength=21))
  assert torch.equal(c2[2], torch.bincount(big_t[valid & (big == big_t)], minlength=21))


def run_case(ci, model=None):
  g = load_golden('n6_softmax_inference')
  cfg, image, conv, state = n6_case(g, ci)
  if model is None:
    model = make_classifier(cfg['c'], cfg['ncls'], state).to(DEV)
  out = inference.predict_softmax_full_resolution(StubEmbedder(conv).to(DEV), model, image.to(DEV), cfg['valid'],
                                                  cfg['crop'], cfg['stride'])
  return g, cfg, out, model


@pytest.mark.parametrize('ci', [0, 1])
def test_full_resolution_softmax_matches_reference_lines(ci):
  """max|d semantic_logit| <= 1e-4 * max|logit_ref| (the project's parity bound); labels exact on every valid pixel
  whose stored margin is at least 2e-4 * max|logit| (a flip needs both competitors to move by the full bound), and
  fewer than 1 % of the valid pixels are outside that set."""
  g, cfg, out, _ = run_case(ci)
  t = 'c%d_' % ci
  ref = g[t + 'semantic_logit']
  scale = ref.abs().max().item()
  assert out['head_path'] == sc.HIP_HEAD_PATH
  assert tuple(out['semantic_logit'].shape) == tuple(ref.shape)
  err = (out['semantic_logit'].cpu() - ref).abs().max().item()
  print('case %d: max|d logit| %.3e = %.3e of max|logit| %.4f' % (ci, err, err / scale, scale))
  assert err <= 1e-4 * scale
  sure = g[t + 'margin'] >= LOW_MARGIN * scale
  assert (~sure).float().mean().item() < 0.01
  pred = out['semantic_prediction'].cpu()
  assert pred.dtype == torch.int64 and tuple(pred.shape) == cfg['valid']
  assert torch.equal(pred[sure], g[t + 'semantic_pred'].long()[sure])


def test_unsupported_channel_count_takes_the_framework_path_with_the_same_result():
  gen = torch.Generator().manual_seed(24)
  torch.manual_seed(24)
  cfg = dict(c=24, ncls=5, pad=(40, 52), valid=(33, 52), crop=(32, 32), stride=(20, 20))
  conv = torch.nn.Conv2d(3, 24, 5, padding=2)
  model = make_classifier(24, 5)
  with torch.no_grad():
    model.semantic_classifier[1].running_mean.copy_(0.05 * torch.randn(48, generator=gen))
    model.semantic_classifier[1].running_var.copy_(0.02 + 0.05 * torch.rand(48, generator=gen))
  image = torch.randn(1, 3, 40, 52, generator=gen)
  want, want_pred = restated_inference(image, conv, model.state_dict(), cfg)
  out = inference.predict_softmax_full_resolution(StubEmbedder(conv).to(DEV), model.to(DEV), image.to(DEV),
                                                  cfg['valid'], cfg['crop'], cfg['stride'])
  assert out['head_path'] == sc.FRAMEWORK_HEAD_PATH
  scale = want.abs().max().item()
  assert (out['semantic_logit'].cpu() - want).abs().max().item() <= 1e-4 * scale
  top2 = want[0, :, :33, :52].topk(2, dim=0).values
  sure = (top2[0] - top2[1]) >= LOW_MARGIN * scale
  assert torch.equal(out['semantic_prediction'].cpu()[sure], want_pred[sure])


def test_stale_cache_guard():
  """The folded operands live on the module: new weights written through `.data.copy_()` (no version counter moves)
  and through `load_state_dict` must both reach the next image."""
  g, cfg, first, model = run_case(0)
  assert model._inference_cache is not None
  gen = torch.Generator().manual_seed(9)
  other = make_classifier(cfg['c'], cfg['ncls'])
  with torch.no_grad():
    for p in other.parameters():
      p.copy_(p + 0.05 * torch.randn(p.shape, generator=gen))
    other.semantic_classifier[1].running_var.copy_(0.03 + 0.05 * torch.rand(2 * cfg['c'], generator=gen))
  fresh = run_case(0, make_classifier(cfg['c'], cfg['ncls'], other.state_dict()).to(DEV))[2]
  assert not torch.equal(fresh['semantic_logit'], first['semantic_logit'])
  # 1. raw writes into the storage the cache was built from
  for name, t in other.state_dict().items():
    dict(model.state_dict(keep_vars=True))[name].data.copy_(t)
  assert model._inference_cache is not None                       # nothing told the module
  got = run_case(0, model)[2]
  assert torch.equal(got['semantic_logit'], fresh['semantic_logit'])
  assert torch.equal(got['semantic_prediction'], fresh['semantic_prediction'])
  # 2. load_state_dict back to the fixture's weights
  model.load_state_dict(n6_case(g, 0)[3])
  assert model._inference_cache is None
  got = run_case(0, model)[2]
  assert torch.equal(got['semantic_logit'], first['semantic_logit'])


def test_inference_entry_point_reads_a_classifier_snapshot(tmp_path, capsys):
  """pyscripts/inference/inference_softmax.py on a snapshot written by pyscripts/train/train_classifier.py (stage 1 ->
  stage 2 -> label maps + one JSON line with mIoU against the synthetic labels)."""
  import importlib.util
  import json
  import os
  from test_train_cli import ROOT, YAML, load_cli
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101')                    # 129 x 129 images, 2 x 2 windows
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
  load('spml_inference_softmax_cli', ('pyscripts', 'inference', 'inference_softmax.py')).main(
      ['--snapshot_dir', str(snap2), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic'])
  line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
  result = json.loads(line)
  assert result['images'] >= 1 and result['images_per_s'] > 0 and 0.0 <= result['mIoU'] <= 100.0
  assert result['head_path'] == sc.HIP_HEAD_PATH
  maps = sorted(os.listdir(str(save / 'semantic_gray')))
  assert len(maps) == result['images'] and maps[0].endswith('.npy')
  label = np.load(str(save / 'semantic_gray' / maps[0]))
  assert label.dtype == np.uint8 and label.shape == (129, 129) and label.max() < 21
