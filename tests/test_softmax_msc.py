"""Multi-scale + flip softmax inference, the parts that need no GPU: the fixture (tests/golden/n8_softmax_msc.npz, exec'd
from pyscripts/inference/inference_softmax_msc.py:107-143 / :146-149 by tools/gen_golden.py) against a plain-torch
restatement with separable window counts, `window_counts` against the reference's counts loop, the low-margin cap, the
argument errors of `predict_softmax_multiscale` and the header's declaration."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_softmax_inference import make_classifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_BOUND = 1e-4       # the project's parity bound on a logit, relative to max|logit| (tests/test_softmax_inference_gpu.py)


def n8_case(g, ci):
  """(cfg dict, views, stub conv, classifier state dict) of fixture case `ci`; views = list of
  `(image [1,3,Hp,Wp], (rh, rw), is_flip)` rebuilt from the stored un-flipped scaled images (flip and zero-padding are
  exact), in the stored order: per scale the flipped view first."""
  t = 'c%d_' % ci
  c, ncls, h, w, ch, cw, sh, sw = [int(v) for v in g[t + 'cfg']]
  conv = torch.nn.Conv2d(3, c, 5, padding=2)
  with torch.no_grad():
    conv.weight.copy_(g[t + 'conv_w'])
    conv.bias.copy_(g[t + 'conv_b'])
  state = {k: torch.as_tensor(g[t + 'sd_' + k]) for k in g[t + 'state_names']}
  views = []
  for si, pad_h, pad_w, rh, rw, flip in g[t + 'views'].tolist():
    scaled = g[t + 'scaled%d' % si]
    assert tuple(scaled.shape) == (1, 3, rh, rw) and pad_h == max(rh, ch) and pad_w == max(rw, cw)
    view = torch.zeros(1, 3, pad_h, pad_w)
    view[:, :, :rh, :rw] = torch.flip(scaled, dims=[3]) if flip else scaled
    views.append((view, (rh, rw), bool(flip)))
  cfg = dict(c=c, ncls=ncls, image=(h, w), crop=(ch, cw), stride=(sh, sw))
  return cfg, views, conv, state


def prob_bound(g, ci):
  """B of the issue: the logit bound is 1e-4 * max|logit| per view, a softmax moves a probability by at most half of
  the logit error, and the errors of the views are summed."""
  t = 'c%d_' % ci
  return 0.5 * len(g[t + 'views']) * LOGIT_BOUND * float(g[t + 'max_abs_logit'])


def reference_counts(pad_h, pad_w, crop, stride):
  """The counts loop of inference_softmax_msc.py:108-134, restated."""
  nh = math.ceil(1.0 * (pad_h - crop[0]) / stride[0]) + 1
  nw = math.ceil(1.0 * (pad_w - crop[1]) / stride[1]) + 1
  counts = torch.zeros(pad_h, pad_w)
  for eh in np.linspace(crop[0], pad_h, nh, dtype=np.int32):
    for ew in np.linspace(crop[1], pad_w, nw, dtype=np.int32):
      counts[eh - crop[0]:eh, ew - crop[1]:ew] += 1
  return counts


def restated_view_tail(canvas, cnt_y, cnt_x, crop_hw, flip, out_hw):
  """inference_softmax_msc.py:135-143 in plain torch ops, in the dtype of `canvas` [ncls,Hp,Wp]: divide by the counts,
  crop, bilinear resize to `out_hw`, softmax over the classes, flip the RESULT.  -> probabilities [ncls,h,w]."""
  logit = canvas.unsqueeze(0) / (cnt_y.view(-1, 1) * cnt_x.view(1, -1))
  logit = logit[..., :crop_hw[0], :crop_hw[1]]
  logit = F.interpolate(logit, size=tuple(out_hw), mode='bilinear')
  prob = F.softmax(logit, dim=1)[0]
  return torch.flip(prob, dims=[2]) if flip else prob


def restated_multiscale(views, conv, state, cfg, dtype=torch.float32, stats=None):
  """inference_softmax_msc.py:107-149 + softmax_classifier.py:52-55 (eval mode) in plain torch ops on the CPU, the counts
  as the outer product of `window_counts`.  -> (summed probabilities [ncls,h,w], labels [h,w]); `stats`, when given,
  receives `max_abs_logit`, the largest |crop logit|."""
  from spml_amd.inference import sliding_window_ends, window_counts
  ch, cw = cfg['crop']
  p = 'semantic_classifier.'
  st = {k: v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v for k, v in state.items()}
  conv_w, conv_b = conv.weight.detach().to(dtype), conv.bias.detach().to(dtype)
  total = None
  with torch.no_grad():
    for image, (rh, rw), flip in views:
      pad_h, pad_w = image.shape[-2:]
      canvas = torch.zeros(1, cfg['ncls'], pad_h, pad_w, dtype=dtype)
      for eh in sliding_window_ends(pad_h, ch, cfg['stride'][0]):
        for ew in sliding_window_ends(pad_w, cw, cfg['stride'][1]):
          sh, sw = int(eh) - ch, int(ew) - cw
          emb = F.conv2d(image[:, :, sh:eh, sw:ew].to(dtype), conv_w, conv_b, padding=2)
          x = emb / torch.norm(emb, dim=1, keepdim=True)
          x = F.conv2d(x, st[p + '0.weight'], padding=1)
          x = F.batch_norm(x, st[p + '1.running_mean'], st[p + '1.running_var'], st[p + '1.weight'], st[p + '1.bias'],
                           training=False, eps=1e-5)
          x = F.conv2d(F.relu(x), st[p + '4.weight'], st[p + '4.bias'])
          if stats is not None:
            stats['max_abs_logit'] = max(stats.get('max_abs_logit', 0.0), x.abs().max().item())
          canvas[..., sh:eh, sw:ew] += x
      cnt_y = torch.from_numpy(window_counts(pad_h, ch, cfg['stride'][0])).to(dtype)
      cnt_x = torch.from_numpy(window_counts(pad_w, cw, cfg['stride'][1])).to(dtype)
      prob = restated_view_tail(canvas[0], cnt_y, cnt_x, (rh, rw), flip, cfg['image'])
      total = prob if total is None else total + prob
  return total, torch.argmax(total, 0)


@pytest.mark.parametrize('ci', [0, 1])
def test_fixture_is_reproduced_by_plain_torch(ci):
  g = load_golden('n8_softmax_msc')
  cfg, views, conv, state = n8_case(g, ci)
  t = 'c%d_' % ci
  ref = g[t + 'semantic_prob']
  assert tuple(ref.shape) == (cfg['ncls'],) + cfg['image'] and ref.dtype == torch.float32
  assert g[t + 'semantic_pred'].dtype == torch.uint8 and tuple(g[t + 'semantic_pred'].shape) == cfg['image']
  flips = [v[2] for v in views]
  assert len(views) == 6 and flips == [True, False] * 3          # per scale the flipped view first
  total, pred = restated_multiscale(views, conv, state, cfg)
  err = (total - ref).abs().max().item()
  print('case %d: max prob sum %.4f, restatement error %.3e' % (ci, ref.max().item(), err))
  assert torch.allclose(total, ref, rtol=1e-5, atol=1e-6)
  sure = g[t + 'margin'] >= 2 * prob_bound(g, ci)
  assert torch.equal(pred[sure], g[t + 'semantic_pred'].long()[sure])
  # every pixel's probabilities sum to the number of views
  assert (ref.sum(0) - len(views)).abs().max().item() <= 1e-4


@pytest.mark.parametrize('ci', [0, 1])
def test_stored_margin_is_the_sums_own_and_the_cap_holds(ci):
  g = load_golden('n8_softmax_msc')
  t = 'c%d_' % ci
  ref = g[t + 'semantic_prob']
  top2 = ref.topk(2, dim=0).values
  assert torch.equal(top2[0] - top2[1], g[t + 'margin'])
  assert torch.equal(torch.argmax(ref, 0), g[t + 'semantic_pred'].long())
  bound = prob_bound(g, ci)
  low = (g[t + 'margin'] < 2 * bound).float().mean().item()
  print('case %d: max|logit| %.4f, B %.3e, low-margin share %.4f' % (ci, float(g[t + 'max_abs_logit']), bound, low))
  assert 1.0 < float(g[t + 'max_abs_logit']) < 50.0
  assert low < 0.01
  assert g[t + 'semantic_pred'].unique().numel() >= 3


def test_window_counts_outer_product_is_the_reference_counts():
  from spml_amd.inference import window_counts
  g = load_golden('n8_softmax_msc')
  seen = set()
  for ci in (0, 1):
    cfg, views, _, _ = n8_case(g, ci)
    for image, _, _ in views:
      seen.add((tuple(image.shape[-2:]), cfg['crop'], cfg['stride']))
  seen.add(((513, 750), (513, 513), (342, 342)))                  # the benchmark's largest view
  assert ((66, 90), (32, 32), (20, 20)) in seen and ((51, 62), (50, 50), (33, 33)) in seen
  for (pad_h, pad_w), crop, stride in sorted(seen):
    cy, cx = window_counts(pad_h, crop[0], stride[0]), window_counts(pad_w, crop[1], stride[1])
    assert cy.dtype == np.float32 and cy.shape == (pad_h,) and cx.shape == (pad_w,)
    assert torch.equal(torch.from_numpy(cy).view(-1, 1) * torch.from_numpy(cx).view(1, -1),
                       reference_counts(pad_h, pad_w, crop, stride))
  # the 66 x 90 view: 3 x 4 windows, two of them over a pixel per axis -- non-uniform counts 1, 2 and 4
  assert window_counts(66, 32, 20).max() == 2 and window_counts(90, 32, 20).max() == 2
  assert window_counts(750, 513, 342).max() == 2 and window_counts(750, 513, 342).min() == 1
  ones = window_counts(50, 50, 33)                                  # pad = crop: one window
  assert ones.dtype == np.float32 and np.array_equal(ones, np.ones(50, dtype=np.float32))


def test_predict_softmax_multiscale_argument_errors():
  from spml_amd import _ffi, inference
  model = make_classifier(16, 5)
  conv = torch.nn.Conv2d(3, 16, 5, padding=2)
  with pytest.raises(ValueError):
    inference.predict_softmax_multiscale(conv, model, [], (8, 8), (8, 8), (5, 5))
  views = inference.flip_scale_views(torch.zeros(1, 3, 8, 8), [1], True, (8, 8))
  with pytest.raises(_ffi.SpmlHipError):
    inference.predict_softmax_multiscale(conv, model, views, (8, 8), (8, 8), (5, 5))
  with pytest.raises(ValueError):
    inference.predict_softmax_multiscale(conv, model, [(torch.zeros(3, 8, 8), (8, 8), False)], (8, 8), (8, 8), (5, 5))


def test_header_declares_the_entry_and_version_7():
  # (the entry point arrived with version 7; the header has since moved to 8: spml_upsample_ce_bwd_path_name)
  from spml_amd import _ffi
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  assert int(re.search(r'#define SPML_ABI_VERSION (\d+)', hdr).group(1)) == 8 == _ffi.ABI_VERSION
  decl = re.search(r'int spml_view_probs_accumulate_f32\(([^)]*)\);', hdr)
  assert decl is not None and 'spml_view_probs_accumulate_f32' in _ffi.EXPORTS
  args = [a.strip() for a in decl.group(1).split(',')]
  assert args == ['const float* canvas', 'int ncls', 'int Hp', 'int Wp', 'const float* cnt_y', 'const float* cnt_x',
                  'int rh', 'int rw', 'int flip', 'int h', 'int w', 'float* acc', 'void* stream']
  assert len(_ffi._SIGNATURES['spml_view_probs_accumulate_f32'][1]) == len(args)
