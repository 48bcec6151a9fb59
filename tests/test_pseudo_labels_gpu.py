"""Pseudo-label generation on the GPU: the kernels of csrc/pseudo_label.hip one by one against the plain-torch
restatement (tests/pseudo_label_ref.py), then `pseudo_labels_softmax` against the fixture exec'd from the reference's
own lines (tests/golden/n7_pseudo_labels.npz; tests/test_pseudo_labels.py keeps fixture and restatement honest on the
CPU).  Tolerances are the project's existing ones: 2e-6 absolute for unit embeddings and class sums (the K1 / window
bar), rtol 1e-4 / atol 1e-6 for CAMs and walked CAMs, rtol 1e-4 / atol 1e-9 for the transition matrix (the bars of
test_affinity_random_walk_matches_reference_lines), labels exact wherever the yardstick's top-2 margin is at least
2e-4 * max, with fewer than 1 % of the pixels outside that set."""
import json
import os

import numpy as np
import pytest
import torch

import pseudo_label_ref as ref
from conftest import load_golden
from spml_amd import _ffi, inference
from spml_amd.models.predictions import softmax_classifier as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def network_like(gen, c, hp, wp, amplitude=1.0):
  """A smooth map plus noise, [1, c, hp, wp] on the CPU (what a network produces: neighbouring pixels correlate)."""
  base = torch.randn(1, c, hp // 8 + 2, wp // 8 + 2, generator=gen)
  x = torch.nn.functional.interpolate(base, size=(hp, wp), mode='bilinear', align_corners=False)
  return amplitude * (x + 0.1 * torch.randn(1, c, hp, wp, generator=gen))


def both_layouts(x):
  """The [C, Hp, Wp] view of an NCHW and of a channels-last device copy of x [1, C, Hp, Wp]."""
  nchw = x.to(DEV).contiguous()
  nhwc = x.to(DEV).contiguous(memory_format=torch.channels_last)
  assert nchw[0].stride() != nhwc[0].stride() or x.shape[1] == 1
  return nchw[0], nhwc[0]


# (C, Hp, Wp, rh, rw, oh, ow): rh = Hp and rh < Hp, outputs that do not divide the source, one output row / column
VIEW_SHAPES = [(8, 40, 56, 40, 56, 5, 7), (64, 72, 64, 70, 58, 11, 9), (66, 96, 80, 93, 77, 11, 9),
               (64, 33, 47, 30, 41, 1, 5), (130, 24, 40, 17, 40, 3, 1)]


@pytest.mark.parametrize('c,hp,wp,rh,rw,oh,ow', VIEW_SHAPES)
@pytest.mark.parametrize('views', [1, 2, 4])
def test_resample_unit_against_the_restatement(c, hp, wp, rh, rw, oh, ow, views):
  gen = torch.Generator().manual_seed(c + hp + views)
  out_a = torch.full((views, c, oh * ow), float('nan'), device=DEV)
  out_b = torch.full((views, c, oh * ow), float('nan'), device=DEV)
  want = []
  for b in range(views):
    flip = b % 2 == 0
    x = network_like(gen, c, hp, wp, amplitude=0.5 + b)
    nchw, nhwc = both_layouts(x)
    _ffi.resample_unit(nchw, (rh, rw), flip, (oh, ow), out_a, b)
    _ffi.resample_unit(nhwc, (rh, rw), flip, (oh, ow), out_b, b)
    want.append(ref.view_unit_embedding(x, (rh, rw), flip, (oh, ow)).reshape(c, -1))
  want = torch.stack(want, 0)
  assert torch.equal(out_a, out_b)                      # NCHW and channels-last: the same bits
  err = (out_a.cpu() - want).abs().max().item()
  print('resample_unit C=%d %dx%d -> %dx%d, %d views: max error %.3e' % (c, rh, rw, oh, ow, views, err))
  assert err <= 2e-6
  torch.testing.assert_close(out_a.cpu().pow(2).sum(1), torch.ones(views, oh * ow), rtol=0, atol=1e-5)


@pytest.mark.parametrize('ncls,hp,wp,rh,rw,oh,ow', [(5, 40, 56, 40, 56, 5, 7), (21, 72, 64, 70, 58, 11, 9),
                                                    (21, 96, 80, 93, 77, 11, 9), (5, 33, 47, 30, 41, 1, 5),
                                                    (70, 24, 40, 17, 40, 3, 2), (130, 24, 40, 17, 40, 2, 3)])
@pytest.mark.parametrize('views', [1, 2, 4])
@pytest.mark.parametrize('combine', ['prob_mean', 'logit_mean'])
def test_resample_classes_accumulate_against_the_restatement(ncls, hp, wp, rh, rw, oh, ow, views, combine):
  gen = torch.Generator().manual_seed(ncls + hp + views)
  # 2e-6 absolute is a bar for values of order one (a unit vector's components, probabilities: a few roundings of
  # 2^-24 each).  Probabilities come from logits of the amplitude a trained head gives; where the LOGITS themselves are
  # summed (`logit_mean`) the inputs are scaled so that the sum of four views stays of order one -- at |sum| = 16 one
  # ulp alone is 1.9e-6 (the fixture test below covers logits of amplitude 4 at the CAM bar)
  amplitude = 3.0 if combine == 'prob_mean' else 0.25
  acc_a = torch.zeros((ncls, oh * ow), device=DEV)
  acc_b = torch.zeros((ncls, oh, ow), device=DEV)
  want = torch.zeros(ncls, oh, ow)
  for b in range(views):
    flip = b % 2 == 0
    x = network_like(gen, ncls, hp, wp, amplitude=amplitude)
    nchw, nhwc = both_layouts(x)
    _ffi.resample_classes_accumulate(nchw, (rh, rw), flip, (oh, ow), acc_a, combine)
    _ffi.resample_classes_accumulate(nhwc, (rh, rw), flip, (oh, ow), acc_b, combine)
    want += ref.view_classes(x, (rh, rw), flip, (oh, ow), combine)[0]         # views are added in call order
  assert torch.equal(acc_a.view(-1), acc_b.view(-1))
  err = (acc_b.cpu() - want).abs().max().item()
  print('resample_classes %s ncls=%d, %d views: max error %.3e at max|value| %.3f'
        % (combine, ncls, views, err, want.abs().max().item()))
  assert want.abs().max().item() < 8.0
  assert err <= 2e-6
  if combine == 'prob_mean':
    torch.testing.assert_close(acc_b.sum(0).cpu(), torch.full((oh, ow), float(views)), rtol=0, atol=1e-5)


@pytest.mark.parametrize('ncls,oh,ow', [(5, 5, 7), (21, 11, 9), (21, 46, 62), (70, 5, 7), (130, 5, 7)])
@pytest.mark.parametrize('views', [1, 2, 4])
@pytest.mark.parametrize('combine', ['prob_mean', 'logit_mean'])
@pytest.mark.parametrize('threshold', [None, 0.3])
def test_cam_finalize_against_the_restatement(ncls, oh, ow, views, combine, threshold):
  gen = torch.Generator().manual_seed(ncls + oh + views)
  terms = []
  for _ in range(views):
    x = network_like(gen, ncls, oh, ow, amplitude=4.0)
    terms.append(torch.softmax(x, 1) if combine == 'prob_mean' else x)
  acc = terms[0][0].clone()
  for t in terms[1:]:
    acc += t[0]
  tags = torch.ones(ncls, dtype=torch.bool)
  tags[[1, ncls - 1]] = False                                     # absent classes, the last plane among them
  if threshold is None:
    tags[0] = False                                               # ... and class 0 without a threshold
  want = ref.cams(terms, tags, combine, threshold)
  got = _ffi.cam_finalize(acc.to(DEV), views, tags.to(DEV), combine, threshold)
  assert tuple(got.shape) == (ncls, oh, ow)
  torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-6)
  absent = ~tags
  absent[0] = False
  assert bool((got.cpu()[absent] == 0).all())
  if threshold is None:
    assert bool((got[0] == 0).all())
  else:
    assert bool((got[0] == threshold).all())
  present = tags.clone()
  present[0] = False
  assert torch.equal(got.cpu()[present].flatten(1).max(1).values, torch.ones(int(present.sum())))
  assert torch.equal(got, _ffi.cam_finalize(acc.to(DEV), views, tags.to(DEV).to(torch.uint8), combine, threshold))


@pytest.mark.parametrize('ncls,oh,ow,h,w', [(21, 11, 15, 88, 120), (21, 11, 9, 93, 77), (5, 3, 4, 29, 37),
                                            (21, 46, 62, 375, 500), (12, 1, 1, 9, 15)])
def test_upsample_argmax_against_the_yardstick(ncls, oh, ow, h, w):
  gen = torch.Generator().manual_seed(ncls + h)
  cam = torch.rand(1, ncls, oh, ow, generator=gen) if oh * ow == 1 else network_like(gen, ncls, oh, ow).abs()
  cam = cam[0].contiguous()
  want, margin = ref.labels_and_margin(cam, (h, w))
  got = _ffi.upsample_argmax(cam.to(DEV), h, w)
  assert got.dtype == torch.int64 and tuple(got.shape) == (h, w)
  sure = margin >= ref.LOW_MARGIN * cam.abs().max()
  low = (~sure).float().mean().item()
  print('upsample_argmax %dx%d -> %dx%d: %.2f %% below the margin, %d mismatches among them'
        % (oh, ow, h, w, 100 * low, int((got.cpu() != want)[~sure].sum())))
  assert low < 0.01
  assert torch.equal(got.cpu()[sure], want[sure])


def test_upsample_argmax_ties_and_nans():
  gen = torch.Generator().manual_seed(3)
  cam = torch.rand(7, 6, 8, generator=gen)
  cam[2] = cam[2] + 10.0
  cam[5] = cam[2]                                         # two identical planes above all others: the lower index wins
  got = _ffi.upsample_argmax(cam.to(DEV), 45, 61).cpu()
  assert bool((got == 2).all())
  assert torch.equal(_ffi.upsample_argmax(torch.zeros(4, 3, 3, device=DEV), 20, 20).cpu(), torch.zeros(20, 20, dtype=torch.int64))
  cam = torch.rand(7, 6, 8, generator=gen)                # NaN, outside the contract: as torch.argmax, no fault
  cam[4, 2, 3] = float('nan')
  cam[1, 4, 6] = float('nan')
  cam[4, 4, 6] = float('nan')                             # two NaNs at one place: the first is kept
  up = ref.upsampled(cam, (45, 61))
  want = up.argmax(0)
  got = _ffi.upsample_argmax(cam.to(DEV), 45, 61).cpu()
  nan = torch.isnan(up).any(0)
  assert int(nan.sum()) > 20 and set(want[nan].unique().tolist()) == {1, 4}
  assert torch.equal(got[nan], want[nan])
  _, margin = ref.labels_and_margin(torch.nan_to_num(cam, nan=0.0), (45, 61))
  sure = ~nan & (margin >= ref.LOW_MARGIN)
  assert torch.equal(got[sure], want[sure])


def test_unsupported_and_invalid_shapes_raise():
  with pytest.raises(_ffi.SpmlHipError):                   # more channels than the kernels take
    _ffi.resample_unit(torch.zeros(260, 8, 8, device=DEV), (8, 8), False, (1, 1), torch.zeros(1, 260, 1, device=DEV), 0)
  with pytest.raises(_ffi.SpmlHipError):                   # crop outside the plane
    _ffi.resample_unit(torch.zeros(8, 8, 8, device=DEV), (9, 8), False, (1, 1), torch.zeros(1, 8, 1, device=DEV), 0)
  with pytest.raises(_ffi.SpmlHipError):                   # slice outside [B, C, n]
    _ffi.resample_unit(torch.zeros(8, 8, 8, device=DEV), (8, 8), False, (1, 1), torch.zeros(1, 8, 1, device=DEV), 1)
  with pytest.raises(_ffi.SpmlHipError):                   # fp16 logits
    _ffi.resample_classes_accumulate(torch.zeros(5, 8, 8, device=DEV).half(), (8, 8), False, (1, 1),
                                     torch.zeros(5, 1, device=DEV))
  with pytest.raises(_ffi.SpmlHipError):                   # accumulator of another size
    _ffi.resample_classes_accumulate(torch.zeros(5, 8, 8, device=DEV), (8, 8), False, (2, 2), torch.zeros(5, 3, device=DEV))
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.cam_finalize(torch.zeros(5, 4, device=DEV), 0, torch.ones(5, dtype=torch.bool, device=DEV))
  with pytest.raises(_ffi.SpmlHipError):                   # more classes than the kernels take
    _ffi.cam_finalize(torch.zeros(260, 4, device=DEV), 1, torch.ones(260, dtype=torch.bool, device=DEV))


# ---- the fixture, end to end ------------------------------------------------------------------------------------
class StubEmbedder(torch.nn.Module):
  """Returns the fixture's embeddings: every view image carries its index in pixel [0, 0, 0, 0]."""

  def __init__(self, outputs, channels_last=False):
    super().__init__()
    self.outputs, self.channels_last, self.calls = outputs, channels_last, 0

  def generate_embeddings(self, datas, targets=None, resize_as_input=False):
    assert resize_as_input
    self.calls += 1
    ids = [int(v) for v in datas['image'][:, 0, 0, 0].cpu()]
    emb = torch.cat([self.outputs[i][0] for i in ids], 0).to(DEV)
    if self.channels_last:
      emb = emb.contiguous(memory_format=torch.channels_last)
    return {'embedding': emb}


class StubHead(torch.nn.Module):
  """Adds the fixture's logits of the view whose embedding it is handed (found by its first values)."""

  def __init__(self, outputs, num_classes=21):
    super().__init__()
    self.outputs, self.num_classes = outputs, num_classes

  def prepare_inference(self):
    return None

  def accumulate_logits(self, embedding, canvas, sh, sw):
    probe = embedding[0, :4, :2, :2].cpu()
    match = [i for i, (e, _) in enumerate(self.outputs) if e.shape == embedding.shape and torch.equal(e[0, :4, :2, :2], probe)]
    assert len(match) == 1 and (sh, sw) == (0, 0) and bool((canvas == 0).all())
    canvas += self.outputs[match[0]][1].to(DEV)
    return 'fixture'


def run_fixture(g, ci, combine, steps, channels_last=False):
  outputs, meta, image_hw, tags = ref.fixture_case(g, ci)
  views = []
  for vi, ((emb, _), (rh, rw, flip)) in enumerate(zip(outputs, meta)):
    image = torch.zeros(1, 3, emb.shape[2], emb.shape[3])
    image[0, 0, 0, 0] = vi
    views.append((image.to(DEV), (rh, rw), flip))
  embedder = StubEmbedder(outputs, channels_last)
  out = inference.pseudo_labels_softmax(embedder, StubHead(outputs), views, image_hw, tags.to(DEV), combine=combine,
                                        walk_steps=steps, return_transition=True)
  assert embedder.calls == len({tuple(o[0].shape) for o in outputs})          # a flip pair shares the backbone call
  return out, image_hw


@pytest.mark.parametrize('ci', range(ref.NUM_CASES))
@pytest.mark.parametrize('tag,combine,steps', ref.RECIPES)
def test_pseudo_labels_match_reference_lines(ci, tag, combine, steps):
  g = load_golden('n7_pseudo_labels')
  t = 'c%d_' % ci
  out, image_hw = run_fixture(g, ci, combine, steps)
  torch.testing.assert_close(out['transition'].cpu(), g[t + 'trans'], rtol=1e-4, atol=1e-9)
  torch.testing.assert_close(out['cam'].cpu(), g[t + tag + '_cam'], rtol=1e-4, atol=1e-6)
  cam_rw = g[t + tag + '_cam_rw']
  err = (out['cam_rw'].cpu() - cam_rw).abs().max().item()
  print('case %d %s: max|d cam_rw| %.3e at max %.4f' % (ci, tag, err, cam_rw.abs().max().item()))
  torch.testing.assert_close(out['cam_rw'].cpu(), cam_rw, rtol=1e-4, atol=1e-6)
  want, margin = ref.labels_and_margin(cam_rw, image_hw)
  assert torch.equal(margin, g[t + tag + '_margin'])
  sure = margin >= ref.LOW_MARGIN * cam_rw.abs().max()
  assert (~sure).float().mean().item() < 0.01
  pred = out['semantic_prediction'].cpu()
  assert pred.dtype == torch.int64 and tuple(pred.shape) == image_hw
  assert torch.equal(pred[sure], want[sure])
  # a channels-last network output gives the same bits
  again, _ = run_fixture(g, ci, combine, steps, channels_last=True)
  for k in ('transition', 'cam', 'cam_rw', 'semantic_prediction'):
    assert torch.equal(out[k], again[k]), k


def test_two_calls_are_bit_identical_in_either_mode():
  g = load_golden('n7_pseudo_labels')
  first, _ = run_fixture(g, 1, 'prob_mean', 6)
  second, _ = run_fixture(g, 1, 'prob_mean', 6)
  before = _ffi.set_deterministic(True)
  try:
    third, _ = run_fixture(g, 1, 'prob_mean', 6)
    fourth, _ = run_fixture(g, 1, 'prob_mean', 6)
  finally:
    _ffi.set_deterministic(before)
  for k in ('transition', 'cam', 'cam_rw', 'semantic_prediction'):
    assert torch.equal(first[k], second[k]) and torch.equal(third[k], fourth[k]) and torch.equal(first[k], third[k]), k


def test_real_network_flip_pair():
  """ResNet-101 DeepLab + SoftmaxClassifier at random weights, channels-last, a flip pair of a 161 x 225 image."""
  from spml_amd.train import build_models, voc12_scribble_config
  cfg = voc12_scribble_config(batch_size=1, use_syncbn=False)
  ncls = cfg.dataset.num_classes
  torch.manual_seed(7)
  emb_model, _ = build_models(cfg, softmax_head=False)
  emb_model = emb_model.to(DEV).to(memory_format=torch.channels_last).eval()
  head = sc.softmax_classifier(cfg).to(DEV).eval()
  gen = torch.Generator().manual_seed(8)
  image = torch.randn(1, 3, 161, 225, generator=gen).to(DEV)
  views = inference.flip_scale_views(image, [1], True, (193, 225))
  assert [tuple(v[0].shape) for v in views] == [(1, 3, 193, 225)] * 2 and [v[2] for v in views] == [True, False]
  label = torch.zeros(161, 225, dtype=torch.long)
  label[:, 100:] = 7
  label[80:, :50] = 15
  label[:4] = 255
  tags = inference.label_tags_from_map(label.to(DEV), ncls)
  out = inference.pseudo_labels_softmax(emb_model, head, views, (161, 225), tags, return_transition=True)
  assert out['head_path'] == sc.HIP_HEAD_PATH
  assert tuple(out['cam'].shape) == (ncls, 20, 28) == tuple(out['cam_rw'].shape)
  assert tuple(out['transition'].shape) == (560, 560)
  pred = out['semantic_prediction']
  assert pred.dtype == torch.int64 and tuple(pred.shape) == (161, 225)
  for k in ('cam', 'cam_rw', 'transition'):
    assert bool(torch.isfinite(out[k]).all()), k
  torch.testing.assert_close(out['transition'].sum(0).cpu(), torch.ones(560), rtol=1e-4, atol=0)
  assert set(pred.unique().tolist()) <= {0, 7, 15}
  assert bool((out['cam'][~tags] == 0).all()) and 'transition' not in inference.pseudo_labels_softmax(
      emb_model, head, views, (161, 225), tags)


@pytest.mark.parametrize('name', ['pseudo_softmaxrw', 'pseudo_softmax'])
def test_programs_write_label_maps_from_a_stage1_snapshot(name, tmp_path, capsys):
  """Stage-1 snapshot written by pyscripts/train/train.py (a SegsortSoftmax snapshot carries the classifier head) ->
  label maps + one JSON line."""
  from test_pseudo_labels import load_program
  from test_train_cli import YAML, load_cli
  yaml = YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101').replace('image_size: 97', 'image_size: 129')
  assert 'image_size: 129' in yaml
  cfg = tmp_path / 'config_emb.yaml'
  cfg.write_text(yaml)
  snap = tmp_path / 'stage1'
  load_cli().main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--data_list', 'synthetic'])
  capsys.readouterr()
  save = tmp_path / 'pseudo'
  prog = load_program(name)
  prog.main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic'])
  line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
  result = json.loads(line)
  assert result['images'] >= 1 and result['images_per_s'] > 0 and 0.0 <= result['mIoU'] <= 100.0
  assert (result['combine'], result['walk_steps'], tuple(result['scales'])) == (prog.COMBINE, prog.WALK_STEPS, tuple(prog.SCALES))
  assert result['head_path'] == sc.HIP_HEAD_PATH
  maps = sorted(os.listdir(str(save / 'semantic_gray')))
  assert len(maps) == result['images'] and maps[0].endswith('.npy')
  label = np.load(str(save / 'semantic_gray' / maps[0]))
  assert label.dtype == np.uint8 and label.shape == (129, 129) and label.max() < 21
