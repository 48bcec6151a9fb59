"""Multi-scale + flip kNN inference on the GPU: the vote-view kernel of csrc/knn_msc.hip alone against the reference's
torch ops, then `predict_knn_multiscale` against the fixture exec'd from the reference's own lines
(tests/golden/n9_knn_msc.npz; tests/test_knn_msc.py keeps that fixture honest on the CPU), its framework path above 64
classes and the command-line entry point.  Measured figures: profiles/knn_msc.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from spml_amd import _ffi, inference
from test_knn_msc import LOW_CAP, load_program, n9_case, restated_multiscale, restated_view_tail, restated_votes, \
    sure_pixels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (ncls, m, k, (rh, rw), (h, w), flip)
KERNEL_CASES = [
    (5, 7, 20, (22, 30), (44, 60), 1),            # up-sampling
    (21, 144, 20, (51, 62), (41, 50), 0),         # down-sampling, the largest k-means m
    (33, 9, 3, (37, 23), (19, 45), 1),            # down on one axis, up on the other, odd w
    (64, 1, 1, (1, 1), (7, 5), 1),                # a one-pixel source, one segment
    (1, 4, 20, (8, 8), (8, 8), 0),                # every output is exactly start + 1
    (8, 50, 20, (20, 130), (20, 130), 1),         # scale 1: start + votes[clu] mirrored, bit for bit
    (21, _ffi.MAX_VIEW_VOTES_SEGMENTS, 20, (70, 64), (35, 50), 0)]      # the largest supported m (every id occurs)


def device_inputs(case, seed, label_high=None):
  """Inputs made on the device: one segment id per source pixel (every id of a permutation first, so that the largest
  occurs), retrieved labels per segment, a non-zero accumulator."""
  ncls, m, k, (rh, rw), out_hw, _ = case
  gen = torch.Generator(device=DEV).manual_seed(seed)
  clu = torch.randint(0, m, (rh * rw,), generator=gen, device=DEV)
  head = min(m, rh * rw)
  clu[:head] = torch.randperm(m, generator=gen, device=DEV)[:head]
  clu[0] = m - 1
  topk = torch.randint(0, label_high or ncls, (m, k), generator=gen, device=DEV)
  start = torch.rand((ncls,) + out_hw, generator=gen, device=DEV)
  return clu, topk, start


def cpu_refs(clu, topk, case, start, calls):
  """start + `calls` x the restated tail (tests/test_knn_msc.py) on the CPU, in fp32 and in fp64."""
  ncls, _, _, crop, out_hw, flip = case
  refs = {}
  for dtype in (torch.float32, torch.float64):
    ref = start.cpu().to(dtype)
    for _ in range(calls):
      ref = ref + restated_view_tail(clu.cpu(), topk.cpu(), ncls, crop, flip, out_hw, dtype)
    refs[dtype] = ref
  return refs[torch.float32], refs[torch.float64]


def assert_within_the_bound(got, ref32, ref64, what):
  """Yardstick: the reference's ops in fp64.  Bound: 4 x the error of the same ops in fp32 on the CPU against that fp64
  result on this very case (the project's N8 rule: both are fp32 chains of the same length; the factor covers fma
  contraction and another order of the four products).  Where that error is 0 the kernel must be exact."""
  ref_err = (ref32.double() - ref64).abs().max().item()
  err = (got.cpu().double() - ref64).abs().max().item()
  print('%s: max error %.3e, fp32 CPU ops %.3e (both against fp64)' % (what, err, ref_err))
  assert torch.isfinite(got).all()
  assert err <= 4 * ref_err


@functools.lru_cache(maxsize=None)
def kernel_case(index):
  """One kernel case, computed once: the kernel's result after one and after two calls and the two CPU references."""
  case = KERNEL_CASES[index]
  ncls, _, _, crop, _, flip = case
  clu, topk, start = device_inputs(case, 900 + index)
  acc = start.clone()
  assert _ffi.view_votes_accumulate(clu, crop, topk, ncls, flip, acc) is acc
  once = acc.cpu()
  _ffi.view_votes_accumulate(clu.view(crop), crop, topk, ncls, flip, acc)              # ([rh, rw] is taken as well)
  twice = acc.cpu()
  ref32, ref64 = cpu_refs(clu, topk, case, start, 2)
  return dict(clu=clu.cpu(), topk=topk.cpu(), start=start.cpu(), once=once, twice=twice, ref32=ref32, ref64=ref64)


@pytest.mark.parametrize('index', range(len(KERNEL_CASES)))
def test_view_kernel_matches_the_reference_ops(index):
  case, r = KERNEL_CASES[index], kernel_case(index)
  ncls, m, k, crop, out_hw, flip = case
  assert torch.isfinite(r['once']).all()
  assert not torch.equal(r['once'], r['start']) and not torch.equal(r['twice'], r['once'])
  assert_within_the_bound(r['twice'], r['ref32'], r['ref64'], 'view kernel %r' % (case,))
  if ncls == 1:                                                # one class: every vote is exactly 1
    assert torch.equal(r['once'], r['start'] + 1.0) and torch.equal(r['twice'], r['start'] + 1.0 + 1.0)
  if crop == out_hw:                                           # scale 1: the weights are exactly 0 and 1
    votes = restated_votes(r['topk'], ncls)[r['clu']].view(crop + (ncls,)).permute(2, 0, 1)
    votes = torch.flip(votes, dims=[2]) if flip else votes
    assert torch.equal(r['once'], r['start'] + votes) and torch.equal(r['twice'], r['start'] + votes + votes)


def ulp_distance(got, want):
  """max |got - want| in units of the fp32 spacing at `want`."""
  ulp = (torch.nextafter(want, torch.full_like(want, float('inf'))) - want).double()
  return ((got.double() - want.double()).abs() / ulp).max().item()


def source_taps(out_size, in_size):
  """(i0, i1) of ATen's bilinear rule (align_corners = False) for every destination index, restated on the host."""
  d = np.arange(out_size, dtype=np.float32)
  src = np.maximum(np.float32(in_size / out_size) * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0))
  i0 = np.minimum(src.astype(np.int64), in_size - 1)
  return i0, np.minimum(i0 + 1, in_size - 1)


@pytest.mark.parametrize('flip', [0, 1])
def test_pixels_inside_a_segment_carry_its_vote_vector(flip):
  """Three segments laid out as stripes six source pixels wide, k = 4 (votes are multiples of 1/4), 2 x up-sampling
  (weights 1/4 and 3/4: every product and sum is exact): every output pixel whose four taps share a segment equals that
  segment's vote vector, to 2 ulp."""
  ncls, (rh, rw), (h, w) = 4, (12, 18), (24, 36)
  seg_of_x = torch.arange(rw) // 6
  clu = seg_of_x.view(1, rw).expand(rh, rw).contiguous().to(DEV)
  topk = torch.tensor([[0, 0, 1, 2], [1, 1, 1, 1], [2, 3, 3, 0]], device=DEV)
  want_rows = torch.tensor([[.5, .25, .25, 0.], [0., 1., 0., 0.], [.25, 0., .25, .5]])
  assert torch.equal(restated_votes(topk.cpu(), ncls), want_rows)
  got = _ffi.view_votes_accumulate(clu, (rh, rw), topk, ncls, flip, torch.zeros((ncls, h, w), device=DEV)).cpu()
  i0, i1 = source_taps(w, rw)
  xd = w - 1 - np.arange(w) if flip else np.arange(w)          # evaluated at xd, stored at x
  seg0, seg1 = seg_of_x[i0[xd]], seg_of_x[i1[xd]]
  inside = seg0 == seg1
  assert 0.7 < inside.float().mean().item() < 1.0              # the stripe borders are the rest
  want = want_rows[seg0].t().unsqueeze(1).expand(ncls, h, w)
  dist = ulp_distance(got[:, :, inside], want[:, :, inside].contiguous())
  print('flip %d: %.2f ulp from the segments\' vote vectors inside the stripes' % (flip, dist))
  assert dist <= 2.0
  assert not torch.equal(got[:, :, ~inside], want[:, :, ~inside])     # (and the borders do blend)


@pytest.mark.parametrize('flip', [0, 1])
def test_id_map_cropped_from_a_padded_tensor(flip):
  """The id map is the top-left crop of a padded tensor made contiguous -- what `predict_knn_multiscale` hands over.  Ids
  outside [:rh, :rw] do not exist for the kernel: the taps `i1` are clamped to rh - 1 / rw - 1 (an `i1 = rw` would read
  the first id of the next row), pinned by the restatement on the bottom rows and right columns."""
  case = (6, 12, 20, (9, 11), (20, 23), flip)
  ncls, m, _, (rh, rw), out_hw, _ = case
  gen = torch.Generator(device=DEV).manual_seed(77)
  padded = torch.randint(0, m, (12, 16), generator=gen, device=DEV)
  clu = padded[:rh, :rw].contiguous()
  assert clu.is_contiguous() and not padded[:rh, :rw].is_contiguous()
  with pytest.raises(_ffi.SpmlHipError):                          # (the strided crop itself is refused)
    _ffi.view_votes_accumulate(padded[:rh, :rw], (rh, rw), padded[:m, :4].contiguous(), ncls, flip,
                               torch.zeros((ncls,) + out_hw, device=DEV))
  topk = torch.randint(0, ncls, (m, 20), generator=gen, device=DEV)
  start = torch.zeros((ncls,) + out_hw, device=DEV)
  got = _ffi.view_votes_accumulate(clu, (rh, rw), topk, ncls, flip, start.clone())
  ref32, ref64 = cpu_refs(clu, topk, case, start, 1)
  assert_within_the_bound(got, ref32, ref64, 'cropped id map, flip %d' % flip)
  for name, region in (('bottom rows', (slice(None), slice(-3, None))), ('right columns', (Ellipsis, slice(-3, None))),
                       ('left columns', (Ellipsis, slice(0, 3)))):
    assert_within_the_bound(got[region], ref32[region], ref64[region], name)


def test_labels_outside_the_classes_add_to_no_class():
  case = (5, 11, 20, (13, 17), (26, 31), 1)
  ncls, m, k, crop, out_hw, flip = case
  clu, topk, _ = device_inputs(case, 950, label_high=ncls + 4)
  assert int(topk.max()) >= ncls
  start = torch.zeros((ncls,) + out_hw, device=DEV)
  got = _ffi.view_votes_accumulate(clu, crop, topk, ncls, flip, start.clone())
  ref32, ref64 = cpu_refs(clu, topk, case, start, 1)              # (the restatement drops those entries)
  assert_within_the_bound(got, ref32, ref64, 'labels >= ncls')
  sums = got.sum(0)
  assert sums.max().item() < 1.0 and sums.min().item() > 0.0
  inside = torch.where(topk < ncls, topk, torch.zeros_like(topk))  # the same rows with the outside labels as class 0 ...
  full = _ffi.view_votes_accumulate(clu, crop, inside, ncls, flip, start.clone())
  assert torch.equal(full[1:], got[1:])                            # ... change class 0 alone
  assert (full.sum(0) - 1.0).abs().max().item() <= 1e-5


def test_two_calls_are_bit_identical():
  case = KERNEL_CASES[2]
  ncls, _, _, crop, _, flip = case
  clu, topk, start = device_inputs(case, 960)
  first = _ffi.view_votes_accumulate(clu, crop, topk, ncls, flip, start.clone())
  again = _ffi.view_votes_accumulate(clu, crop, topk, ncls, flip, start.clone())
  was = _ffi.set_deterministic(True)
  try:
    third = _ffi.view_votes_accumulate(clu, crop, topk, ncls, flip, start.clone())
  finally:
    _ffi.set_deterministic(was)
  assert torch.equal(first, again) and torch.equal(first, third)


def test_argument_errors():
  """The entry's own checks, through the raw C call: nothing is launched for any of them."""
  lib = _ffi.lib()
  ncls, m, k, rh, rw, h, w = 5, 6, 20, 4, 5, 8, 10
  clu = torch.zeros(rh * rw, dtype=torch.int64, device=DEV)
  topk = torch.zeros((m, k), dtype=torch.int64, device=DEV)
  acc = torch.zeros((ncls, h, w), device=DEV)
  need = lib.spml_view_votes_workspace_bytes(m, ncls)
  ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  null = ctypes.c_void_p(0)
  pick = lambda given, tensor: P(tensor) if given is None else given      # (a null c_void_p is falsy)

  def call(clu_p=None, topk_p=None, acc_p=None, ws_p=None, ws_bytes=None, **sizes):
    s = dict(rh=rh, rw=rw, m=m, k=k, ncls=ncls, h=h, w=w)
    s.update(sizes)
    return lib.spml_view_votes_accumulate_f32(
        pick(clu_p, clu), s['rh'], s['rw'], pick(topk_p, topk), s['m'], s['k'], s['ncls'], 0, s['h'], s['w'],
        pick(acc_p, acc), pick(ws_p, ws), ws.numel() if ws_bytes is None else ws_bytes, _ffi.stream_ptr())

  INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
  assert call() == 0
  assert call(clu_p=null) == INVALID and call(topk_p=null) == INVALID and call(acc_p=null) == INVALID
  for name in ('rh', 'rw', 'm', 'k', 'ncls', 'h', 'w'):
    assert call(**{name: 0}) == INVALID and call(**{name: -3}) == INVALID, name
  assert call(acc_p=P(clu)) == INVALID and call(acc_p=P(topk)) == INVALID          # acc aliases an input
  assert call(acc_p=P(ws)) == INVALID and call(ws_p=P(topk)) == INVALID            # ... the workspace; ws an input
  assert call(ws_p=ctypes.c_void_p(ws.data_ptr() + 4)) == INVALID                  # a workspace off its 16-byte alignment
  assert call(ncls=65) == UNSUPPORTED and call(m=_ffi.MAX_VIEW_VOTES_SEGMENTS + 1) == UNSUPPORTED
  assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_p=null) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
  torch.cuda.synchronize()
  # the wrapper: shapes that do not fit, tensors on the CPU
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.view_votes_accumulate(clu, (rh, rw + 1), topk, ncls, 0, acc)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.view_votes_accumulate(clu, (rh, rw), topk, ncls + 1, 0, acc)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.view_votes_accumulate(clu, (rh, rw), topk.view(-1), ncls, 0, acc)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.view_votes_accumulate(clu, (rh, rw), torch.zeros((5000, k), dtype=torch.int64, device=DEV), ncls, 0, acc)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.view_votes_accumulate(clu.cpu(), (rh, rw), topk.cpu(), ncls, 0, acc.cpu())


def test_arg_max_resolves_ties_to_the_lowest_class():
  """`spml_argmax_channels_i64` gives the labels of :242 (`np.argmax`): exact ties -- votes are multiples of 1/k, so they
  do occur -- go to the lowest class, as numpy's."""
  gen = torch.Generator().manual_seed(3)
  prob = torch.randint(0, 4, (6, 9, 11), generator=gen).float() / 20.0
  want = np.argmax(prob.numpy(), axis=0)
  assert (np.sort(prob.numpy(), axis=0)[-1] == np.sort(prob.numpy(), axis=0)[-2]).mean() > 0.2     # many ties
  got = _ffi.argmax_channels(prob.to(DEV), 9, 11).cpu().numpy()
  assert np.array_equal(got, want)


def test_segment_predictions_are_what_predictions_gathers():
  """N1 fixture: `topk[clu]` of `segment_predictions` is the `semantic_score` of `predictions`, and both are the
  reference's."""
  from test_mirror_gpu import _cfg
  from spml_amd.models.predictions.segsort import Segsort
  g = load_golden('n1_predictions')
  model = Segsort(_cfg())
  datas = {'cluster_embedding': g.emb.to(DEV), 'cluster_index': g.clu.to(DEV)}
  targets = {'semantic_memory_prototype': g.bank.to(DEV), 'semantic_memory_prototype_label': g.bank_lab.to(DEV)}
  topk, clu = model.segment_predictions(datas, targets)
  pred, score = model.predictions(datas, targets)
  assert topk.dtype == clu.dtype == torch.int64 and topk.shape[1] == 20 and clu.shape == g.clu.shape
  assert int(clu.max()) + 1 == topk.shape[0] == g.clu.unique().numel()
  assert torch.equal(topk[clu], score) and torch.equal(score.cpu(), g.topk) and torch.equal(pred.cpu(), g.pred)
  assert model.segment_predictions({'cluster_embedding': g.emb.to(DEV)}, {}) == (None, None)


# ---------------------------------------------------------------------------
# predict_knn_multiscale against tests/golden/n9_knn_msc.npz
def check_labels(pred, g, ci, image_hw):
  t = 'c%d_' % ci
  sure = sure_pixels(g, ci)
  assert (~sure).float().mean().item() <= LOW_CAP
  assert pred.dtype == torch.int64 and tuple(pred.shape) == tuple(image_hw)
  assert torch.equal(pred.cpu()[sure], g[t + 'semantic_pred'].long()[sure])


@pytest.mark.parametrize('ci', [0, 1])
def test_tail_on_the_fixtures_own_segments_matches_reference_lines(ci):
  """The wrapper fed the fixture's own `cluster_index` and `topk` per view: `semantic_prob` within the kernel bound
  (4 x the error of the fp32 CPU restatement against the fp64 one), labels exact outside the low margin."""
  g = load_golden('n9_knn_msc')
  cfg, views = n9_case(g, ci)
  acc = torch.zeros((cfg['ncls'],) + cfg['image'], device=DEV)
  for v in views:
    _ffi.view_votes_accumulate(v['cluster_index'].to(DEV), v['crop_hw'], v['topk'].to(DEV), cfg['ncls'], v['flip'], acc)
  acc /= len(views)
  ref32, _ = restated_multiscale(views, cfg, torch.float32)
  ref64, _ = restated_multiscale(views, cfg, torch.float64)
  assert_within_the_bound(acc, ref32, ref64, 'n9 case %d, given segments' % ci)
  fix_err = (acc.cpu() - g['c%d_semantic_prob' % ci]).abs().max().item()
  print('against the stored semantic_prob: %.3e' % fix_err)
  check_labels(_ffi.argmax_channels(acc, *cfg['image']), g, ci, cfg['image'])


def fixture_models(g, ci, cfg):
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.train import voc12_scribble_config
  from test_inference_gpu import TinyEmbedder
  t = 'c%d_' % ci
  model = TinyEmbedder(cfg['c'], cfg['grid']).to(DEV)
  model.conv.load_state_dict({'weight': g[t + 'conv_w'].to(DEV), 'bias': g[t + 'conv_b'].to(DEV)})
  predictor = segsort(voc12_scribble_config()).to(DEV).eval()
  bank, bank_lab = inference.drop_ignored_memory(g[t + 'bank'].to(DEV), g[t + 'bank_lab'].to(DEV))
  return model, predictor, bank, bank_lab


@pytest.mark.parametrize('ci', [0, 1])
def test_multiscale_end_to_end_matches_reference_lines(ci):
  """Stub embedder and k-means on the GPU.  k-means near ties on a GPU convolution's output make exact equality the
  wrong demand (tests/test_stage2_gpu.py): the project's statistical bounds of the N5 test -- cluster maps agree on more
  than 0.97 of the pixels of every view, labels on more than 0.97 of the image."""
  g = load_golden('n9_knn_msc')
  cfg, views = n9_case(g, ci)
  model, predictor, bank, bank_lab = fixture_models(g, ci, cfg)
  out = inference.predict_knn_multiscale(model, predictor, [(v['image'].to(DEV), v['crop_hw'], v['flip']) for v in views],
                                         cfg['image'], cfg['crop'], cfg['stride'], bank, bank_lab, cfg['ncls'])
  assert out['combine_path'] == inference.HIP_VIEW_VOTES_PATH == 'hip_view_votes'
  prob, pred = out['semantic_prob'], out['semantic_prediction']
  assert tuple(prob.shape) == (cfg['ncls'],) + cfg['image'] and pred.dtype == torch.int64
  assert (prob.sum(0) - 1.0).abs().max().item() <= 1e-5
  for vi, v in enumerate(views):
    agree = (out['cluster_index'][vi].cpu() == v['cluster_index']).float().mean().item()
    print('case %d view %d: cluster maps agree on %.4f' % (ci, vi, agree))
    assert agree > 0.97, (vi, agree)
  agree = (pred.cpu() == g['c%d_semantic_pred' % ci].long()).float().mean().item()
  print('case %d: labels agree on %.4f' % (ci, agree))
  assert agree > 0.97, agree
  # ... and the tail on the segments this run found is the restatement's
  mine = [dict(v, cluster_index=out['cluster_index'][vi].cpu(), topk=out['segment_topk'][vi].cpu())
          for vi, v in enumerate(views)]
  assert_within_the_bound(prob, restated_multiscale(mine, cfg, torch.float32)[0],
                          restated_multiscale(mine, cfg, torch.float64)[0], 'n9 case %d, end to end' % ci)


def test_more_than_64_classes_take_the_framework_tail():
  """65 classes on a tiny image: `combine_path` names the framework ops, and the result agrees with the restatement on
  the segments the run found (the bound of the kernel tests)."""
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.train import voc12_scribble_config
  from test_inference_gpu import TinyEmbedder, blobs
  gen = torch.Generator().manual_seed(65)
  cfg = dict(ncls=65, image=(30, 37))
  model = TinyEmbedder(16, [3, 3]).to(DEV)
  predictor = segsort(voc12_scribble_config()).to(DEV).eval()
  bank = torch.nn.functional.normalize(torch.randn(90, 16, generator=gen), dim=1).to(DEV)
  bank_lab = torch.randint(0, 65, (90,), generator=gen).to(DEV)
  views = inference.flip_scale_views(blobs(gen, 30, 37).to(DEV), [0.75, 1.25], True, (24, 24))
  out = inference.predict_knn_multiscale(model, predictor, views, cfg['image'], (24, 24), (15, 15), bank, bank_lab, 65)
  assert out['combine_path'] == inference.FRAMEWORK_VIEW_VOTES_PATH == 'framework_view_votes'
  mine = [dict(crop_hw=hw, flip=flip, cluster_index=out['cluster_index'][vi].cpu(), topk=out['segment_topk'][vi].cpu())
          for vi, (_, hw, flip) in enumerate(views)]
  ref32, pred32 = restated_multiscale(mine, cfg, torch.float32)
  ref64, _ = restated_multiscale(mine, cfg, torch.float64)
  assert_within_the_bound(out['semantic_prob'], ref32, ref64, '65 classes, framework tail')
  top2 = ref32.topk(2, dim=0).values
  sure = (top2[0] - top2[1]) >= 2e-4 * ref32.abs().max()
  assert torch.equal(out['semantic_prediction'].cpu()[sure], pred32[sure])
  # the framework ops alone against the kernel, on a case both take
  case = KERNEL_CASES[0]
  clu, topk, start = device_inputs(case, 970)
  a = _ffi.view_votes_accumulate(clu, case[3], topk, case[0], case[5], start.clone())
  b = inference.framework_view_votes_accumulate(clu, case[3], topk, case[0], case[5], start.clone())
  ref32, ref64 = cpu_refs(clu, topk, case, start, 1)
  assert_within_the_bound(a, ref32, ref64, 'kernel')
  assert_within_the_bound(b, ref32, ref64, 'framework ops')


def test_entry_point_builds_its_bank_and_writes_label_maps(tmp_path, capsys, monkeypatch):
  """pyscripts/inference/inference_msc.py end to end on a tiny config: a two-class snapshot written here, crop 65, two
  synthetic images, ten views each; without --semantic_memory_dir it builds the bank from the synthetic images, writes it
  in the reference's format and loads it back from those files."""
  import json
  import os
  from test_train_cli import YAML
  import spml_amd.utils.segsort.others as segsort_others
  from spml_amd import inference_cli
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101').replace('num_classes: 21', 'num_classes: 2')
          .replace('image_size: 97', 'image_size: 65').replace('- 97', '- 65'))
  yaml = yaml.replace('stride:\n    - 65\n    - 65', 'stride:\n    - 43\n    - 43')
  assert 'num_classes: 2' in yaml and yaml.count('- 65') == 4 and yaml.count('- 43') == 2
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(yaml)
  from spml_amd.config.default import config, update_config
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  from spml_amd.models.predictions.segsort import segsort
  update_config(str(cfg))
  torch.manual_seed(9)
  snap = tmp_path / 'snapshot'
  os.makedirs(str(snap))
  torch.save({'embedding_model': resnet_101_deeplab(config).state_dict(), 'prediction_model': segsort(config).state_dict()},
             str(snap / 'model-{:d}.pth'.format(config.train.max_iteration - 1)))
  prog = load_program()
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  save = tmp_path / 'results'
  capsys.readouterr()
  prog.main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic',
             '--kmeans_num_clusters', '4,4', '--label_divisor', '2048'])
  line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
  result = json.loads(line)
  for key in ('images', 'images_per_s', 'mIoU', 'pixel_acc', 'views', 'combine_path', 'memory_prototypes', 'snapshot',
              'semantic_memory_dir', 'save_dir'):
    assert key in result, key
  assert result['images'] == 2 and result['images_per_s'] > 0 and 0.0 <= result['mIoU'] <= 100.0
  assert result['views'] == 10 and result['combine_path'] == 'hip_view_votes'
  maps = sorted(os.listdir(str(save / 'semantic_gray')))
  assert maps == ['synthetic_0000.npy', 'synthetic_0001.npy']
  label = np.load(str(save / 'semantic_gray' / maps[0]))
  assert label.dtype == np.uint8 and label.shape == (65, 65) and label.max() < 2
  # the bank it retrieved from is the one on disk, in the reference's format
  assert result['semantic_memory_dir'] == str(save / 'semantic_prototype')
  assert sorted(os.listdir(result['semantic_memory_dir'])) == maps
  protos, labels = segsort_others.load_memory_banks(result['semantic_memory_dir'])
  kept = int((labels != 255).sum())
  assert result['memory_prototypes'] == kept >= 20 and protos.shape == (labels.shape[0], 32)
