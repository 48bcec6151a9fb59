"""Tag-recipe kNN pseudo labels on the GPU: the tag-normalised arg-max of csrc/tag_normalize.hip alone against the same
chain of torch ops on the CPU (bit for bit: both are one IEEE division by the view count, an exact maximum and one IEEE
division), then with the vote-view kernel in front of it against the fixture exec'd from the reference's own lines
(tests/golden/n11_pseudo_knn_msc.npz; tests/test_pseudo_knn_msc.py keeps that fixture honest on the CPU),
`pseudo_labels_knn_multiscale` end to end, its framework tail above 64 classes, the helper it shares with
`predict_knn_multiscale`, and the program.  Measured figures: profiles/pseudo_knn_msc.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from spml_amd import _ffi, inference
from test_knn_msc import LOW_CAP, n9_case
from test_knn_msc_gpu import assert_within_the_bound, fixture_models
from test_pseudo_knn_msc import FLOOR, load_program, n11_case, restated_sum, restated_tag_tail, sure_pixels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32

# (ncls, h, w, V)
KERNEL_CASES = [
    (1, 1, 1, 1),                # smallest
    (5, 44, 60, 8),              # fixture-like
    (21, 37, 53, 10),            # odd n, a V that is no power of two
    (64, 7, 5, 3),               # the largest class count, n below one wave
    (15, 1, 4099, 6),            # one long row across chunk borders
    (21, 300, 333, 8),           # several workgroups per class meet
    (2, 513, 513, 8)]
KINDS = ('exact', 'untagged', 'weak', 'negative', 'zero')      # the classes 0 .. 4 of every shape with more than 2 classes


def sum_that_divides_to(value, v):
  """An fp32 `a` with fl(a / v) == value: the quotients of consecutive floats near value * v are closer together than
  the floats near value, so one of the neighbours of fl(value * v) hits it."""
  a = F32(value) * F32(v)
  for cand in [a] + [np.nextafter(a, F32(s * np.inf), dtype=F32) for s in (1, -1)]:
    if F32(cand) / F32(v) == F32(value):
      return float(cand)
  lo, hi = a, a
  for _ in range(8):
    lo, hi = np.nextafter(lo, F32(-np.inf), dtype=F32), np.nextafter(hi, F32(np.inf), dtype=F32)
    for cand in (lo, hi):
      if F32(cand) / F32(v) == F32(value):
        return float(cand)
  raise AssertionError('no fp32 sum divides by %d to %r' % (v, value))


def make_case(case, seed):
  """-> (acc [ncls,h,w] fp32 on the CPU: the SUM over V views, tags bool [ncls], the pixel of every class's peak, kinds).
  The peak of class c is planted at pixel (c * 2654435761) mod n -- class 0 at pixel 0 -- and the last class's at n - 1,
  so a lost head, tail or part shows.  With more than two classes the classes 0 .. 4 are: a peak of exactly
  float32(0.15), an untagged class with a peak of 0.5, a tagged class with a peak of 0.1, a tagged class whose values
  are all negative, an all-zero tagged class; the others have peaks of 0.6 and more over values below 0.3, and every
  third of them is untagged."""
  ncls, h, w, v = case
  n = h * w
  gen = torch.Generator().manual_seed(seed)
  acc = torch.rand((ncls, n), generator=gen) * (0.3 * v)
  tags = torch.tensor([c % 3 != 2 for c in range(ncls)])
  kinds = ['normal'] * ncls
  if ncls > 2:
    kinds[:5] = KINDS
  where = [(c * 2654435761) % n for c in range(ncls)]
  where[-1] = n - 1
  for c, kind in enumerate(kinds):
    tags[c] = {'normal': bool(tags[c]), 'untagged': False}.get(kind, True)
    if kind == 'normal':
      acc[c, where[c]] = (0.6 + 0.3 * c / ncls) * v
    elif kind == 'exact':
      acc[c] *= 0.3                                            # (values below 0.09 * v)
      acc[c, where[c]] = sum_that_divides_to(F32(0.15), v)
    elif kind == 'untagged':
      acc[c, where[c]] = 0.5 * v
    elif kind == 'weak':
      acc[c] *= 0.1                                            # (values below 0.03 * v)
      acc[c, where[c]] = 0.1 * v
    elif kind == 'negative':
      acc[c] = -acc[c] - 0.01 * v
      acc[c, where[c]] = -0.005 * v
    else:
      acc[c] = 0.0
  return acc.view(ncls, h, w).contiguous(), tags, where, kinds


@functools.lru_cache(maxsize=None)
def kernel_case(index):
  """One kernel case, computed once: the kernel's outputs and the framework ops' on the CPU, given the same fp32 sum."""
  case = KERNEL_CASES[index]
  acc, tags, where, kinds = make_case(case, 1100 + index)
  dev_acc = acc.to(DEV)
  labels, prob, divisor = _ffi.tag_normalize_argmax(dev_acc, case[3], tags.to(DEV), FLOOR, want_prob=True)
  ref_labels, ref_prob, ref_divisor = inference.framework_tag_normalize_argmax(acc, case[3], tags, FLOOR, want_prob=True)
  return dict(acc=acc, tags=tags, where=where, kinds=kinds, acc_after=dev_acc.cpu(), labels=labels.cpu(), prob=prob.cpu(),
              divisor=divisor.cpu(), ref_labels=ref_labels, ref_prob=ref_prob, ref_divisor=ref_divisor)


@pytest.mark.parametrize('index', range(len(KERNEL_CASES)))
def test_kernel_is_the_framework_ops_bit_for_bit(index):
  case, r = KERNEL_CASES[index], kernel_case(index)
  ncls, h, w, v = case
  assert r['labels'].dtype == torch.int64 and tuple(r['labels'].shape) == (h, w)
  assert tuple(r['prob'].shape) == (ncls, h, w) and tuple(r['divisor'].shape) == (ncls,)
  diff = (r['prob'] - r['ref_prob']).abs().max().item()
  wrong = (r['labels'] != r['ref_labels']).sum().item()
  print('%r: divisor %s, max |prob - CPU ops| %.3e, %d labels differ' % (case, r['divisor'].tolist()[:6], diff, wrong))
  assert torch.equal(r['divisor'], r['ref_divisor'])
  assert torch.equal(r['prob'], r['ref_prob'])
  assert torch.equal(r['labels'], r['ref_labels'])
  assert torch.equal(r['acc_after'], r['acc'])                # the sum is only read
  # the divisors are the planted peaks: a lost head, tail or part would give a smaller one
  floor = torch.tensor(FLOOR)
  mean_peak = torch.stack([r['acc'].view(ncls, -1)[c, p] for c, p in enumerate(r['where'])]) / torch.tensor(float(v))
  for c, kind in enumerate(r['kinds']):
    if kind in ('weak', 'negative', 'zero', 'exact'):
      assert r['divisor'][c] == floor, (c, kind)
    elif kind == 'untagged' or not r['tags'][c]:
      assert r['divisor'][c] == 1.0, (c, kind)
    else:
      assert r['divisor'][c] == mean_peak[c] > floor, (c, kind)
    if kind == 'exact':
      assert mean_peak[c] == floor                             # the peak is float32(0.15) itself
    if kind not in ('zero',) and r['tags'][c] and r['divisor'][c] > floor:
      assert r['prob'].view(ncls, -1)[c, r['where'][c]] == 1.0   # a tagged class above the floor peaks at exactly 1


def raw_call(acc, num_views, tags8, floor=FLOOR, labels=None, prob=None, divisor=None, ws=None, ws_bytes=None, ncls=None,
             n=None, acc_p=None, tags_p=None, labels_p=None, ws_p=None):
  """spml_tag_normalize_argmax_f32 through ctypes: every pointer can be replaced (`*_p`) or left out (None -> NULL for
  prob and divisor)."""
  lib = _ffi.lib()
  P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
  pick = lambda given, tensor: P(tensor) if given is None else given
  return lib.spml_tag_normalize_argmax_f32(
      pick(acc_p, acc), acc.shape[0] if ncls is None else ncls, acc[0].numel() if n is None else n, num_views,
      pick(tags_p, tags8), floor, pick(labels_p, labels), P(prob), P(divisor), pick(ws_p, ws),
      ws.numel() if ws_bytes is None else ws_bytes, _ffi.stream_ptr())


def test_null_outputs_nan_workspace_repeat_and_deterministic_mode():
  """prob = NULL and divisor = NULL give the same labels; a workspace of NaN bytes changes nothing; two calls, and a call
  in the deterministic mode, are bit-identical."""
  index = 2
  case, r = KERNEL_CASES[index], kernel_case(index)
  ncls, h, w, v = case
  acc, tags8 = r['acc'].to(DEV), r['tags'].to(DEV).view(torch.uint8)
  need = _ffi.lib().spml_tag_normalize_workspace_bytes(ncls, h * w)
  assert need > 0

  def run(want_prob, want_divisor, fill):
    ws = torch.full((need + 16,), fill, dtype=torch.uint8, device=DEV)
    labels = torch.full((h, w), -1, dtype=torch.int64, device=DEV)
    prob = torch.full((ncls, h, w), -7.0, device=DEV) if want_prob else None
    divisor = torch.full((ncls,), -7.0, device=DEV) if want_divisor else None
    assert raw_call(acc, v, tags8, labels=labels, prob=prob, divisor=divisor, ws=ws) == 0
    return labels.cpu(), None if prob is None else prob.cpu(), None if divisor is None else divisor.cpu()

  full = run(True, True, 0)
  assert torch.equal(full[0], r['labels']) and torch.equal(full[1], r['prob']) and torch.equal(full[2], r['divisor'])
  for want_prob, want_divisor in ((False, True), (True, False), (False, False)):
    got = run(want_prob, want_divisor, 0)
    assert torch.equal(got[0], r['labels'])
    assert got[1] is None or torch.equal(got[1], r['prob'])
    assert got[2] is None or torch.equal(got[2], r['divisor'])
  nan_ws = run(True, True, 0xFF)                               # 0xFFFFFFFF is a NaN
  assert all(torch.equal(a, b) for a, b in zip(nan_ws, full))
  was = _ffi.set_deterministic(True)
  try:
    det = run(True, True, 0)
  finally:
    _ffi.set_deterministic(was)
  assert all(torch.equal(a, b) for a, b in zip(det, full))
  assert torch.equal(acc.cpu(), r['acc'])


def test_ties_go_to_the_lowest_class():
  """Votes are multiples of 1/20, so equal values do occur: untagged classes over a handful of values tie on most pixels,
  and two tagged classes with one plane normalise to the same map and tie everywhere.  np.argmax's rule."""
  gen = torch.Generator().manual_seed(5)
  acc = torch.randint(0, 4, (6, 9, 11), generator=gen).float() / 20.0 * 8.0
  acc[4] = acc[2]
  tags = torch.tensor([False, False, True, False, True, False])
  ref_labels, ref_prob, _ = inference.framework_tag_normalize_argmax(acc, 8, tags, FLOOR, want_prob=True)
  top2 = np.sort(ref_prob.numpy(), axis=0)[-2:]
  assert (top2[0] == top2[1]).mean() > 0.2                     # many ties
  assert np.array_equal(ref_labels.numpy(), np.argmax(ref_prob.numpy(), axis=0))
  labels, prob, _ = _ffi.tag_normalize_argmax(acc.to(DEV), 8, tags.to(DEV), FLOOR, want_prob=True)
  assert torch.equal(prob.cpu(), ref_prob) and torch.equal(prob[4], prob[2])
  assert np.array_equal(labels.cpu().numpy(), np.argmax(ref_prob.numpy(), axis=0))
  assert not (labels == 4).any() and (labels == 2).any()
  zeros, all_tags = torch.zeros((5, 3, 4), device=DEV), torch.ones(5, dtype=torch.bool, device=DEV)
  assert not _ffi.tag_normalize_argmax(zeros, 3, all_tags)[0].any()            # all equal: class 0
  assert not _ffi.tag_normalize_argmax(-zeros, 3, all_tags)[0].any()           # (negative zeros too)


def test_offsets_beyond_32_bits():
  """64 class planes of 2^25 + 2^20 + 3 pixels: the last plane starts more than 2^31 elements into the sum, past what a
  32-bit element index holds, and its byte offsets are past 2^33.  The sum is zero but for two planted votes in untagged
  classes (so nothing on the CPU has to walk 8.9 GB): the labels are 0 but for those two pixels."""
  ncls, n = 64, (1 << 25) + (1 << 20) + 3
  assert (ncls - 1) * n > (1 << 31)
  acc = torch.zeros((ncls, 1, n), device=DEV)
  acc[63, 0, n - 1] = 4.0
  acc[40, 0, 12345] = 2.0
  tags = torch.zeros(ncls, dtype=torch.bool, device=DEV)
  tags[7] = True
  labels, prob, divisor = _ffi.tag_normalize_argmax(acc, 4, tags, FLOOR)
  assert prob is None and int(torch.count_nonzero(labels)) == 2
  assert int(labels[0, n - 1]) == 63 and int(labels[0, 12345]) == 40
  want = torch.ones(ncls)
  want[7] = FLOOR
  assert torch.equal(divisor.cpu(), want)
  tags[63] = True                                              # ... and the peak of the last plane is found
  labels, _, divisor = _ffi.tag_normalize_argmax(acc, 4, tags, FLOOR)
  assert float(divisor[63]) == 1.0 and int(labels[0, n - 1]) == 63 and int(torch.count_nonzero(labels)) == 2


def test_argument_errors():
  """The entry's own checks, through the raw C call: nothing is launched for any of them."""
  lib = _ffi.lib()
  ncls, h, w, v = 5, 6, 7, 8
  acc = torch.rand((ncls, h, w), device=DEV)
  tags8 = torch.ones(16, dtype=torch.uint8, device=DEV)
  labels = torch.zeros((h, w), dtype=torch.int64, device=DEV)
  prob, divisor = torch.zeros_like(acc), torch.zeros(ncls, device=DEV)
  need = lib.spml_tag_normalize_workspace_bytes(ncls, h * w)
  ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  null = ctypes.c_void_p(0)
  call = lambda **kw: raw_call(acc, kw.pop('num_views', v), tags8, **dict(dict(labels=labels, prob=prob, divisor=divisor,
                                                                            ws=ws), **kw))
  INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
  assert call() == 0
  torch.cuda.synchronize()
  untouched = [t.clone() for t in (labels, prob, divisor)]
  assert call(acc_p=null) == INVALID and call(tags_p=null) == INVALID and call(labels_p=null) == INVALID
  for name in ('n', 'ncls', 'num_views'):
    assert call(**{name: 0}) == INVALID and call(**{name: -3}) == INVALID, name
  for floor in (0.0, -0.15, float('inf'), float('nan')):
    assert call(floor=floor) == INVALID, floor
  # outputs that alias the sum, the tags, the workspace or each other
  assert call(labels_p=P(acc)) == INVALID and call(prob=acc) == INVALID and call(divisor=acc) == INVALID
  assert call(ws_p=P(acc)) == INVALID and call(divisor=tags8.view(torch.float32)) == INVALID
  assert call(labels_p=P(ws)) == INVALID and call(prob=ws.view(torch.float32)) == INVALID
  assert call(labels_p=P(prob)) == INVALID and call(divisor=prob) == INVALID and call(divisor=labels) == INVALID
  assert call(ncls=65) == UNSUPPORTED and call(n=(1 << 30) + 1) == UNSUPPORTED
  assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_p=null) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
  assert call(ws_p=ctypes.c_void_p(ws.data_ptr() + 2)) == WORKSPACE             # a workspace off its 4-byte alignment
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(untouched, (labels, prob, divisor)))
  # the wrapper: shapes that do not fit, a class count outside the kernel, tensors on the CPU
  tags = torch.ones(ncls, dtype=torch.bool, device=DEV)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.tag_normalize_argmax(acc, v, tags[:4])
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.tag_normalize_argmax(acc[0], v, tags)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.tag_normalize_argmax(acc, v, tags.float())
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.tag_normalize_argmax(torch.zeros((65, 2, 2), device=DEV), v, torch.ones(65, dtype=torch.bool, device=DEV))
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.tag_normalize_argmax(acc.cpu(), v, tags.cpu())
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.tag_normalize_argmax(acc, 0, tags)


# ---------------------------------------------------------------------------
# with the vote-view kernel in front: tests/golden/n11_pseudo_knn_msc.npz
def restated_refs(views, cfg, tags):
  """(prob fp32, prob fp64, labels of the fp32 chain) of the restated per-view tails and the restated tag tail."""
  p32, _, labels = restated_tag_tail(restated_sum(views, cfg, torch.float32), len(views), tags, torch.float32)
  p64, _, _ = restated_tag_tail(restated_sum(views, cfg, torch.float64), len(views), tags, torch.float64)
  return p32, p64, labels


@pytest.mark.parametrize('ci', [0, 1])
def test_tail_on_the_fixtures_own_segments_matches_reference_lines(ci):
  """Both kernels fed the fixture's own `cluster_index` and `topk` per view: the normalised `semantic_prob` within the N9
  bound (4 x the error of the fp32 CPU restatement against the fp64 one, on this case), labels exact where the margin is
  sure, and at most 1 % of the pixels are not."""
  g = load_golden('n11_pseudo_knn_msc')
  cfg, views = n11_case(g, ci)
  t = 'c%d_' % ci
  tags = g[t + 'label_tags']
  acc = torch.zeros((cfg['ncls'],) + cfg['image'], device=DEV)
  for v in views:
    _ffi.view_votes_accumulate(v['cluster_index'].to(DEV), v['crop_hw'], v['topk'].to(DEV), cfg['ncls'], v['flip'], acc)
  labels, prob, divisor = _ffi.tag_normalize_argmax(acc, len(views), tags.to(DEV), FLOOR, want_prob=True)
  ref32, ref64, _ = restated_refs(views, cfg, tags)
  assert_within_the_bound(prob, ref32, ref64, 'n11 case %d, given segments' % ci)
  print('against the stored semantic_prob: %.3e; divisor %s (stored %s)'
        % ((prob.cpu() - g[t + 'semantic_prob']).abs().max().item(), divisor.tolist(), g[t + 'divisor'].tolist()))
  sure = sure_pixels(g, ci)
  assert (~sure).float().mean().item() <= LOW_CAP
  assert torch.equal(labels.cpu()[sure], g[t + 'semantic_pred'].long()[sure])


@pytest.mark.parametrize('ci', [0, 1])
def test_end_to_end_matches_reference_lines(ci):
  """Stub embedder and k-means on the GPU, the project's statistical bounds of the N5 test: cluster maps agree on more
  than 0.97 of the pixels of every view, labels on more than 0.97 of the image; and the tail on the segments this run
  found is within the N9 bound of the restatement."""
  g = load_golden('n11_pseudo_knn_msc')
  cfg, views = n11_case(g, ci)
  t = 'c%d_' % ci
  tags = g[t + 'label_tags']
  model, predictor, bank, bank_lab = fixture_models(g, ci, cfg)
  out = inference.pseudo_labels_knn_multiscale(
      model, predictor, [(v['image'].to(DEV), v['crop_hw'], v['flip']) for v in views], cfg['image'], cfg['crop'],
      cfg['stride'], bank, bank_lab, cfg['ncls'], tags.to(DEV), floor=FLOOR, return_prob=True)
  assert out['normalize_path'] == inference.HIP_TAG_NORMALIZE_PATH == 'hip_tag_normalize'
  assert out['combine_path'] == 'hip_view_votes'
  assert set(out) == {'semantic_prediction', 'semantic_prob', 'class_divisor', 'combine_path', 'normalize_path',
                      'cluster_index', 'segment_topk'}
  prob, pred = out['semantic_prob'], out['semantic_prediction']
  assert tuple(prob.shape) == (cfg['ncls'],) + cfg['image'] and pred.dtype == torch.int64
  assert tuple(out['class_divisor'].shape) == (cfg['ncls'],)
  for vi, v in enumerate(views):
    agree = (out['cluster_index'][vi].cpu() == v['cluster_index']).float().mean().item()
    print('case %d view %d: cluster maps agree on %.4f' % (ci, vi, agree))
    assert agree > 0.97, (vi, agree)
  agree = (pred.cpu() == g[t + 'semantic_pred'].long()).float().mean().item()
  print('case %d: labels agree on %.4f' % (ci, agree))
  assert agree > 0.97, agree
  mine = [dict(v, cluster_index=out['cluster_index'][vi].cpu(), topk=out['segment_topk'][vi].cpu())
          for vi, v in enumerate(views)]
  ref32, ref64, _ = restated_refs(mine, cfg, tags)
  assert_within_the_bound(prob, ref32, ref64, 'n11 case %d, end to end' % ci)
  # without return_prob the map is not written, and the labels are the same
  again = inference.pseudo_labels_knn_multiscale(
      model, predictor, [(v['image'].to(DEV), v['crop_hw'], v['flip']) for v in views], cfg['image'], cfg['crop'],
      cfg['stride'], bank, bank_lab, cfg['ncls'], tags.to(DEV))
  assert again['semantic_prob'] is None and torch.equal(again['semantic_prediction'], pred)


def test_more_than_64_classes_take_the_framework_tail():
  """65 classes on a tiny image: `normalize_path` names the framework ops, and the result agrees with the restatement on
  the segments the run found."""
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.train import voc12_scribble_config
  from test_inference_gpu import TinyEmbedder, blobs
  gen = torch.Generator().manual_seed(65)
  cfg = dict(ncls=65, image=(30, 37))
  model = TinyEmbedder(16, [3, 3]).to(DEV)
  predictor = segsort(voc12_scribble_config()).to(DEV).eval()
  bank = torch.nn.functional.normalize(torch.randn(90, 16, generator=gen), dim=1).to(DEV)
  bank_lab = torch.randint(0, 65, (90,), generator=gen).to(DEV)
  tags = torch.rand(65, generator=gen) < 0.5
  views = inference.flip_scale_views(blobs(gen, 30, 37).to(DEV), [0.5, 1.5], True, (24, 24))
  out = inference.pseudo_labels_knn_multiscale(model, predictor, views, cfg['image'], (24, 24), (15, 15), bank, bank_lab,
                                               65, tags.to(DEV), return_prob=True)
  assert out['normalize_path'] == inference.FRAMEWORK_TAG_NORMALIZE_PATH == 'framework_tag_normalize'
  assert out['combine_path'] == 'framework_view_votes'
  mine = [dict(crop_hw=hw, flip=flip, cluster_index=out['cluster_index'][vi].cpu(), topk=out['segment_topk'][vi].cpu())
          for vi, (_, hw, flip) in enumerate(views)]
  ref32, ref64, pred32 = restated_refs(mine, cfg, tags)
  assert_within_the_bound(out['semantic_prob'], ref32, ref64, '65 classes, framework tail')
  top2 = ref32.topk(2, dim=0).values
  sure = (top2[0] - top2[1]) >= 2e-4 * ref32.abs().max()
  assert torch.equal(out['semantic_prediction'].cpu()[sure], pred32[sure])
  # the framework ops on the device against the kernel, on a case both take: the kernel's bits or the N9 bound
  r = kernel_case(1)
  _, prob, divisor = inference.framework_tag_normalize_argmax(r['acc'].to(DEV), KERNEL_CASES[1][3], r['tags'].to(DEV),
                                                              FLOOR, want_prob=True)
  assert torch.allclose(prob.cpu(), r['prob'], rtol=1e-6, atol=0) and torch.allclose(divisor.cpu(), r['divisor'], rtol=1e-6)


@pytest.mark.parametrize('ci', [0, 1])
def test_shared_helper_leaves_predict_knn_multiscale_as_it_was(ci):
  """An n9 case through both entries: with no class tagged every divisor is 1, so the normalised map times the divisor is
  the un-normalised mean -- bit for bit the `semantic_prob` of `predict_knn_multiscale` (2 and 4 views: the division by
  the view count is exact either way), with the same labels, segments and retrievals."""
  g = load_golden('n9_knn_msc')
  cfg, views = n9_case(g, ci)
  model, predictor, bank, bank_lab = fixture_models(g, ci, cfg)
  dev_views = [(v['image'].to(DEV), v['crop_hw'], v['flip']) for v in views]
  args = (model, predictor, dev_views, cfg['image'], cfg['crop'], cfg['stride'], bank, bank_lab, cfg['ncls'])
  plain = inference.predict_knn_multiscale(*args)
  assert set(plain) == {'semantic_prob', 'semantic_prediction', 'combine_path', 'cluster_index', 'segment_topk'}
  tags = torch.zeros(cfg['ncls'], dtype=torch.bool, device=DEV)
  out = inference.pseudo_labels_knn_multiscale(*args, tags, return_prob=True)
  assert torch.equal(out['class_divisor'], torch.ones(cfg['ncls'], device=DEV))
  assert torch.equal(out['semantic_prob'] * out['class_divisor'].view(-1, 1, 1), plain['semantic_prob'])
  assert torch.equal(out['semantic_prediction'], plain['semantic_prediction'])
  assert all(torch.equal(a, b) for a, b in zip(out['cluster_index'], plain['cluster_index']))
  assert all(torch.equal(a, b) for a, b in zip(out['segment_topk'], plain['segment_topk']))
  assert (plain['semantic_prob'].sum(0) - 1.0).abs().max().item() <= 1e-5


def test_entry_point_builds_its_bank_and_writes_label_maps(tmp_path, capsys):
  """pyscripts/inference/pseudo_inference_msc.py end to end on a tiny config: a two-class snapshot written here (two
  steps of nothing: freshly initialised weights under the name of step 2), crop 65, four synthetic images, eight views
  each; without --semantic_memory_dir it builds the bank from the synthetic images first."""
  import json
  import os
  from test_train_cli import YAML
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
  assert inference_cli.NUM_SYNTHETIC_IMAGES == 4
  save = tmp_path / 'results'
  capsys.readouterr()
  prog.main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic',
             '--kmeans_num_clusters', '4,4', '--label_divisor', '2048'])
  lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
  assert len(lines) == 1
  result = json.loads(lines[0])
  for key in ('images', 'images_per_s', 'mIoU', 'pixel_acc', 'instance_mIoU', 'views', 'combine_path', 'normalize_path',
              'memory_prototypes', 'snapshot', 'semantic_memory_dir', 'save_dir'):
    assert key in result, key
  assert result['images'] == 4 and result['images_per_s'] > 0
  assert np.isfinite(result['mIoU']) and np.isfinite(result['instance_mIoU'])
  assert 0.0 <= result['mIoU'] <= 100.0 and 0.0 <= result['instance_mIoU'] <= 100.0
  assert result['views'] == 8 and result['combine_path'] == 'hip_view_votes'
  assert result['normalize_path'] == 'hip_tag_normalize'
  maps = sorted(os.listdir(str(save / 'semantic_gray')))
  assert maps == ['synthetic_%04d.npy' % i for i in range(4)]
  label = np.load(str(save / 'semantic_gray' / maps[0]))
  assert label.dtype == np.uint8 and label.shape == (65, 65) and label.max() < 2
  assert result['semantic_memory_dir'] == str(save / 'semantic_prototype')
  assert sorted(os.listdir(result['semantic_memory_dir'])) == maps
