"""The fused segment-votes + dense-CRF call on the GPU (crf_votes_table and crf_init_votes of csrc/dense_crf.hip through
spml_amd.models.crf.DenseCRF.infer_votes) against the yardsticks of tests/knn_crf_ref.py: the vote map, the
label before the CRF, marginals and labels against the fp64 oracle, bit-identity with the two-step path, ties, foreign
labels, the limits and the argument errors, the framework route, and the three programs end to end.  Measured figures and
how the bounds follow from them: profiles/knn_crf.md."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import dense_crf_ref
import knn_crf_ref as ref
from spml_amd import _ffi, inference, inference_cli
from spml_amd.models.crf import DenseCRF
from test_dense_crf_gpu import on_device, tiny_config, write_snapshot
from test_inference_cli import load_program

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = ref.SEED
IDS = dict(ids=lambda s: '%dx%dx%d' % s)
PARAMETERS = ['defaults', 'alternative']

# max |Q - fp64 oracle|: 4 x the largest deviation measured on one MI355X over the shape list, both parameter sets and
# seeds 1-3 (Q_MEASURED: profiles/knn_crf.md; the factor is for the summation order, as in test_dense_crf_gpu.py), never
# above 5e-4.  The largest value is (17, 129, 64), defaults, seed 3; seed 1, which runs here, stays below 1.5e-6.  The
# framework route (4100 segments) and the driver on a stub embedder measured 1.1e-6 and 1.3e-6 under the same bound.
Q_MEASURED = 1.7251e-6
Q_BOUND = min(4 * Q_MEASURED, 5e-4)
# max |Q of the fused call - Q of spml_dense_crf_infer_f32 on the fused call's own vote map|, without and with iterations:
# measured 0 (bit-identical, labels included) on all 54 cases of the list above, so the comparison is for equality.
TWO_STEP_MEASURED = 0.0


def params(parameters, **changes):
  return dict(dense_crf_ref.PARAMETER_SETS[parameters], **changes)


@functools.lru_cache(maxsize=None)
def fused_case(shape, parameters, seed=SEED):
  """(Q, labels, labels_before, prob) of the fused call on one case of the yardstick, as numpy arrays; computed once."""
  image, clu, topk, _, _ = ref.yardstick(shape, parameters, seed)
  crf = DenseCRF(**params(parameters))
  ws = crf.prepare(on_device(image), shape[2])
  out = crf.infer_votes(ws, on_device(clu), on_device(topk), shape[2], shape[:2], want_prob=True)
  return tuple(o.cpu().numpy() for o in out)


# ---------------------------------------------------------------------------
# 1. the vote map and the label before the CRF
@pytest.mark.parametrize('parameters', PARAMETERS)
@pytest.mark.parametrize('shape', ref.SHAPES, **IDS)
def test_prob_is_the_vote_map_bit_for_bit_and_labels_before_its_argmax(shape, parameters):
  _, _, _, votes, _ = ref.yardstick(shape, parameters)
  _, _, before, prob = fused_case(shape, parameters)
  assert prob.dtype == np.float32 and prob.shape == votes.shape and np.array_equal(prob, votes)
  assert before.dtype == np.int64 and np.array_equal(before, np.argmax(votes, 0))


# 2. + 3. marginals and labels against the fp64 yardstick
@pytest.mark.parametrize('parameters', PARAMETERS)
@pytest.mark.parametrize('shape', ref.SHAPES, **IDS)
def test_marginals_and_labels_against_the_fp64_yardstick(shape, parameters):
  _, _, _, votes, want = ref.yardstick(shape, parameters)
  got, labels, before, _ = fused_case(shape, parameters)
  what = '%s %s' % (shape, parameters)
  dev = float(np.abs(got.astype(np.float64) - want).max())
  print('%s: max |Q - yardstick| = %.3e (bound %.2e)' % (what, dev, Q_BOUND))
  assert got.dtype == np.float32 and got.shape == want.shape
  assert np.abs(got.sum(0) - 1.0).max() <= 1e-5
  assert np.array_equal(labels, got.argmax(0)), what + ': the fused arg-max is not the arg-max of the returned Q'
  assert dev <= Q_BOUND, (what, dev)
  keep, left_out = ref.under_margin(want)
  print('%s: %.4f of the pixels under the margin (cap %.2f)' % (what, left_out, ref.LABEL_CAP))
  assert left_out <= ref.LABEL_CAP, (what, left_out)
  assert np.array_equal(labels[keep], want.argmax(0)[keep]), what
  if shape in ((16, 24, 2), (33, 47, 5)):
    assert (labels != before).any(), 'the CRF changed no label: the result may be the input'
  if shape == (9, 9, 1):
    assert np.array_equal(got, np.ones((1, 9, 9), np.float32)) and not labels.any() and not before.any()


# 4. the fused path is the two-step path
@pytest.mark.parametrize('parameters', PARAMETERS)
@pytest.mark.parametrize('shape', ref.SHAPES, **IDS)
def test_fused_call_equals_infer_on_its_own_vote_map(shape, parameters):
  image, clu, topk, _, _ = ref.yardstick(shape, parameters)
  clu_d, topk_d = on_device(clu), on_device(topk)
  for iter_max in (0, dense_crf_ref.PARAMETER_SETS[parameters]['iter_max']):
    crf = DenseCRF(**params(parameters, iter_max=iter_max))
    ws = crf.prepare(on_device(image), shape[2])
    q, labels, before, prob = crf.infer_votes(ws, clu_d, topk_d, shape[2], shape[:2], want_prob=True)
    q_two, labels_two = crf.infer(ws, prob)
    diff = float((q - q_two).abs().max())
    print('%s %s iter_max=%d: max |fused - two-step| = %.3e' % (shape, parameters, iter_max, diff))
    assert torch.equal(q, q_two) and torch.equal(labels, labels_two), (shape, parameters, iter_max, diff)
    if iter_max:
      assert np.array_equal(q.cpu().numpy(), fused_case(shape, parameters)[0])


def test_two_calls_are_bit_identical_and_the_optional_outputs_change_nothing():
  shape = (33, 47, 5)
  image, clu, topk, _, _ = ref.yardstick(shape, 'defaults')
  crf = DenseCRF(**params('defaults'))
  ws = crf.prepare(on_device(image), 5)
  clu_d, topk_d = on_device(clu), on_device(topk)
  first = crf.infer_votes(ws, clu_d, topk_d, 5, shape[:2], want_prob=True)
  again = crf.infer_votes(ws, clu_d, topk_d, 5, shape[:2], want_prob=True)
  assert all(torch.equal(a, b) for a, b in zip(first, again))
  q_bare, labels_bare, none_before, none_prob = crf.infer_votes(ws, clu_d, topk_d, 5, shape[:2], want_labels_before=False)
  assert none_before is None and none_prob is None and torch.equal(q_bare, first[0]) and torch.equal(labels_bare, first[1])
  q_only = crf.infer_votes(ws, clu_d, topk_d, 5, shape[:2], want_labels=False, want_labels_before=False)
  assert q_only[1] is None and torch.equal(q_only[0], first[0])
  # the id map as [h, w] is the same call
  as_map = crf.infer_votes(ws, clu_d.view(33, 47), topk_d, 5, shape[:2], want_prob=True)
  assert all(torch.equal(a, b) for a, b in zip(first, as_map))


# ---------------------------------------------------------------------------
# ties, foreign labels, strided id maps
def test_a_tie_goes_to_the_lowest_class_before_and_after_the_init():
  image, clu, topk = ref.votes_case(16, 24, 5, SEED)
  topk = np.array(topk)
  tied = int(clu[0])
  topk[tied] = np.array([1, 3] * 10)
  crf = DenseCRF(**params('defaults', iter_max=0))
  ws = crf.prepare(on_device(image), 5)
  q, labels, before, prob = crf.infer_votes(ws, on_device(clu), on_device(topk), 5, (16, 24), want_prob=True)
  where = on_device(clu).view(16, 24) == tied
  assert where.any() and bool((before[where] == 1).all()) and bool((labels[where] == 1).all())
  assert bool((prob[1][where] == 0.5).all()) and bool((prob[3][where] == 0.5).all())
  assert torch.equal(q[1][where], q[3][where])


def test_a_label_outside_the_classes_adds_to_no_class():
  image, clu, topk = ref.votes_case(16, 24, 5, SEED)
  topk = np.array(topk)
  foreign, partly = int(clu[0]), int(clu[-1])
  assert foreign != partly
  topk[foreign] = np.array([5, 21, 255, -1, 64] * 4)           # an all-foreign row: v = 0 everywhere
  topk[partly, :5] = np.array([5, -7, 1 << 40, 64, 255])       # 15 of 20 votes are left
  votes = ref.vote_map(clu, topk, 5, (16, 24))
  for iter_max in (0, 3):
    crf = DenseCRF(**params('defaults', iter_max=iter_max))
    ws = crf.prepare(on_device(image), 5)
    q, labels, before, prob = crf.infer_votes(ws, on_device(clu), on_device(topk), 5, (16, 24), want_prob=True)
    assert np.array_equal(prob.cpu().numpy(), votes)
    q_two, labels_two = crf.infer(ws, prob)                     # crf_init on the same map
    assert torch.equal(q, q_two) and torch.equal(labels, labels_two)
    assert np.array_equal(before.cpu().numpy(), votes.argmax(0))
  where = on_device(clu).view(16, 24) == foreign                # (iter_max = 3 above, 0 here)
  crf = DenseCRF(**params('defaults', iter_max=0))
  q, labels, before, prob = crf.infer_votes(crf.prepare(on_device(image), 5), on_device(clu), on_device(topk), 5, (16, 24),
                                            want_prob=True)
  assert not prob[:, where].any() and not before[where].any() and not labels[where].any()
  assert bool((q[:, where] == q[0][where][0]).all()) and abs(float(q[0][where][0]) - 0.2) <= 1e-7   # Q_0 uniform
  assert abs(float(prob[:, on_device(clu).view(16, 24) == partly].sum(0)[0]) - 0.75) <= 1e-6


def test_an_id_outside_the_segments_is_clamped():
  image, clu, topk = ref.votes_case(7, 5, 2, SEED)
  m = topk.shape[0]
  wild = np.array(clu)
  wild[0], wild[1] = -3, m + 5
  clamped = np.clip(wild, 0, m - 1)
  crf = DenseCRF(**params('alternative'))
  ws = crf.prepare(on_device(image), 2)
  a = crf.infer_votes(ws, on_device(wild), on_device(topk), 2, (7, 5), want_prob=True)
  b = crf.infer_votes(ws, on_device(clamped), on_device(topk), 2, (7, 5), want_prob=True)
  assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_strided_id_map_is_copied_by_refine_votes_and_refused_below_it():
  """The crop of a padded id map: `DenseCRF.refine_votes` makes it contiguous, `infer_votes` and the _ffi wrapper take
  raw pointers and refuse it."""
  shape = (33, 47, 5)
  image, clu, topk, _, _ = ref.yardstick(shape, 'alternative')
  crf = DenseCRF(**params('alternative'))
  padded = torch.full((40, 64), 3, dtype=torch.int64, device=DEV)
  padded[:33, :47] = on_device(clu).view(33, 47)
  crop = padded[:33, :47]
  assert not crop.is_contiguous()
  q, labels, before = crf.refine_votes(on_device(image), crop, on_device(topk), 5)
  want = fused_case(shape, 'alternative')
  assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((q, labels, before), want))
  ws = crf.prepare(on_device(image), 5)
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_votes(ws, crop, on_device(topk), 5, shape[:2])
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.dense_crf_infer_votes(crop, on_device(topk), 5, shape[:2], 1, 3.0, 4.0, ws)


# ---------------------------------------------------------------------------
# argument errors: one case per status, none of them launches anything
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_argument_errors_return_their_status():
  h, w, c, m, k = 33, 47, 5, 24, 20
  crf = DenseCRF(**params('defaults'))
  ws = crf.prepare(torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV), c)
  clu = torch.zeros(h * w, dtype=torch.int64, device=DEV)
  topk = torch.zeros((4097, k), dtype=torch.int64, device=DEV)
  q = torch.empty((c, h, w), device=DEV)
  labels = torch.empty((h, w), dtype=torch.int64, device=DEV)
  need = _ffi.lib().spml_dense_crf_votes_workspace_bytes(m, c)
  assert need == m * 100 * 4 and q.numel() * 4 >= need + 16
  table = _ffi.workspace(need + 16, DEV)
  good = dict(clu=clu.data_ptr(), topk=topk.data_ptr(), m=m, k=k, ncls=c, q=q.data_ptr(), labels=labels.data_ptr(),
              before=0, prob=0, table=table.data_ptr(), table_bytes=need, ws=ws.data_ptr(), ws_bytes=ws.numel())

  def status(**changes):
    a = dict(good, **changes)
    p = ctypes.c_void_p
    return _ffi.lib().spml_dense_crf_infer_votes_f32(p(a['clu']), p(a['topk']), a['m'], a['k'], a['ncls'], h, w, 0, 3.0,
                                                     4.0, p(a['q']), p(a['labels']), p(a['before']), p(a['prob']),
                                                     p(a['table']), a['table_bytes'], p(a['ws']), a['ws_bytes'],
                                                     _ffi.stream_ptr())

  assert status() == 0
  assert [status(clu=0), status(topk=0), status(q=0)] == [INVALID] * 3                    # null pointers
  assert [status(m=0), status(k=0)] == [INVALID] * 2
  assert status(before=labels.data_ptr() + 4) == INVALID and status(prob=q.data_ptr() + 2) == INVALID
  assert status(m=4097, table_bytes=need * 200) == UNSUPPORTED
  assert status(ncls=65) == UNSUPPORTED
  assert status(table=0) == WORKSPACE and status(table_bytes=need - 1) == WORKSPACE       # missing, short
  assert status(table=table.data_ptr() + 4) == WORKSPACE                                 # misaligned
  assert status(ws_bytes=ws.numel() // 2) == WORKSPACE
  assert status(table=q.data_ptr()) == INVALID                                           # overlapping q
  assert status(table=clu.data_ptr()) == INVALID and status(table=ws.data_ptr()) == INVALID
  torch.cuda.synchronize()
  # ... and through the wrappers
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_votes(ws, clu, topk, c, (h, w))                                            # 4097 segments
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_votes(ws, clu, topk[:m], 65, (h, w))
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_votes(ws, clu[:-1], topk[:m], c, (h, w))
  with pytest.raises(_ffi.SpmlHipError):
    crf.infer_votes(ws, clu.cpu(), topk[:m], c, (h, w))


# ---------------------------------------------------------------------------
# more than 4096 segments: the framework route
def test_more_than_4096_segments_take_the_framework_route():
  h, w, c, k = 70, 60, 5, 20
  m = 4100
  rng = np.random.RandomState(7)
  image = dense_crf_ref.blocky(h, w, c, SEED)[0]
  clu = np.minimum(np.arange(h * w), m - 1).astype(np.int64)
  favoured = (np.arange(m) * 9 // m) % (c - 1)
  topk = np.where(rng.rand(m, k) < 0.7, favoured[:, None], rng.randint(0, c - 1, size=(m, k))).astype(np.int64)
  crf = DenseCRF(**params('alternative'))
  out = inference.knn_votes_crf_refine(on_device(image), on_device(clu), on_device(topk), c, crf)
  assert out['votes_path'] == inference.FRAMEWORK_SEGMENT_VOTES_PATH == 'framework_segment_votes'
  assert out['crf_path'].startswith('pairs_mfma_f16x2_c32')
  votes = ref.vote_map(clu, topk, c, (h, w))
  assert np.array_equal(inference.framework_segment_votes(on_device(clu), on_device(topk), c, (h, w)).cpu().numpy(), votes)
  assert np.array_equal(out['semantic_prediction_before_crf'].cpu().numpy(), votes.argmax(0))
  want = dense_crf_ref.dense_crf(image, votes, **params('alternative'))
  got = out['semantic_prob'].cpu().numpy()
  dev = float(np.abs(got.astype(np.float64) - want).max())
  print('4100 segments: max |Q - yardstick| = %.3e (bound %.2e)' % (dev, Q_BOUND))
  assert dev <= Q_BOUND and torch.equal(out['semantic_prediction'], out['semantic_prob'].argmax(0))
  # one segment fewer than the limit's successor takes the kernel, and both routes agree on a case both can take
  small = inference.knn_votes_crf_refine(on_device(image), on_device(np.minimum(clu, 4095)), on_device(topk[:4096]), c, crf)
  assert small['votes_path'] == inference.HIP_SEGMENT_VOTES_PATH == 'hip_segment_votes'
  two_step = crf.refine(on_device(image), on_device(ref.vote_map(np.minimum(clu, 4095), topk[:4096], c, (h, w))))
  assert torch.equal(small['semantic_prob'], two_step[0]) and torch.equal(small['semantic_prediction'], two_step[1])


# ---------------------------------------------------------------------------
# the driver on a stub embedder
def test_predict_knn_full_resolution_crf_on_a_padded_image():
  from spml_amd.models.predictions.segsort import segsort
  from spml_amd.train import voc12_scribble_config
  from test_inference_gpu import TinyEmbedder, blobs
  gen = torch.Generator().manual_seed(41)
  h, w, c, crop, stride = 30, 37, 5, (48, 48), (32, 32)
  model = TinyEmbedder(16, [3, 3]).to(DEV)
  predictor = segsort(voc12_scribble_config()).to(DEV).eval()
  bank = torch.nn.functional.normalize(torch.randn(90, 16, generator=gen), dim=1).to(DEV)
  bank_lab = torch.randint(0, c, (90,), generator=gen).to(DEV)
  image = blobs(gen, h, w)
  image_u8 = ((image[0] * 0.2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous().to(DEV)
  padded = inference.flip_scale_views(image.to(DEV), [1], False, crop)[0][0]
  assert tuple(padded.shape[-2:]) == crop
  crf = DenseCRF(**params('alternative'))
  before = _ffi.set_deterministic(True)                        # two runs of the k-means are compared bit for bit
  try:
    out = inference.predict_knn_full_resolution_crf(model, predictor, padded, (h, w), crop, stride, bank, bank_lab, c,
                                                    image_u8, crf)
    plain = inference.predict_full_resolution(model, predictor, padded, (h, w), crop, stride, bank, bank_lab)
  finally:
    _ffi.set_deterministic(before)
  clu, topk = out['cluster_index'], out['segment_topk']
  assert clu.numel() == h * w and clu.dtype == torch.int64 and tuple(topk.shape) == (int(clu.max()) + 1, 20)
  assert torch.equal(topk[clu], plain['semantic_score'])
  assert out['votes_path'] == 'hip_segment_votes' and out['crf_path'].startswith('pairs_mfma_f16x2_c32')
  again = inference.knn_votes_crf_refine(image_u8, clu, topk, c, crf)
  for key in ('semantic_prob', 'semantic_prediction', 'semantic_prediction_before_crf'):
    assert torch.equal(out[key], again[key]), key
  votes = ref.vote_map(clu.cpu().numpy(), topk.cpu().numpy(), c, (h, w))
  want = dense_crf_ref.dense_crf(image_u8.cpu().numpy(), votes, **params('alternative'))
  dev = float(np.abs(out['semantic_prob'].cpu().numpy().astype(np.float64) - want).max())
  print('end to end: max |Q - yardstick| = %.3e (bound %.2e)' % (dev, Q_BOUND))
  assert dev <= Q_BOUND
  assert np.array_equal(out['semantic_prediction_before_crf'].cpu().numpy(), votes.argmax(0))
  with pytest.raises(ValueError):
    inference.predict_knn_full_resolution_crf(model, predictor, padded, (h, w), crop, stride, bank, bank_lab, c,
                                              image_u8[:-1], crf)


# ---------------------------------------------------------------------------
# the three programs, end to end on two tiny synthetic images of a two-class config
COMMON = ('images', 'images_per_s', 'mIoU', 'pixel_acc', 'memory_prototypes', 'snapshot', 'semantic_memory_dir', 'save_dir')
FIELDS = {'inference': COMMON,
          'inference_crf': COMMON + ('mIoU_before_crf', 'changed_by_crf', 'crf_path', 'votes_path', 'crf_share'),
          'inference_crf_msc': COMMON + ('views', 'combine_path', 'crf_path', 'crf_share')}


@pytest.mark.parametrize('name', sorted(FIELDS))
def test_program_end_to_end(name, tmp_path, capsys, monkeypatch):
  cfg = tiny_config(tmp_path, 2, 'segsort')
  snap = write_snapshot(tmp_path, cfg, 'segsort')
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  save = tmp_path / 'results'
  extra = [] if name == 'inference' else ['--crf_iter_max', '2']
  capsys.readouterr()
  load_program(name).main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list',
                           'synthetic', '--kmeans_num_clusters', '4,4', '--label_divisor', '2048'] + extra)
  lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
  assert len(lines) == 1
  result = json.loads(lines[0])
  for key in FIELDS[name]:
    assert key in result, key
  assert result['images'] == 2 and result['images_per_s'] > 0 and 0.0 <= result['mIoU'] <= 100.0
  assert result['semantic_memory_dir'] == str(save / 'semantic_prototype')      # it built its own bank
  maps = [np.load(str(save / 'semantic_gray' / ('synthetic_%04d.npy' % i))) for i in range(2)]
  assert all(m.dtype == np.uint8 and m.shape == (65, 65) and m.max() < 2 for m in maps)
  if name != 'inference':
    assert result['crf_path'].startswith('pairs_mfma_f16x2_c32') and 0.0 < result['crf_share'] < 1.0
  if name == 'inference_crf':
    assert result['votes_path'] == 'hip_segment_votes' and 0.0 <= result['changed_by_crf'] <= 1.0
    assert 0.0 <= result['mIoU_before_crf'] <= 100.0
  if name == 'inference_crf_msc':
    assert result['views'] == 10 and result['combine_path'] == 'hip_view_votes'
