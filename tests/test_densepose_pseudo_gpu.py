"""The DensePose pseudo labels on the GPU (csrc/segment_cam.hip through spml_amd._ffi.segment_tag_cam and
spml_amd.inference) against the yardsticks of tests/densepose_pseudo_ref.py: the per-segment counts exactly,
the shares and the resampled map against the fp64 restatement and the golden of the reference's own lines, both routes,
the limits, one image on the tiny network and the program end to end.  Measured figures and how the bound follows from
them: profiles/densepose_pseudo.md."""
import functools

import numpy as np
import pytest
import torch

import densepose_pseudo_ref as ref
from spml_amd import _ffi, inference, inference_cli
from test_dense_crf_gpu import on_device, reference_stage, run_program, tiny_config, write_snapshot

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = dict(ids=ref.shape_id)

# max |probs - fp64| and max |acc - fp64|, values in [0, 1]: 4 x the largest deviation measured on one MI355X over the
# shape list and seeds 1-3 (MEASURED: profiles/densepose_pseudo.md; the factor covers FMA contraction, which differs
# between compilers, and the reference's double rounding of the row mean, which the golden carries and the kernel does
# not), never above 1e-5: about twenty fp32 roundings are 1.2e-6 at worst, a wrong tap weight or divisor errs by 1e-2.
MEASURED = 1.1912e-06              # (33, 47) -> (8, 11), seed 3: acc; probs stay below 2.8e-8
BOUND = min(4 * MEASURED, 1e-5)


def device_case(c):
  return {k: on_device(c[k]) for k in ('nn_index', 'nn_value', 'proto_label', 'cluster_index')}


def call(t, s, ncls, half_hw, out_hw, threshold=ref.THRESHOLD, want_tables=True):
  return _ffi.segment_tag_cam(t['nn_index'], t['nn_value'], t['proto_label'], threshold, t['cluster_index'], s, ncls,
                              half_hw, out_hw, want_tables=want_tables)


@functools.lru_cache(maxsize=None)
def hip_case(shape, seed=1):
  """(acc, counts, probs) of the entry on one case of the yardstick, as numpy arrays; computed once."""
  half_hw, out_hw, s, ncls = shape
  return tuple(o.cpu().numpy() for o in call(device_case(ref.case(shape, seed)), s, ncls, half_hw, out_hw))


# ---------------------------------------------------------------------------
# 1. counts and gather
@pytest.mark.parametrize('shape', ref.SHAPES, **IDS)
def test_counts_equal_bincount_exactly(shape):
  half_hw, out_hw, s, ncls = shape
  c = ref.case(shape)
  t = device_case(c)
  counts = hip_case(shape)[1]
  lab = t['proto_label'][t['nn_index']]
  ok = (t['nn_value'] >= ref.THRESHOLD) & (lab >= 0) & (lab < ncls)
  want = torch.bincount((t['cluster_index'] * ncls + lab)[ok], minlength=s * ncls).view(s, ncls)
  assert counts.dtype == np.int32 and counts.shape == (s, ncls)
  assert np.array_equal(counts, want.cpu().numpy()) and np.array_equal(counts, ref.yardstick(shape)[1])
  assert _ffi.segment_tag_cam_path_name(half_hw[0] * half_hw[1], s, ncls) == \
      ('global_table' if s * ncls > 8192 else 'lds_table')


@pytest.mark.parametrize('shape', ref.SHAPES, **IDS)
def test_two_calls_are_bit_identical_and_the_tables_leave_acc_alone(shape):
  half_hw, out_hw, s, ncls = shape
  t = device_case(ref.case(shape))
  first = call(t, s, ncls, half_hw, out_hw)
  again = call(t, s, ncls, half_hw, out_hw)
  assert all(torch.equal(a, b) for a, b in zip(first, again))
  bare = call(t, s, ncls, half_hw, out_hw, want_tables=False)
  assert torch.is_tensor(bare) and bare.dtype == torch.float32 and torch.equal(bare, first[0])
  assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(first, hip_case(shape)))
  before = _ffi.set_deterministic(True)
  try:
    assert all(torch.equal(a, b) for a, b in zip(first, call(t, s, ncls, half_hw, out_hw)))
  finally:
    _ffi.set_deterministic(before)


# 2. shares and map against the fp64 restatement
@pytest.mark.parametrize('shape', ref.SHAPES, **IDS)
def test_probs_and_acc_against_the_fp64_restatement(shape):
  (h2, w2), (oh, ow), s, ncls = shape
  _, counts, want_probs, want_acc = ref.yardstick(shape)
  acc, _, probs = hip_case(shape)
  dev_p = float(np.abs(probs.astype(np.float64) - want_probs).max())
  dev_a = float(np.abs(acc.astype(np.float64) - want_acc).max())
  print('%s: max |probs - fp64| = %.3e, max |acc - fp64| = %.3e (bound %.2e)' % (ref.shape_id(shape), dev_p, dev_a, BOUND))
  assert probs.dtype == np.float32 and probs.shape == (s, ncls) and acc.dtype == np.float32 and acc.shape == (ncls, oh, ow)
  assert not np.isnan(probs).any() and not np.isnan(acc).any()
  empty = counts.sum(1) == 0
  assert (s == 1 or empty.any()) and not probs[empty].any()              # rows without a counted pixel are zeros
  assert dev_p <= BOUND, (shape, dev_p)
  assert dev_a <= BOUND, (shape, dev_a)


@pytest.mark.parametrize('ci', [0, 1])
def test_golden_indices_give_the_golden_map(ci):
  g = ref.golden_cases()[ci]
  acc, counts, probs = (o.cpu().numpy() for o in call(device_case(g), g['num_segments'], g['ncls'], g['half_hw'],
                                                      g['out_hw']))
  assert np.array_equal(counts.sum(1), np.bincount(g['cluster_index'], minlength=g['num_segments']))
  dev_p = float(np.abs(probs.astype(np.float64) - g['s_probs']).max())
  dev_a = float(np.abs(acc.astype(np.float64) - g['semantic_probs']).max())
  print('golden %d: max |probs - s_probs| = %.3e, max |acc - semantic_probs| = %.3e (bound %.2e)' % (ci, dev_p, dev_a, BOUND))
  assert dev_p <= BOUND and dev_a <= BOUND


def golden_clustering(g):
  """What `generate_clusters` returned in the golden, on the device."""
  return {'cluster_embedding': on_device(g['cluster_embedding']),
          'cluster_semantic_label': on_device(g['cluster_semantic_label']),
          'cluster_index': on_device(g['raw_cluster_index'])}


@pytest.mark.parametrize('ci', [0, 1])
def test_densepose_segment_cam_gives_the_golden_cam(ci):
  g = ref.golden_cases()[ci]
  out = inference.densepose_segment_cam(golden_clustering(g), on_device(g['tags']), g['half_hw'], g['out_hw'], g['ncls'],
                                        int(g['cfg'][6]))
  assert out['cam_path'] == 'hip_segment_cam' and out['num_segments'] == g['num_segments']
  # the discrete part is the golden's: segment ids, prototype labels, every pixel's nearest labelled prototype
  assert np.array_equal(out['cluster_index'].cpu().numpy(), g['cluster_index'])
  assert np.array_equal(out['proto_label'].cpu().numpy(), g['proto_label'])
  assert np.array_equal(out['nn_index'].cpu().numpy(), g['nn_index'])
  assert float(np.abs(out['nn_value'].cpu().numpy() - g['nn_value']).max()) <= 1e-5
  cam = out['cam'].cpu().numpy()
  dev = float(np.abs(cam.astype(np.float64) - g['cam_full_arr']).max())
  print('golden %d: max |cam - cam_full_arr| = %.3e (bound %.2e)' % (ci, dev, BOUND))
  assert cam.shape == g['cam_full_arr'].shape and not np.isnan(cam).any() and dev <= BOUND
  assert not cam[~g['tags']].any() and np.array_equal(cam[g['tags']].reshape(3, -1).max(1), np.ones(3, np.float32))
  background = inference.densepose_segment_cam(golden_clustering(g), on_device(g['tags']), g['half_hw'], g['out_hw'],
                                               g['ncls'], int(g['cfg'][6]), background_threshold=0.25)['cam']
  assert torch.equal(background[1:], out['cam'][1:]) and bool((background[0] == 0.25).all())


# 3. routes
@pytest.mark.parametrize('ci', [0, 1])
def test_both_routes_agree_on_the_same_retrieval(ci, monkeypatch):
  g = ref.golden_cases()[ci]
  tags = on_device(g['tags'])
  arguments = (golden_clustering(g), tags, g['half_hw'], g['out_hw'], g['ncls'], int(g['cfg'][6]))
  hip = inference.densepose_segment_cam(*arguments)
  acc = inference.framework_densepose_segment_cam(hip['nn_index'], hip['nn_value'], hip['proto_label'], ref.THRESHOLD,
                                                  hip['cluster_index'], g['ncls'], g['half_hw'], g['out_hw'])
  want = _ffi.cam_finalize(acc.contiguous(), 1, tags, 'prob_mean', None)
  assert float((hip['cam'] - want).abs().max()) <= BOUND
  monkeypatch.setattr(_ffi, 'MAX_SEGMENT_TAG_CAM_SEGMENTS', 0)
  framework = inference.densepose_segment_cam(*arguments)
  assert framework['cam_path'] == 'framework_segment_cam' and hip['cam_path'] == 'hip_segment_cam'
  assert torch.equal(framework['cam'], want) and torch.equal(framework['nn_index'], hip['nn_index'])
  assert float(np.abs(framework['cam'].cpu().numpy().astype(np.float64) - g['cam_full_arr']).max()) <= BOUND


def test_no_labelled_prototype_raises():
  g = ref.golden_cases()[0]
  clustered = golden_clustering(g)
  clustered['cluster_semantic_label'] = torch.full_like(clustered['cluster_semantic_label'], 254)
  with pytest.raises(ValueError, match='no prototype'):
    inference.densepose_segment_cam(clustered, on_device(g['tags']), g['half_hw'], g['out_hw'], g['ncls'], 2048)


# 4. limits
def test_limits_raise():
  shape = ref.SHAPES[1]
  half_hw, out_hw, s, ncls = shape
  t = device_case(ref.case(shape))
  with pytest.raises(_ffi.SpmlHipError, match='outside the kernel'):
    call(t, s, 65, half_hw, out_hw)
  with pytest.raises(_ffi.SpmlHipError, match='outside the kernel'):
    call(t, 4097, ncls, half_hw, out_hw)
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    call(dict(t, nn_value=t['nn_value'].cpu()), s, ncls, half_hw, out_hw)
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    call(dict(t, cluster_index=t['cluster_index'].cpu()), s, ncls, half_hw, out_hw)
  with pytest.raises(_ffi.SpmlHipError, match='entries'):
    call(dict(t, nn_index=t['nn_index'][:-1]), s, ncls, half_hw, out_hw)
  with pytest.raises(_ffi.SpmlHipError, match='entries'):
    call(t, s, ncls, (8, 9), out_hw)
  with pytest.raises(_ffi.SpmlHipError, match='int64'):
    call(dict(t, cluster_index=t['cluster_index'].int()), s, ncls, half_hw, out_hw)
  with pytest.raises(_ffi.SpmlHipError):
    call(t, s, ncls, half_hw, (0, 2))
  with pytest.raises(_ffi.SpmlHipError):
    call(t, s, ncls, half_hw, out_hw, threshold=float('nan'))
  acc = call(t, s, ncls, half_hw, out_hw, want_tables=False)                  # and the call the others were built from
  assert tuple(acc.shape) == (ncls,) + out_hw


@pytest.mark.parametrize('shape', [ref.SHAPES[2], ref.SHAPES[5]], **IDS)
def test_an_index_just_past_the_end_counts_nowhere(shape):
  """`nn_index` = M or -1 and a segment id = S or -1: the pixel is counted nowhere, its taps contribute 0, and every other
  entry is what the call gives without them."""
  half_hw, out_hw, s, ncls = shape
  c = {k: np.array(v) for k, v in ref.case(shape).items()}
  m, n = len(c['proto_label']), c['nn_index'].size
  c['nn_index'][[3, n - 2]] = (m, -1)
  gone = np.array([0, 7, n - 1, n // 2])
  c['cluster_index'][gone] = (s, -1, s, -1)
  acc, counts, probs = (o.cpu().numpy() for o in call(device_case(c), s, ncls, half_hw, out_hw))
  valid = np.ones(n, bool)
  valid[[3, n - 2]] = False
  valid[gone] = False
  classes = ref.pixel_classes(np.where(valid, c['nn_index'], 0), c['nn_value'], c['proto_label'], ref.THRESHOLD, ncls)
  classes[~valid] = -1
  clu = np.where(valid, c['cluster_index'], 0)
  want_counts = ref.segment_counts(classes, clu, s, ncls)
  assert np.array_equal(counts, want_counts)
  # the map: a tap on an id outside [0, S) reads a row of zeros
  want_probs = ref.segment_probs(want_counts, clu)
  rows = np.vstack([want_probs, np.zeros((1, ncls))])
  ids = np.where((c['cluster_index'] >= 0) & (c['cluster_index'] < s), c['cluster_index'], s)
  want_acc = ref.resampled(rows, ids, half_hw, out_hw)
  assert np.abs(probs - want_probs).max() <= BOUND and np.abs(acc - want_acc).max() <= BOUND
  assert not np.isnan(acc).any()


# ---------------------------------------------------------------------------
# 5. one image on the tiny network
CRF_OPTIONS = ['--crf_iter_max', '2']


def test_pseudo_labels_densepose_crf_on_the_tiny_network(tmp_path, monkeypatch):
  cfg = tiny_config(tmp_path, 21, 'segsort')
  snap = write_snapshot(tmp_path, cfg, 'segsort')
  config, device, (emb, _, _), (ncls, crop, _, size), crf = reference_stage(cfg, snap, None)
  crf.crf.iter_max = 2
  # (a tiny synthetic image may keep no labelled point at all: the first that has one)
  index = next(i for i in range(8) if bool((inference_cli.synthetic_image(i, size, ncls, device)[1] < ncls).any()))
  image, label, instance = inference_cli.synthetic_image(index, size, ncls, device)
  padded = inference.flip_scale_views(image, [1], False, crop)[0][0]
  tags = inference.label_tags_from_map(label, ncls)
  image_u8 = crf.image_u8(padded, (size, size))
  walks, plain_walk = [], inference._walk

  def recording_walk(trans, cam, walk_steps):
    walks.append((cam, walk_steps))
    return plain_walk(trans, cam, walk_steps)

  monkeypatch.setattr(inference, '_walk', recording_walk)
  out = inference.pseudo_labels_densepose_crf(emb, padded, (size, size), label, instance, tags, image_u8, crf.crf)
  for key in ('cam', 'cam_rw', 'semantic_prob', 'semantic_prediction', 'semantic_prediction_before_crf', 'crf_path',
              'cam_path', 'cluster_index', 'num_segments'):
    assert key in out, key
  n8 = size // 8
  assert tuple(out['cam'].shape) == (ncls, n8, n8) == tuple(out['cam_rw'].shape)
  assert out['cam_path'] == 'hip_segment_cam' and out['crf_path'].startswith('pairs_mfma_')
  assert tuple(out['cluster_index'].shape) == ((size // 2) ** 2,)
  assert int(out['cluster_index'].max()) + 1 == out['num_segments']
  # the walk's input is the function's own cam, which carries the image's tags and nothing else
  assert len(walks) == 1 and walks[0][0] is out['cam'] and walks[0][1] == 6
  assert bool(tags.any()) and not out['cam'][~tags].any() and bool(out['cam'][tags].any())
  # the tail is the existing fused call on the function's own walked maps, bit for bit
  assert torch.equal(out['semantic_prediction_before_crf'], _ffi.upsample_argmax(out['cam_rw'], size, size))
  tail = inference.random_walk_crf_refine(image_u8, out['cam_rw'], crf.crf)
  assert torch.equal(out['semantic_prob'], tail['semantic_prob'])
  assert torch.equal(out['semantic_prediction_before_crf'], tail['semantic_prediction_before_crf'])
  ignored = label == 255
  assert bool(ignored.any()) and bool((out['semantic_prediction'][ignored] == 255).all())
  assert torch.equal(out['semantic_prediction'][~ignored], tail['semantic_prediction'][~ignored])
  assert int(out['semantic_prediction'][~ignored].max()) < ncls


# 6. the program, end to end on two tiny synthetic images
FIELDS = ('images_per_s', 'mIoU', 'pixel_acc', 'mIoU_before_crf', 'changed_by_crf', 'crf_path', 'crf_share', 'cam_path',
          'walk_steps', 'num_segments', 'images_without_labels', 'snapshot', 'save_dir')


def test_pseudo_denseposerw_crf_program(tmp_path, capsys, monkeypatch):
  cfg = tiny_config(tmp_path, 21, 'segsort')
  snap = write_snapshot(tmp_path, cfg, 'segsort')
  result, maps, _ = run_program('pseudo_denseposerw_crf', tmp_path, cfg, snap, CRF_OPTIONS, capsys, monkeypatch)
  for key in FIELDS:
    assert key in result, key
  assert result['crf_path'].startswith('pairs_mfma_') and result['cam_path'] == 'hip_segment_cam'
  assert result['walk_steps'] == 6 and 0.0 <= result['changed_by_crf'] <= 1.0
  # the maps written are the API's on the same snapshot
  config, device, (emb, _, _), (ncls, crop, _, size), crf = reference_stage(cfg, snap, None)
  crf.crf.iter_max = 2
  segments = []
  for index in range(2):
    image, label, instance = inference_cli.synthetic_image(index, size, ncls, device)
    padded = inference.flip_scale_views(image, [1], False, crop)[0][0]
    try:
      out = inference.pseudo_labels_densepose_crf(emb, padded, (size, size), label, instance,
                                                  inference.label_tags_from_map(label, ncls),
                                                  crf.image_u8(padded, (size, size)), crf.crf)
    except inference.NoLabelledPrototypeError:                # an image without a labelled point: ignored as a whole
      assert (maps[index] == 255).all()
      continue
    assert np.array_equal(maps[index], out['semantic_prediction'].to(torch.uint8).cpu().numpy())
    assert (maps[index] == 255).any() and (maps[index] < ncls).any()
    segments.append(out['num_segments'])
  assert segments and result['num_segments'] == round(sum(segments) / float(len(segments)), 1)
  assert result['images_without_labels'] == 2 - len(segments)
