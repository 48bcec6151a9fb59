"""The dense CRF on the GPU (csrc/dense_crf.hip through spml_amd.models.crf.DenseCRF) against the fp64 brute-force
oracle of tests/dense_crf_ref.py: marginals and labels over the shape list of that file, three image generators and two
parameter sets; the fused arg-max, bit-reproducibility, the prepare / infer split, the numpy route, the image
de-normalisation and the three `*_crf*` programs end to end.  Measured figures and how the bounds follow from them:
profiles/dense_crf.md."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import dense_crf_ref as ref
from spml_amd import _ffi, inference, inference_cli
from spml_amd.models.crf import DenseCRF
from test_dense_crf import denormalize_case, reference_denormalize
from test_inference_cli import load_program
from test_train_cli import YAML

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 1

# max |Q - oracle| per generator: at least 4 x the largest deviation the HIP path showed over every shape, both parameter
# sets and seeds 1-3 on one MI355X (1.38e-6 blocky, 8.65e-7 flat, 4.25e-5 noise: profiles/dense_crf.md; the factor is for
# the summation order, which differs with tile shape and box), and never above 5e-4, the limit of what counts as
# fp32-class here.  The same mathematics in fp32 numpy deviates up to 7.4e-7 / 5.9e-5 (blocky and flat / noise).
Q_BOUND = {'blocky': 6e-6, 'flat': 4e-6, 'noise': 2e-4}
assert max(Q_BOUND.values()) <= 5e-4
MARGIN = 1e-3                      # labels are compared where the oracle's top two marginals are further apart


def on_device(array):
  """A device copy of a numpy array (through a writable copy: the cached oracle cases are read-only)."""
  return torch.from_numpy(np.array(array)).to(DEV)


def label_cap(generator, shape):
  """Largest share of pixels that may fall under MARGIN where labels are compared, None where the case is Q-only."""
  if generator == 'blocky' and 1 < shape[2] <= 21:
    return 0.02
  if generator == 'blocky' and shape == (17, 129, 64):
    return 0.20
  if generator == 'flat' and shape == (33, 47, 5):
    return 0.02
  return None


@functools.lru_cache(maxsize=None)
def oracle_case(generator, shape, parameters, seed=SEED):
  """(image, probmap, fp64 Q) of one case, computed once and shared by the tests; read-only."""
  image, prob = ref.GENERATORS[generator](*shape, seed)
  want = ref.dense_crf(image, prob, **ref.PARAMETER_SETS[parameters])
  for a in (image, prob, want):
    a.setflags(write=False)
  return image, prob, want


@functools.lru_cache(maxsize=None)
def hip_case(generator, shape, parameters, seed=SEED):
  image, prob, _ = oracle_case(generator, shape, parameters, seed)
  crf = DenseCRF(**ref.PARAMETER_SETS[parameters])
  q, labels = crf.refine(on_device(image), on_device(prob))
  return q.cpu().numpy(), labels.cpu().numpy()


def check_against_oracle(got, labels, want, bound, cap, what):
  dev = float(np.abs(got.astype(np.float64) - want).max())
  print('%s: max |Q - oracle| = %.3e (bound %.1e)' % (what, dev, bound))
  assert got.dtype == np.float32 and got.shape == want.shape
  assert np.array_equal(labels, got.argmax(0)), what + ': the fused arg-max is not the arg-max of the returned Q'
  assert dev <= bound, (what, dev)
  assert np.abs(got.sum(0) - 1.0).max() <= 1e-5
  if cap is not None:
    top = np.sort(want, axis=0)
    keep = (top[-1] - top[-2]) > MARGIN
    left_out = 1.0 - keep.mean()
    print('%s: %.4f of the pixels under the margin (cap %.2f)' % (what, left_out, cap))
    assert left_out <= cap, (what, left_out)
    assert np.array_equal(labels[keep], want.argmax(0)[keep]), what


@pytest.mark.parametrize('parameters', ['defaults', 'alternative'])
@pytest.mark.parametrize('generator', ['blocky', 'flat', 'noise'])
@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_marginals_and_labels_against_the_fp64_oracle(shape, generator, parameters):
  _, _, want = oracle_case(generator, shape, parameters)
  got, labels = hip_case(generator, shape, parameters)
  check_against_oracle(got, labels, want, Q_BOUND[generator], label_cap(generator, shape),
                       '%s %s %s' % (generator, shape, parameters))
  if shape[2] == 1:
    assert np.array_equal(got, np.ones_like(got)) and not labels.any()      # one class: Q is exactly 1


@pytest.mark.parametrize('iter_max', [0, 1])
def test_no_and_one_iteration(iter_max):
  image, prob = ref.blocky(33, 47, 5, SEED)
  params = dict(ref.DEFAULTS, iter_max=iter_max)
  want = ref.dense_crf(image, prob, **params)
  q, labels = DenseCRF(**params).refine(on_device(image), on_device(prob))
  check_against_oracle(q.cpu().numpy(), labels.cpu().numpy(), want, Q_BOUND['blocky'], 0.02, 'iter_max %d' % iter_max)


def test_unnormalised_probmap_with_exact_zeros():
  """What the tag recipe feeds: every class divided by its own maximum, classes the image does not carry all zero."""
  image, prob = ref.blocky(32, 40, 21, SEED)
  prob = prob / prob.reshape(21, -1).max(1).reshape(21, 1, 1)
  prob[[3, 7, 20]] = 0.0
  prob[:, 5, 6] = 0.0                                         # and one pixel with no vote at all
  assert prob.max() == 1.0 and abs(prob.sum(0) - 1).max() > 0.5
  want = ref.dense_crf(image, prob, **ref.DEFAULTS)
  q, labels = DenseCRF(**ref.DEFAULTS).refine(on_device(image), on_device(prob))
  check_against_oracle(q.cpu().numpy(), labels.cpu().numpy(), want, Q_BOUND['blocky'], 0.02, 'un-normalised')


def test_wide_spatial_kernel():
  """pos_xy_std = 8: the separable filter keeps 48 taps on either side, more than this image is high."""
  image, prob = ref.blocky(33, 47, 5, SEED)
  params = dict(ref.ALTERNATIVE, pos_xy_std=8)
  assert DenseCRF(**params).path_name(33, 47, 5) == 'pairs_mfma_f16x2_c32+separable_r48'
  want = ref.dense_crf(image, prob, **params)
  q, labels = DenseCRF(**params).refine(on_device(image), on_device(prob))
  check_against_oracle(q.cpu().numpy(), labels.cpu().numpy(), want, Q_BOUND['blocky'], 0.02, 'pos_xy_std 8')


@pytest.mark.parametrize('shape', [(1, 2048, 2), (2048, 1, 2)], ids=['row', 'column'])
def test_longest_row_and_column(shape):
  """The side limit: centred coordinates reach -1024 and 1023, the squared distances 2047^2 -- still exact integers on the
  matrix cores (a rounded distance would show at once: K1 and K2 fall off over a few pixels)."""
  image, prob = ref.blocky(*shape, SEED)
  want = ref.dense_crf(image, prob, **ref.DEFAULTS)
  q, labels = DenseCRF(**ref.DEFAULTS).refine(on_device(image), on_device(prob))
  check_against_oracle(q.cpu().numpy(), labels.cpu().numpy(), want, Q_BOUND['blocky'], 0.02, 'side 2048 %s' % (shape,))


def test_two_calls_are_bit_identical():
  image, prob, _ = oracle_case('noise', (33, 47, 5), 'defaults')
  first = hip_case('noise', (33, 47, 5), 'defaults')
  crf = DenseCRF(**ref.DEFAULTS)
  q, labels = crf.refine(on_device(image), on_device(prob))
  assert np.array_equal(q.cpu().numpy(), first[0]) and np.array_equal(labels.cpu().numpy(), first[1])


def test_prepare_once_infer_twice_equals_two_full_calls():
  image, prob, _ = oracle_case('blocky', (17, 129, 64), 'defaults')
  image_d, prob_d = on_device(image), on_device(prob)
  crf = DenseCRF(**ref.DEFAULTS)
  ws = crf.prepare(image_d, 64)
  q_a, lab_a = crf.infer(ws, prob_d)
  q_b, lab_b = crf.infer(ws, prob_d, iter_max=4, pos_w=1.5, bi_w=7)
  q_c, lab_c = crf.infer(ws, prob_d, want_labels=False)
  full_a = hip_case('blocky', (17, 129, 64), 'defaults')
  full_b = DenseCRF(**dict(ref.DEFAULTS, iter_max=4, pos_w=1.5, bi_w=7)).refine(image_d, prob_d)
  assert np.array_equal(q_a.cpu().numpy(), full_a[0]) and np.array_equal(lab_a.cpu().numpy(), full_a[1])
  assert torch.equal(q_b, full_b[0]) and torch.equal(lab_b, full_b[1])
  assert lab_c is None and torch.equal(q_c, q_a)
  assert not torch.equal(q_a, q_b)


def test_numpy_route_equals_tensor_route():
  image, prob, _ = oracle_case('blocky', (33, 47, 5), 'alternative')
  crf = DenseCRF(**ref.ALTERNATIVE)
  got = crf(np.array(image), np.array(prob))
  assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == prob.shape
  assert np.array_equal(got, hip_case('blocky', (33, 47, 5), 'alternative')[0])
  as_tensor = crf(on_device(image), on_device(prob))
  assert as_tensor.is_cuda and np.array_equal(as_tensor.cpu().numpy(), got)
  out = inference.dense_crf_refine(on_device(image), on_device(prob), crf)
  assert set(out) == {'semantic_prob', 'semantic_prediction', 'crf_path'}
  assert out['crf_path'] == 'pairs_mfma_f16x2_c32+separable_r18'
  assert np.array_equal(out['semantic_prob'].cpu().numpy(), got)
  assert torch.equal(out['semantic_prediction'], out['semantic_prob'].argmax(0))


def test_unsupported_class_count_raises():
  image = torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV)
  with pytest.raises(_ffi.SpmlHipError):
    DenseCRF(**ref.DEFAULTS)(image, torch.full((65, 4, 4), 1.0 / 65, device=DEV))


def test_denormalized_uint8_on_the_device_is_the_reference_lines_on_every_pixel():
  x, means, stds = denormalize_case(37, 53, 12)
  want = reference_denormalize(x.copy(), means, stds)
  got = inference.denormalized_uint8(on_device(x), means, stds)
  assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------
# the three programs, end to end on two tiny synthetic images
def tiny_config(tmp_path, num_classes, prediction_types):
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101').replace('num_classes: 21', 'num_classes: %d' % num_classes)
          .replace('image_size: 97', 'image_size: 65').replace('- 97', '- 65')
          .replace('prediction_types: segsort', 'prediction_types: ' + prediction_types))
  yaml = yaml.replace('stride:\n    - 65\n    - 65', 'stride:\n    - 43\n    - 43')
  assert yaml.count('- 65') == 4 and yaml.count('- 43') == 2
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(yaml)
  return cfg


def write_snapshot(tmp_path, cfg, head):
  from spml_amd.config.default import config, update_config
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  update_config(str(cfg))
  torch.manual_seed(9)
  snap = tmp_path / 'snapshot'
  os.makedirs(str(snap))
  if head == 'segsort':
    from spml_amd.models.predictions.segsort import segsort
    prediction = segsort(config).state_dict()
  else:
    from spml_amd.models.predictions.softmax_classifier import softmax_classifier
    prediction = softmax_classifier(config).state_dict()
  torch.save({'embedding_model': resnet_101_deeplab(config).state_dict(), 'prediction_model': prediction},
             str(snap / 'model-{:d}.pth'.format(config.train.max_iteration - 1)))
  return snap


def run_program(name, tmp_path, cfg, snap, extra, capsys, monkeypatch):
  monkeypatch.setattr(inference_cli, 'NUM_SYNTHETIC_IMAGES', 2)
  save = tmp_path / 'results'
  capsys.readouterr()
  load_program(name).main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list',
                           'synthetic'] + extra)
  lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
  assert len(lines) == 1
  result = json.loads(lines[0])
  assert result['images'] == 2 and result['images_per_s'] > 0
  assert result['crf_path'] == 'pairs_mfma_f16x2_c32+separable_r6' and 0.0 < result['crf_share'] < 1.0
  maps = [np.load(str(save / 'semantic_gray' / ('synthetic_%04d.npy' % i))) for i in range(2)]
  assert all(m.dtype == np.uint8 and m.shape == (65, 65) for m in maps)
  return result, maps, save


def reference_stage(cfg, snap, head):
  """What a program loads, loaded again: (config, device, models, geometry, the CRF stage with the default options)."""
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  args = parse_args('test', ['--snapshot_dir', str(snap), '--cfg_path', str(cfg)])
  device = torch.device(DEV)
  models = inference_cli.load_models(config, args, device, head)
  return config, device, models, inference_cli.geometry(config), inference_cli.CrfStage(config, args)


def check_refined_maps(maps, pairs):
  """pairs: per image (refined labels by dense_crf_refine on the sibling's semantic_prob, the sibling's own labels)."""
  changed = 0
  for saved, (refined, plain) in zip(maps, pairs):
    assert np.array_equal(saved, refined.to(torch.uint8).cpu().numpy())
    changed += int((refined != plain).sum())
  assert changed > 0, 'the refinement changed no label'


def test_inference_softmax_crf_program(tmp_path, capsys, monkeypatch):
  cfg = tiny_config(tmp_path, 21, 'softmax_classifier')
  snap = write_snapshot(tmp_path, cfg, 'softmax_classifier')
  result, maps, _ = run_program('inference_softmax_crf', tmp_path, cfg, snap, [], capsys, monkeypatch)
  for key in ('mIoU', 'pixel_acc', 'head_path', 'snapshot', 'save_dir'):
    assert key in result, key
  config, device, (emb, pred, _), (ncls, crop, stride, size), crf = reference_stage(cfg, snap, 'softmax_classifier')
  pairs = []
  for index in range(2):
    image, _, _ = inference_cli.synthetic_image(index, size, ncls, device)
    padded = inference.flip_scale_views(image, [1], False, crop)[0][0]
    out = inference.predict_softmax_full_resolution(emb, pred, padded, (size, size), crop, stride)
    prob = torch.softmax(out['semantic_logit'], dim=1)[0, :, :size, :size].contiguous()
    refined = inference.dense_crf_refine(crf.image_u8(padded, (size, size)), prob, crf.crf)
    pairs.append((refined['semantic_prediction'], out['semantic_prediction']))
  check_refined_maps(maps, pairs)


def test_inference_softmax_crf_msc_program(tmp_path, capsys, monkeypatch):
  cfg = tiny_config(tmp_path, 21, 'softmax_classifier')
  snap = write_snapshot(tmp_path, cfg, 'softmax_classifier')
  result, maps, _ = run_program('inference_softmax_crf_msc', tmp_path, cfg, snap, [], capsys, monkeypatch)
  for key in ('mIoU', 'pixel_acc', 'head_path', 'combine_path', 'snapshot', 'save_dir'):
    assert key in result, key
  assert result['views'] == 10
  config, device, (emb, pred, _), (ncls, crop, stride, size), crf = reference_stage(cfg, snap, 'softmax_classifier')
  pairs = []
  for index in range(2):
    image, _, _ = inference_cli.synthetic_image(index, size, ncls, device)
    views = inference.flip_scale_views(image, [0.5, 0.75, 1, 1.25, 1.5], True, crop)
    out = inference.predict_softmax_multiscale(emb, pred, views, (size, size), crop, stride)
    prob = out['semantic_prob'] / torch.full((), 10.0, device=device)
    refined = inference.dense_crf_refine(crf.image_u8(image, (size, size)), prob, crf.crf)
    pairs.append((refined['semantic_prediction'], out['semantic_prediction']))
  check_refined_maps(maps, pairs)


def striped_image(index, size, num_classes, device):
  """Stand-in for `inference_cli.synthetic_image` at 65 x 65: the seeded generator puts one class into a 171-pixel cell,
  so a tiny image carries one tag and the tag-normalised arg-max is constant before and after any refinement.  Three
  vertical stripes of three classes, each with its own colour (+- 0.05 noise in the network's normalised units)."""
  g = torch.Generator().manual_seed(77 + index)
  classes = torch.tensor([1 + index, 7, 15]) % num_classes
  column = torch.arange(size) * 3 // size
  label = classes[column].view(1, size).expand(size, size).contiguous()
  colour = torch.tensor([[-1.0, 0.2, 1.0], [0.8, -0.9, 0.1], [0.0, 1.1, -1.2]])[column]            # [size, 3]
  image = colour.t().reshape(1, 3, 1, size).expand(1, 3, size, size) + 0.05 * torch.randn(1, 3, size, size, generator=g)
  return image.contiguous().to(device), label.to(device), label.clone().to(device)


def test_pseudo_inference_crf_msc_program(tmp_path, capsys, monkeypatch):
  monkeypatch.setattr(inference_cli, 'synthetic_image', striped_image)
  cfg = tiny_config(tmp_path, 21, 'segsort')
  snap = write_snapshot(tmp_path, cfg, 'segsort')
  before = _ffi.set_deterministic(True)                       # the bank and the votes of two runs are compared bit for bit
  try:
    extra = ['--kmeans_num_clusters', '4,4', '--label_divisor', '2048']
    result, maps, save = run_program('pseudo_inference_crf_msc', tmp_path, cfg, snap, extra, capsys, monkeypatch)
    for key in ('mIoU', 'pixel_acc', 'instance_mIoU', 'combine_path', 'normalize_path', 'memory_prototypes', 'snapshot',
                'semantic_memory_dir', 'save_dir'):
      assert key in result, key
    assert result['views'] == 8
    config, device, (emb, pred, _), (ncls, crop, stride, size), crf = reference_stage(cfg, snap, 'segsort')
    config.network.kmeans_num_clusters = [4, 4]
    config.network.label_divisor = 2048
    protos, proto_labels = inference_cli.load_bank(str(save / 'semantic_prototype'), config, device)
    pairs = []
    for index in range(2):
      image, label, _ = inference_cli.synthetic_image(index, size, ncls, device)
      views = inference.flip_scale_views(image, [0.5, 1, 1.5, 2], True, crop)
      tags = inference.label_tags_from_map(label, ncls)
      out = inference.pseudo_labels_knn_multiscale(emb, pred, views, (size, size), crop, stride, protos, proto_labels,
                                                   ncls, tags, floor=0.15, return_prob=True)
      refined = inference.dense_crf_refine(crf.image_u8(image, (size, size)), out['semantic_prob'], crf.crf)
      pairs.append((refined['semantic_prediction'], out['semantic_prediction']))
    check_refined_maps(maps, pairs)
  finally:
    _ffi.set_deterministic(before)
