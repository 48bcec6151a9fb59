"""Training summaries on the GPU (csrc/train_summary.hip, spml_amd/summary.py) against the fp64 yardstick
(tests/train_summary_ref.py): the moments, the projection with its extrema, the one-launch picture, the whole chain with
the library's own eigenvectors, the refusals of the entries, and a Trainer that writes summaries without its training
changing by a bit.

SHAPES
  the fixture's two cases (tests/golden/n16_train_summary.npz): [2, 64, 9, 11] with 33 x 41 labels, [1, 32, 8, 8] with
  8 x 8 labels;
  [2, 64, 13, 17], channels-last and NCHW-contiguous: 442 pixels, no multiple of two pixels' step, of a tile of 64 or of
  a workgroup's four tiles; two workgroups in the moment passes;
  [3, 32, 5, 7] with an all-zero pixel and an image whose embedding is constant (every projected channel constant);
  [1, 64, 1, 3].

BOUNDS, measured on an MI355X against the fp64 yardstick (two runs, the same figures), times four
(profiles/train_summary.md):
  moments     largest |cov - cov64| / max |cov64| 1.48e-7 ([3, 32, 5, 7]); mean 1.03e-7 of max |mean|  -> 6e-7, ceiling 1e-5
  projection  largest |proj - proj64| 1.16e-7 ([1, 64, 1, 3])                                       -> 4.7e-7, ceiling 1e-5
  end to end  largest deviation of the stretched value (v - min) / (max - min) with the library's own eigenvectors
              1.17e-7 (the fixture's first case)                                                    -> 4.7e-7, ceiling 1e-3
Embedding bytes must equal the yardstick's wherever its t = 255 (v - min) / (max - min) is farther than delta from an
integer and may differ by one elsewhere; delta = 255 x the bound.  At most 1 % of a case's values may lie inside delta,
asserted on the yardstick alone; the values that are 0 or 255 by construction (the extrema of an image's channel, two
per channel, and every value of a constant channel) are exact on both sides and are not counted."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import train_summary_ref as R
from spml_amd import _ffi, ops
from spml_amd.utils.general import vis

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOMENTS_BOUND, MOMENTS_CEILING = 6e-7, 1e-5
PROJ_BOUND, PROJ_CEILING = 4.7e-7, 1e-5
E2E_BOUND, E2E_CEILING = 4.7e-7, 1e-3


def _coherent(seed, n, c, h, w, strengths=(3.0, 2.2, 1.6, 1.2, 0.8), noise=0.15):
  """A few directions of graded strength blended by smooth spatial weights, plus noise: separated eigenvalues."""
  rng = np.random.default_rng(seed)
  dirs = rng.standard_normal((len(strengths), c)) * np.array(strengths)[:, None]
  cy, cx = rng.random((n, len(strengths))), rng.random((n, len(strengths)))
  yy, xx = np.linspace(0, 1, h).reshape(1, 1, h, 1), np.linspace(0, 1, w).reshape(1, 1, 1, w)
  weight = np.exp(-((yy - cy[:, :, None, None]) ** 2 + (xx - cx[:, :, None, None]) ** 2) / 0.05)
  emb = np.einsum('nbhw,bc->nchw', weight, dirs) + noise * rng.standard_normal((n, c, h, w))
  return emb.astype(np.float32)


def _labels(seed, n, h, w):
  rng = np.random.default_rng(seed)
  sem = rng.integers(0, 21, size=(n, h, w)).astype(np.int64)
  sem[rng.random((n, h, w)) < 0.1] = 255
  sem[0, 0, 0] = 256 + 7                                   # outside the table: masked to 7
  return sem, rng.integers(0, 40, size=(n, h, w)).astype(np.int64)


@pytest.fixture(scope='module')
def gold():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'n16_train_summary.npz'))


@pytest.fixture(scope='module')
def cases(gold):
  """name -> dict(emb fp32 numpy [N, C, H, W], layout, labels, separated); the yardstick's chain is added once."""
  odd = _coherent(62, 2, 64, 13, 17)
  special = _coherent(18, 3, 32, 5, 7)
  special[0, :, 2, 3] = 0.0                                # an all-zero pixel
  special[1] = special[1, :, 0, 0][:, None, None]          # the embedding constant over image 1
  out = {
      'fixture0': dict(emb=gold['c0_embedding'], layout='nhwc', separated=True,
                       labels=(gold['c0_semantic'].astype(np.int64), gold['c0_instance'].astype(np.int64))),
      'fixture1': dict(emb=gold['c1_embedding'], layout='nchw', separated=True,
                       labels=(gold['c1_semantic'].astype(np.int64), gold['c1_instance'].astype(np.int64))),
      'odd_nhwc': dict(emb=odd, layout='nhwc', separated=True, labels=_labels(1, 2, 13, 17)),
      'odd_nchw': dict(emb=odd, layout='nchw', separated=True, labels=_labels(1, 2, 13, 17)),
      'special': dict(emb=special, layout='nhwc', separated=False, labels=_labels(2, 3, 11, 15)),
      'tiny': dict(emb=_coherent(19, 1, 64, 1, 3), layout='nhwc', separated=False, labels=_labels(3, 1, 1, 3)),
  }
  table = vis.voc_color_map()
  for case in out.values():
    case['ref'] = R.chain(case['emb'], case['labels'][0], case['labels'][1], table)
    # the projection and the panels are judged with the yardstick's basis and projection rounded to fp32
    basis32 = np.ascontiguousarray(case['ref']['basis'].astype(np.float32))
    proj = R.project(case['emb'], basis32)
    case['basis32'], case['proj64'] = basis32, proj
    proj32 = proj.astype(np.float32)
    minmax32 = R.extrema(proj32)
    t, bytes_ = R.stretch(proj32, minmax32)
    case.update(proj32=proj32, minmax32=minmax32.astype(np.float32), t32=t,
                picture32=R.picture(case['labels'][0], case['labels'][1], bytes_, table))
  return out


def _device(case):
  emb = torch.from_numpy(case['emb']).to(DEV)
  if case['layout'] == 'nhwc':
    emb = emb.contiguous(memory_format=torch.channels_last)
  return emb


def _check_bytes(got, t, delta, what):
  """got uint8, t the yardstick's float, same shape: equal outside delta of an integer, within one inside; at most 1 %
  inside, the exact 0 / 255 of the extrema and of constant channels not counted."""
  want = np.floor(t).astype(np.int64)
  near = R.near_integer(t, delta)
  by_construction = (t == 0.0) | (t == 255.0)
  share = (near & ~by_construction).mean()
  assert share <= 0.01, '%s: %.2f %% of the yardstick lies within %.1e of an integer' % (what, 100 * share, delta)
  diff = np.abs(got.astype(np.int64) - want)
  assert (diff[~near] == 0).all(), '%s: %d bytes differ outside delta' % (what, int((diff[~near] != 0).sum()))
  assert (diff[near] <= 1).all(), what


NAMES = ('fixture0', 'fixture1', 'odd_nhwc', 'odd_nchw', 'special', 'tiny')
PATHS = {'fixture0': 'gram_mfma_f32_c64', 'fixture1': 'gram_mfma_f32_c32_nchw', 'odd_nhwc': 'gram_mfma_f32_c64',
         'odd_nchw': 'gram_mfma_f32_c64_nchw', 'special': 'gram_mfma_f32_c32', 'tiny': 'gram_mfma_f32_c64'}


@pytest.mark.parametrize('name', NAMES)
def test_moments(cases, name):
  case = cases[name]
  emb = _device(case)
  assert ops.pca_path_name(emb.shape[1], *_ffi.embedding_strides(emb)) == PATHS[name]
  mean, cov = ops.pca_moments(emb)
  again = ops.pca_moments(emb)
  assert torch.equal(mean, again[0]) and torch.equal(cov, again[1])      # bit-identical from call to call
  assert torch.equal(cov, cov.t())
  ref = case['ref']
  dev_cov = np.abs(cov.cpu().numpy() - ref['cov']).max() / np.abs(ref['cov']).max()
  dev_mean = np.abs(mean.cpu().numpy() - ref['mean']).max() / np.abs(ref['mean']).max()
  print('%s: cov deviates by %.3e of its largest entry, mean by %.3e' % (name, dev_cov, dev_mean))
  assert MOMENTS_BOUND <= MOMENTS_CEILING
  assert dev_cov <= MOMENTS_BOUND and dev_mean <= MOMENTS_BOUND, (dev_cov, dev_mean)


def test_moments_of_the_two_storages_agree(cases):
  a, b = ops.pca_moments(_device(cases['odd_nhwc'])), ops.pca_moments(_device(cases['odd_nchw']))
  scale = np.abs(cases['odd_nhwc']['ref']['cov']).max()
  assert (a[1] - b[1]).abs().max().item() / scale <= MOMENTS_BOUND
  assert (a[0] - b[0]).abs().max().item() <= MOMENTS_BOUND


def test_moments_in_the_deterministic_mode(cases):
  emb = _device(cases['odd_nhwc'])
  plain = ops.pca_moments(emb)
  before = _ffi.set_deterministic(True)
  try:
    det = ops.pca_moments(emb)
  finally:
    _ffi.set_deterministic(before)
  assert torch.equal(plain[0], det[0]) and torch.equal(plain[1], det[1])


@pytest.mark.parametrize('name', NAMES)
def test_projection_and_extrema(cases, name):
  case = cases[name]
  emb = _device(case)
  proj, minmax = ops.pca_project_minmax(emb, torch.from_numpy(case['basis32']).to(DEV))
  n = emb.shape[0]
  assert proj.shape == (n, emb.shape[2], emb.shape[3], 3) and minmax.shape == (n, 3, 2)
  dev = np.abs(proj.cpu().numpy().astype(np.float64) - case['proj64']).max()
  print('%s: proj deviates by %.3e' % (name, dev))
  assert PROJ_BOUND <= PROJ_CEILING
  assert dev <= PROJ_BOUND, dev
  flat = proj.view(n, -1, 3)
  assert torch.equal(minmax[:, :, 0], flat.min(1)[0]) and torch.equal(minmax[:, :, 1], flat.max(1)[0])
  again = ops.pca_project_minmax(emb, torch.from_numpy(case['basis32']).to(DEV))
  assert torch.equal(proj, again[0]) and torch.equal(minmax, again[1])


@pytest.mark.parametrize('name', ('fixture0', 'fixture1', 'special', 'tiny'))
def test_panels(cases, name):
  case = cases[name]
  sem, ins = (torch.from_numpy(x).to(DEV) for x in case['labels'])
  proj, minmax = torch.from_numpy(case['proj32']).to(DEV), torch.from_numpy(case['minmax32']).to(DEV)
  table = torch.from_numpy(vis.voc_color_map()).to(DEV)
  n, h, w = proj.shape[:3]
  out = torch.full((3,) + vis.summary_grid_shape(n, h, w), 77, dtype=torch.uint8, device=DEV)      # every byte is written
  got = ops.summary_panels(sem, ins, proj, minmax, table, out=out).cpu().numpy()
  want = case['picture32']
  assert got.shape == want.shape == (3,) + vis.summary_grid_shape(n, h, w)
  if n == 1:
    assert got.shape == (3, h, 3 * w)                      # no border around a single image
  # everything but the embedding panels: every byte
  emb_mask = np.zeros(want.shape, dtype=bool)
  t_full = np.zeros(want.shape, dtype=np.float64)
  for i in range(n):
    row, col = vis.summary_grid_origin(n, i, h)
    emb_mask[:, row:row + h, col + 2 * w:col + 3 * w] = True
    t_full[:, row:row + h, col + 2 * w:col + 3 * w] = case['t32'][i].transpose(2, 0, 1)
  assert np.array_equal(got[~emb_mask], want[~emb_mask])
  _check_bytes(got[emb_mask], t_full[emb_mask], 255 * PROJ_BOUND, name)
  if name == 'special':                                    # the constant image: every channel 0
    row, col = vis.summary_grid_origin(n, 1, h)
    assert (case['minmax32'][1, :, 0] == case['minmax32'][1, :, 1]).all()
    assert (got[:, row:row + h, col + 2 * w:col + 3 * w] == 0).all()
  # the embedding panel alone
  alone = ops.summary_panels(None, None, proj, minmax, None).cpu().numpy()
  assert alone.shape == (n, 3, h, w)
  for i in range(n):
    row, col = vis.summary_grid_origin(n, i, h)
    assert np.array_equal(alone[i], got[:, row:row + h, col + 2 * w:col + 3 * w])


@pytest.mark.parametrize('name', ('fixture0', 'fixture1', 'odd_nhwc', 'odd_nchw'))
def test_embedding_to_rgb_end_to_end(cases, name):
  case = cases[name]
  ref = case['ref']
  lam = R.eigenvalues(ref['cov'])[:4]
  assert (lam[:-1] >= 1.5 * lam[1:]).all(), lam            # (else the components themselves are arbitrary)
  emb = _device(case)
  basis, mean, values = vis.principal_components(emb, 3)
  assert basis.shape == (emb.shape[1], 3) and basis.dtype == torch.float32 and basis.is_cuda
  assert np.allclose(values.numpy(), ref['values'], rtol=1e-5) and np.allclose(mean.cpu().numpy(), ref['mean'], atol=1e-6)
  proj, minmax = ops.pca_project_minmax(emb, basis)
  low, high = minmax[:, None, None, :, 0].double(), minmax[:, None, None, :, 1].double()
  stretched = ((proj.double() - low) / (high - low)).cpu().numpy()
  dev = np.abs(stretched - ref['t'] / 255.0).max()
  print('%s: end to end the stretched value deviates by %.3e' % (name, dev))
  assert E2E_BOUND <= E2E_CEILING
  assert dev <= E2E_BOUND, dev
  rgb = vis.embedding_to_rgb(emb)
  assert rgb.shape == (emb.shape[0], 3, emb.shape[2], emb.shape[3]) and rgb.dtype == torch.uint8 and rgb.is_cuda
  _check_bytes(rgb.cpu().numpy().transpose(0, 2, 3, 1), ref['t'], 255 * E2E_BOUND, name)


def test_embedding_to_rgb_outside_the_hip_route(cases):
  """C = 48: the same mathematics as framework ops on the device."""
  emb = _coherent(20, 2, 48, 9, 11)
  ref = R.chain(emb)
  lam = R.eigenvalues(ref['cov'])[:4]
  assert (lam[:-1] >= 1.5 * lam[1:]).all(), lam
  rgb = vis.embedding_to_rgb(torch.from_numpy(emb).to(DEV))
  assert ops.pca_path_name(48, 1, 99) == 'unsupported'
  _check_bytes(rgb.cpu().numpy().transpose(0, 2, 3, 1), ref['t'], 255 * E2E_BOUND, 'c48')


def test_training_summary_write(cases, tmp_path):
  from PIL import Image
  from spml_amd.summary import TrainingSummary
  case = cases['fixture0']
  emb = _device(case)
  sem, ins = (torch.from_numpy(x).to(DEV) for x in case['labels'])
  directory = tmp_path / 'summary'
  summary = TrainingSummary(str(directory), vis.voc_color_map(), 2)
  picture = summary.write(5, sem, ins, emb, {'sem_ann_loss': torch.tensor(2.0, device=DEV), 'loss': 2.0, 'lr': 1e-3})
  summary.close()
  got = picture.cpu().numpy()
  n, h, w = 2, 9, 11
  want = case['ref']['picture']
  assert got.shape == want.shape == (3,) + vis.summary_grid_shape(n, h, w)
  emb_mask = np.zeros(want.shape, dtype=bool)
  t_full = np.zeros(want.shape, dtype=np.float64)
  for i in range(n):
    row, col = vis.summary_grid_origin(n, i, h)
    emb_mask[:, row:row + h, col + 2 * w:col + 3 * w] = True
    t_full[:, row:row + h, col + 2 * w:col + 3 * w] = case['ref']['t'][i].transpose(2, 0, 1)
  assert np.array_equal(got[~emb_mask], want[~emb_mask])
  _check_bytes(got[emb_mask], t_full[emb_mask], 255 * E2E_BOUND, 'write')
  image = Image.open(str(directory / 'image-0000005.png'))
  assert image.mode == 'RGB' and np.array_equal(np.asarray(image).transpose(2, 0, 1), got)
  line, = [json.loads(text) for text in open(str(directory / 'scalars.jsonl'))]
  assert line['iter'] == 5 and line['sem_ann_loss'] == 2.0 and line['images_per_s'] is None


def test_refusals_launch_nothing(cases):
  lib = _ffi.lib()
  emb = _device(cases['fixture0'])                          # [2, 64, 9, 11] channels-last
  need = lib.spml_train_summary_workspace_bytes(2, 64, 9, 11)
  assert need > 0
  ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
  mean = torch.full((64,), -7.0, dtype=torch.float64, device=DEV)
  cov = torch.full((64, 64), -7.0, dtype=torch.float64, device=DEV)
  basis = torch.zeros(64, 3, device=DEV)
  proj = torch.full((2, 9, 11, 3), -7.0, device=DEV)
  minmax = torch.full((2, 3, 2), -7.0, device=DEV)
  s = _ffi.stream_ptr()
  off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
  p = lambda t: off(t, 0)                                   # (the embedding is channels-last: a raw pointer)

  def moments(n=2, c=64, h=9, w=11, ps=64, cs=1, wsp=None, nbytes=need):
    return lib.spml_pca_moments_f32(p(emb), n, c, h, w, ps, cs, p(mean), p(cov), wsp or p(ws), nbytes, s)

  def project(n=2, c=64, h=9, w=11, ps=64, cs=1, wsp=None, nbytes=need):
    return lib.spml_pca_project_minmax_f32(p(emb), n, c, h, w, ps, cs, p(basis), p(proj), p(minmax), wsp or p(ws), nbytes, s)

  for call in (moments, project):
    assert call(c=48, ps=48) == -2                         # SPML_ERR_UNSUPPORTED
    assert call(ps=64, cs=2) == -2
    assert call(n=2, h=32768, w=32768) == -2               # P = 2^31, by the arguments alone
    assert call(n=1 << 20, h=1 << 10, w=1 << 11) == -2
    assert call(nbytes=need - 1) == -3                     # SPML_ERR_WORKSPACE
    assert call(wsp=off(ws, 4), nbytes=need + 32) == -1    # SPML_ERR_INVALID_ARG: a misaligned workspace
    assert call(n=0) == -2
  assert lib.spml_pca_moments_f32(off(emb, 4), 2, 64, 9, 11, 64, 1, p(mean), p(cov), p(ws), need, s) == -1
  table = torch.from_numpy(vis.voc_color_map()).to(DEV)
  sem = torch.zeros(2, 33, 41, dtype=torch.int64, device=DEV)
  out = torch.full((3, 24, 37), 77, dtype=torch.uint8, device=DEV)

  def panels(pad=2, out_h=24, out_w=37, n=2):
    return lib.spml_summary_panels_u8(p(sem), p(sem), n, 33, 41, p(proj), p(minmax), 9, 11, p(table), pad, out_h, out_w,
                                      p(out), s)
  assert panels(out_w=35) == -2 and panels(out_h=22) == -2 and panels(pad=0) == -2 and panels(pad=1) == -2
  assert lib.spml_summary_panels_u8(p(sem), None, 2, 33, 41, p(proj), p(minmax), 9, 11, p(table), 2, 24, 37, p(out), s) == -1
  torch.cuda.synchronize()
  assert (mean == -7).all() and (cov == -7).all() and (proj == -7).all() and (minmax == -7).all() and (out == 77).all()
  assert (ws == 0).all()
  assert moments() == 0 and project() == 0 and panels() == 0
  torch.cuda.synchronize()
  assert not (out == 77).all()
  with pytest.raises(_ffi.SpmlHipError):
    ops.pca_moments(torch.zeros(1, 32, 2, 2))              # a CPU tensor: no CPU path


def _train(tensorboard_step, directory, steps=2, batch=4, crop=257):
  """Two steps of the configuration whose steps tests/test_determinism_gpu.py shows to be bit-reproducible (ResNet-50
  DeepLab, batch 4, 257 x 257, channels-last, tools/probe_determinism.py's seeds) -> every parameter afterwards."""
  from spml_amd import synth
  from spml_amd.summary import TrainingSummary
  from spml_amd.train import Trainer, voc12_scribble_config
  torch.manual_seed(235)
  cfg = voc12_scribble_config(batch_size=batch, crop=crop, use_syncbn=False)
  cfg.network.backbone_types = 'panoptic_deeplab_50'
  cfg.train.tensorboard_step = tensorboard_step
  trainer = Trainer(cfg, DEV, softmax_head=True, channels_last=True)
  summary = TrainingSummary(str(directory), vis.voc_color_map(), cfg.train.batch_size)
  for it in range(steps):
    datas, targets = synth.make_batch(batch, crop, seed=100 + it, device=DEV)
    datas['image'] = datas['image'].contiguous(memory_format=torch.channels_last)
    torch.manual_seed(1000 + it)                           # the head's dropout mask
    trainer.step(datas, targets, summary)
  summary.close()
  state = {'emb.' + k: v.detach().clone() for k, v in trainer.embedding_model.named_parameters()}
  state.update({'pred.' + k: v.detach().clone() for k, v in trainer.prediction_model.named_parameters()})
  return state


def test_trainer_writes_summaries_and_trains_the_same(tmp_path):
  """Two steps with `tensorboard_step = 1` write two pictures and two lines; every parameter afterwards is
  bit-identical to a run with the step at 0, which creates no directory.  The library's deterministic mode is on; the
  framework's own convolutions (stem, res2, the stride-2 unit) have been seen to differ from run to run once in a
  while whatever this repository does (tests/test_determinism_gpu.py), so up to three pairs are run and one identical
  pair is the evidence: a summary that touched the training would never give one."""
  from PIL import Image
  before = _ffi.set_deterministic(True)
  try:
    for attempt in range(3):
      with_dir, without_dir = tmp_path / ('with%d' % attempt), tmp_path / ('without%d' % attempt)
      with_summary = _train(1, with_dir)
      without = _train(0, without_dir)
      differ = [k for k in without if not torch.equal(with_summary[k], without[k])]
      if attempt == 0:
        assert sorted(os.listdir(str(with_dir))) == ['image-0000000.png', 'image-0000001.png', 'scalars.jsonl']
        for name in ('image-0000000.png', 'image-0000001.png'):
          image = Image.open(str(with_dir / name))
          # (a 257 x 257 crop gives a 66 x 66 embedding, as 513 gives 130)
          assert image.mode == 'RGB' and image.size[::-1] == vis.summary_grid_shape(4, 66, 66)
          assert np.asarray(image).max() > 0
        lines = [json.loads(text) for text in open(str(with_dir / 'scalars.jsonl'))]
        assert [line['iter'] for line in lines] == [0, 1]
        assert lines[0]['images_per_s'] is None and lines[1]['images_per_s'] > 0
        assert {'sem_ann_loss', 'sem_occ_loss', 'img_sim_loss', 'accuracy', 'loss', 'lr', 'step_ms'} <= set(lines[1])
      assert not without_dir.exists()
      if not differ:
        break
      print('attempt %d: %d of %d tensors differ (first: %s)' % (attempt, len(differ), len(without), differ[:4]))
  finally:
    _ffi.set_deterministic(before)
  assert not differ, differ[:8]
