"""Launch order of the four random-walk pseudo-label functions of spml_amd/inference.py on the GPU: the `_ffi` entry
points they reach, the two model calls and the CRF's fused call are wrapped by recorders that call through, and the
sequence per image is pinned for `pseudo_labels_softmax`, `pseudo_labels_softmax_crf`, `pseudo_labels_cam` and
`pseudo_labels_cam_crf`.  One 65 x 65 image; the flip pair at scale 1 and the flip pair at scale 1.5, so that the views
fall into two groups of one padded size each (65 x 65, the crop size, and 98 x 98); two squarings; two CRF iterations.
Each plain / CRF pair must give bit-identical `cam`, `cam_rw` and labels before the CRF.  The network itself is not
repeatable run to run on this backbone -- two `generate_embeddings` calls on the same two 65 x 65 views differed by up
to 0.035 and on the 98 x 98 views by up to 0.048 (a seeded, untrained network; the library's deterministic mode on),
which moved `cam_rw` by 4e-7 (`pseudo_labels_cam`, all four views) and 8e-7 (`pseudo_labels_softmax`) and no label
(profiles/inference_programs.md has the table) -- and that is the framework's convolutions, not the code under test.
So the recorder of `generate_embeddings` calls through once per group of views and gives the second function of a pair
the tensors the first one got: everything behind the network, which is what the four functions consist of, is compared
bit for bit.  This departs from the issue, which asks for the pair as run: with the network run twice the assertion
holds on no commit.  The sequences were recorded before the two `_walked_cams_*` helpers took one view loop and one
tail; they are written out here, not generated."""
import numpy as np
import pytest
import torch

from spml_amd import _ffi, inference, inference_cli
from test_dense_crf_gpu import tiny_config, write_snapshot

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE, NCLS, WALK_STEPS = 65, 2, 2
RECORDED = ('cam_ingest', 'resample_unit', 'resample_classes_accumulate', 'affinity_transition', 'cam_finalize', 'upsample_argmax')
PER_VIEW_SOFTMAX = ['accumulate_logits', 'resample_unit', 'resample_classes_accumulate']
SOFTMAX = (['embed 2 x 65 x 65'] + PER_VIEW_SOFTMAX * 2 + ['embed 2 x 98 x 98'] + PER_VIEW_SOFTMAX * 2
           + ['affinity_transition', 'cam_finalize'])
CAM = (['cam_ingest', 'embed 2 x 65 x 65'] + ['resample_unit'] * 2 + ['embed 2 x 98 x 98'] + ['resample_unit'] * 2
       + ['affinity_transition'])


@pytest.fixture(autouse=True)
def deterministic_mode():
  """Without the mode the embedding's tap-group sums depend on the arrival order (tests/test_cam_lists_gpu.py)."""
  was = _ffi.set_deterministic(True)
  yield
  _ffi.set_deterministic(was)


@pytest.fixture(scope='module')
def stage(tmp_path_factory):
  from spml_amd.config.default import config
  from spml_amd.config.parse_args import parse_args
  root = tmp_path_factory.mktemp('launch_order')
  cfg = tiny_config(root, NCLS, 'softmax_classifier')
  snap = write_snapshot(root, cfg, 'softmax_classifier')
  args = parse_args('test', ['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--crf_iter_max', '2'])
  device = torch.device(DEV)
  embedding_model, prediction_model, _ = inference_cli.load_models(config, args, device, 'softmax_classifier')
  num_classes, crop_size, _, size = inference_cli.geometry(config)
  assert (num_classes, size, tuple(crop_size)) == (NCLS, SIZE, (SIZE, SIZE))
  image, _, _ = inference_cli.synthetic_image(0, size, num_classes, device)
  views = inference.flip_scale_views(image, [1, 1.5], True, crop_size)
  assert [tuple(v[0].shape[-2:]) for v in views] == [(65, 65)] * 2 + [(98, 98)] * 2 and [v[2] for v in views] == [True, False] * 2
  crf = inference_cli.CrfStage(config, args).crf
  assert crf.iter_max == 2
  image_u8 = inference.denormalized_uint8(image, config.network.pixel_means, config.network.pixel_stds)
  planes = torch.rand((1, SIZE, SIZE), generator=torch.Generator().manual_seed(3)).to(device)
  return dict(embedding_model=embedding_model, prediction_model=prediction_model, views=views, crf=crf, image_u8=image_u8,
              tags=torch.ones((NCLS,), dtype=torch.bool, device=device), planes=planes, keys=np.zeros((1,), np.int32))


@pytest.fixture
def launches(stage, monkeypatch):
  order = []

  def recorder(name, real):
    def call(*args, **kwargs):
      order.append(name)
      return real(*args, **kwargs)
    return call

  for name in RECORDED:
    monkeypatch.setattr(_ffi, name, recorder(name, getattr(_ffi, name)))
  monkeypatch.setattr(stage['prediction_model'], 'accumulate_logits',
                      recorder('accumulate_logits', stage['prediction_model'].accumulate_logits), raising=False)
  monkeypatch.setattr(stage['crf'], 'refine_upsampled', recorder('refine_upsampled', stage['crf'].refine_upsampled),
                      raising=False)
  embed, embedded = stage['embedding_model'].generate_embeddings, {}

  def generate_embeddings(datas, **kwargs):
    # (calls through once per group of views and hands the second function of a pair the same tensors: see the top)
    size = tuple(datas['image'].shape[i] for i in (0, 2, 3))
    order.append('embed %d x %d x %d' % size)
    if size not in embedded:
      embedded[size] = embed(datas, **kwargs)
    return embedded[size]
  monkeypatch.setattr(stage['embedding_model'], 'generate_embeddings', generate_embeddings, raising=False)
  return order


def check_pair(plain, refined, launches, chain):
  assert launches == chain + ['upsample_argmax'] + chain + ['refine_upsampled']
  for key in ('cam', 'cam_rw'):
    assert plain[key].dtype == torch.float32 and tuple(plain[key].shape) == (NCLS, SIZE // 8, SIZE // 8)
    assert torch.equal(plain[key], refined[key]), key
  assert plain['semantic_prediction'].dtype == torch.int64 and tuple(plain['semantic_prediction'].shape) == (SIZE, SIZE)
  assert torch.equal(plain['semantic_prediction'], refined['semantic_prediction_before_crf'])
  assert tuple(refined['semantic_prediction'].shape) == (SIZE, SIZE) and tuple(refined['semantic_prob'].shape) == (NCLS, SIZE, SIZE)
  assert refined['crf_path'].startswith('pairs_mfma_')


def test_softmax_walk_launch_order(stage, launches):
  common = (stage['embedding_model'], stage['prediction_model'], stage['views'], (SIZE, SIZE), stage['tags'])
  plain = inference.pseudo_labels_softmax(*common, combine='prob_mean', walk_steps=WALK_STEPS)
  refined = inference.pseudo_labels_softmax_crf(*common, stage['image_u8'], stage['crf'], combine='prob_mean',
                                                walk_steps=WALK_STEPS)
  check_pair(plain, refined, launches, SOFTMAX)
  assert set(plain) == {'cam', 'cam_rw', 'semantic_prediction', 'head_path'}
  assert set(refined) == {'cam', 'cam_rw', 'head_path', 'semantic_prob', 'semantic_prediction',
                           'semantic_prediction_before_crf', 'crf_path'}
  assert plain['head_path'] == refined['head_path']


def test_cam_walk_launch_order(stage, launches):
  common = (stage['embedding_model'], stage['views'], (SIZE, SIZE), stage['planes'], stage['keys'], NCLS)
  plain = inference.pseudo_labels_cam(*common, alpha=6, walk_steps=WALK_STEPS)
  refined = inference.pseudo_labels_cam_crf(*common, stage['image_u8'], stage['crf'], alpha=6, walk_steps=WALK_STEPS)
  check_pair(plain, refined, launches, CAM)
  assert set(plain) == {'cam', 'cam_rw', 'semantic_prediction', 'cam_path'}
  assert set(refined) == {'cam', 'cam_rw', 'cam_path', 'semantic_prob', 'semantic_prediction',
                           'semantic_prediction_before_crf', 'crf_path'}
  assert plain['cam_path'] == refined['cam_path']
