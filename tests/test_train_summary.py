"""Training summaries without a GPU: the fp64 yardstick (tests/train_summary_ref.py) against the reference's own
output (tests/golden/n16_train_summary.npz, tools/gen_golden.py::gen_n16), the picture's geometry, the sign rule, the
host side of spml_amd.summary.TrainingSummary, and the new entries of the C-ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

import train_summary_ref as R
from spml_amd.utils.general import vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(0, 2, 64, 9, 11, 33, 41), (1, 1, 32, 8, 8, 8, 8)]      # (case, N, C, h, w, Hl, Wl) of the fixture

# Yardstick against the reference, in units of the stretched value (v - min) / (max - min) in [0, 1].  Largest
# deviation measured on the CPU over both cases and all channels: 9.2e-7 (case 0, third component; the reference
# works in fp32 from torch.svd, the yardstick in fp64 from eigh).  The bound is four times that; the ceiling is a
# quarter of a byte step.
YARDSTICK_BOUND = 3.7e-6
YARDSTICK_CEILING = 1e-3

NEW_SYMBOLS = {'spml_train_summary_workspace_bytes': 4, 'spml_pca_path_name': 3, 'spml_pca_moments_f32': 12,
               'spml_pca_project_minmax_f32': 13, 'spml_summary_panels_u8': 15}


@pytest.fixture(scope='module')
def gold():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'n16_train_summary.npz'))


@pytest.fixture(scope='module')
def chains(gold):
  """The yardstick's whole chain per fixture case, computed once."""
  return {ci: R.chain(gold['c%d_embedding' % ci], gold['c%d_semantic' % ci], gold['c%d_instance' % ci], gold['color_map'])
          for ci, *_ in CASES}


@pytest.mark.parametrize('case', CASES)
def test_yardstick_against_the_reference(gold, chains, case):
  ci, n, c, h, w, hl, wl = case
  out, t = chains[ci], 'c%d_' % ci
  assert YARDSTICK_BOUND <= YARDSTICK_CEILING
  lam = R.eigenvalues(out['cov'])[:4]
  assert (lam[:-1] >= 1.5 * lam[1:]).all(), lam            # (a degenerate pair would make the components arbitrary)
  assert gold[t + 'embedding'].shape == (n, c, h, w) and gold[t + 'semantic'].shape == (n, hl, wl)
  ours, ref = out['t'] / 255.0, gold[t + 'floats'].astype(np.float64) / 255.0
  worst = 0.0
  for k in range(3):                                       # the sign freedom: the reference's channel or its mirror
    dev = min(np.abs(ours[..., k] - ref[..., k]).max(), np.abs(ours[..., k] - (1.0 - ref[..., k])).max())
    print('case %d channel %d: stretched value deviates by %.3e' % (ci, k, dev))
    worst = max(worst, dev)
  assert worst <= YARDSTICK_BOUND, worst
  # the reference's bytes are its floats truncated (and so are the yardstick's)
  assert np.array_equal(np.floor(gold[t + 'floats']).astype(np.uint8).transpose(0, 3, 1, 2), gold[t + 'bytes'])
  # label panels: every byte
  panels = gold[t + 'panels']
  assert panels.shape == (n, 3, h, 3 * w)
  for i, name in enumerate(('semantic', 'instance')):
    ours = R.label_panel(gold[t + name], gold['color_map'], h, w).transpose(0, 3, 1, 2)
    assert np.array_equal(ours, panels[:, :, :, i * w:(i + 1) * w]), name
  assert np.array_equal(panels[:, :, :, 2 * w:], gold[t + 'bytes'])


def test_nearest_rule_is_the_frameworks():
  """The yardstick's index rule against `F.interpolate(mode='nearest')` itself, over every pair of sizes up to 48 and
  the recipe's 513 -> 130 and 769 -> 193."""
  pairs = [(i, o) for i in range(1, 49) for o in range(1, 49)] + [(513, 130), (769, 193), (33, 9), (41, 11)]
  for size_in, size_out in pairs:
    ramp = torch.arange(size_in, dtype=torch.float32).view(1, 1, 1, size_in)
    want = torch.nn.functional.interpolate(ramp, size=(1, size_out), mode='nearest').view(-1).long().numpy()
    assert np.array_equal(R.nearest_index(size_out, size_in), want), (size_in, size_out)


def test_summary_grid_shape_and_placement():
  from spml_amd.summary import summary_grid_shape
  assert summary_grid_shape is vis.summary_grid_shape
  # make_grid(nrow=1, padding=2): cells of (h + 2) x (3 w + 2), one more padding at the bottom and on the right
  assert vis.summary_grid_shape(1, 9, 11) == (9, 33)
  assert vis.summary_grid_shape(2, 9, 11) == (2 * 11 + 2, 33 + 4)
  assert vis.summary_grid_shape(3, 5, 7) == (3 * 7 + 2, 21 + 4)
  assert [vis.summary_grid_padding(n) for n in (1, 2, 3)] == [0, 2, 2]
  color_map = vis.voc_color_map()
  for n, h, w in [(1, 4, 5), (2, 4, 5), (3, 3, 2)]:
    marker = 1                                             # one image all of label 1, the others of label 0 (black)
    for at in range(n):
      sem = np.zeros((n, h, w), dtype=np.int64)
      sem[at] = marker
      emb_bytes = np.zeros((n, h, w, 3), dtype=np.uint8)
      emb_bytes[at] = 200
      pic = R.picture(sem, np.zeros_like(sem), emb_bytes, color_map)
      assert pic.shape == (3,) + vis.summary_grid_shape(n, h, w)
      row, col = vis.summary_grid_origin(n, at, h)
      want = np.zeros_like(pic)
      want[:, row:row + h, col:col + w] = color_map[marker][:, None, None]            # semantic panel
      want[:, row:row + h, col + 2 * w:col + 3 * w] = 200                              # embedding panel
      assert np.array_equal(pic, want), (n, at)


def test_sign_rule():
  basis = np.array([[0.5, -0.5, 0.1, 0.0],
                    [-0.7, 0.5, -0.9, 0.0],
                    [0.1, 0.2, 0.9, -1.0]])
  got = vis.fix_component_signs(basis)
  # column 0: the lead -0.7 turns positive; 1: a tie of magnitude 0.5, the lowest index (negative) counts: flipped;
  # 2: a tie of 0.9, index 1 (negative) is lower: flipped; 3: -1 -> 1
  want = basis * np.array([-1.0, -1.0, -1.0, -1.0])
  assert np.array_equal(got, want) and np.array_equal(got, R.fix_signs(basis))
  keep = np.array([[0.9, 0.5], [-0.9, -0.2]])              # tie, the lower index is positive: unchanged
  assert np.array_equal(vis.fix_component_signs(keep), keep)
  assert np.array_equal(basis[:, 0], [0.5, -0.7, 0.1])     # (the argument is not modified)
  # eigenvectors of a known matrix: descending eigenvalues, leading entries positive
  cov = np.diag([1.0, 5.0, 3.0, 0.5])
  vectors, values = vis.leading_components(cov, 3)
  assert np.allclose(values, [5.0, 3.0, 1.0]) and np.allclose(vectors, np.eye(4)[:, [1, 2, 0]])


def test_leading_components_match_the_yardstick(chains):
  for ci, *_ in CASES:
    vectors, values = vis.leading_components(chains[ci]['cov'], 3)
    assert np.abs(vectors - chains[ci]['basis']).max() < 1e-9 and np.allclose(values, chains[ci]['values'])


class StubSummary:
  """TrainingSummary with the launches replaced: the picture is a fixed host tensor."""

  def __new__(cls, directory, batch_images=4):
    from spml_amd.summary import TrainingSummary

    class Stub(TrainingSummary):
      def picture(self, semantic_label, instance_label, embedding):
        pic = torch.zeros(3, 6, 10, dtype=torch.uint8)
        pic[0, 1, 2], pic[1, 3, 4], pic[2, 5, 9] = 255, 128, 7
        return pic
    return Stub(directory, vis.voc_color_map(), batch_images)


def test_training_summary_due():
  from spml_amd.summary import TrainingSummary
  assert [TrainingSummary.due(i, 100) for i in (0, 1, 99, 100, 200)] == [True, False, False, True, True]
  assert not any(TrainingSummary.due(i, 0) for i in (0, 1, 100))
  assert TrainingSummary.due(7, 1)


def test_training_summary_files(tmp_path):
  from PIL import Image
  directory = tmp_path / 'run' / 'summary'
  summary = StubSummary(str(directory), batch_images=4)
  assert not directory.exists()                            # nothing is created before the first write
  scalars = {'sem_ann_loss': torch.tensor(1.5), 'sem_occ_loss': 0.25, 'img_sim_loss': None, 'accuracy': torch.tensor(0.5),
             'loss': torch.tensor(1.75), 'lr': 3e-3}
  summary.write(0, None, None, None, scalars)
  summary.write(2, None, None, None, scalars)
  summary.close()
  lines = [json.loads(line) for line in open(str(directory / 'scalars.jsonl'))]
  assert [sorted(line) for line in lines] == [sorted(['iter', 'sem_ann_loss', 'sem_occ_loss', 'accuracy', 'loss', 'lr',
                                                      'step_ms', 'images_per_s'])] * 2
  assert lines[0]['iter'] == 0 and lines[0]['images_per_s'] is None and lines[0]['step_ms'] is None
  assert lines[0]['sem_ann_loss'] == 1.5 and lines[0]['lr'] == 3e-3
  assert lines[1]['iter'] == 2 and lines[1]['step_ms'] > 0
  # wall clock over the two steps since the previous line, with the global batch
  assert abs(lines[1]['images_per_s'] - 4 * 1e3 / lines[1]['step_ms']) <= 1e-6 * lines[1]['images_per_s']
  assert sorted(os.listdir(str(directory))) == ['image-0000000.png', 'image-0000002.png', 'scalars.jsonl']
  image = Image.open(str(directory / 'image-0000002.png'))
  assert image.mode == 'RGB' and image.size == (10, 6)
  pixels = np.asarray(image)
  assert pixels[1, 2, 0] == 255 and pixels[3, 4, 1] == 128 and pixels[5, 9, 2] == 7 and pixels.sum() == 255 + 128 + 7


def test_no_directory_without_a_due_step(tmp_path):
  """What Trainer.step does with a summary: `due` first, `write` only then."""
  directory = tmp_path / 'summary'
  summary = StubSummary(str(directory))
  for it in range(3):
    if summary.due(it, 0):
      summary.write(it, None, None, None, {})
  summary.close()
  assert not directory.exists()


def _declaration(name):
  text = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  found = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', text)
  assert found, name + ' is not declared in include/spml_hip.h'
  return [a for a in found.group(1).split(',') if a.strip() and a.strip() != 'void']


def test_new_symbols_are_declared_and_bound():
  from spml_amd import _ffi
  for name, nargs in NEW_SYMBOLS.items():
    assert name in _ffi.EXPORTS, name
    assert len(_declaration(name)) == nargs == len(_ffi._SIGNATURES[name][1]), name
  from spml_amd import ops
  for name in ('pca_moments', 'pca_project_minmax', 'summary_panels', 'pca_path_name'):
    assert callable(getattr(ops, name)) and callable(getattr(_ffi, name))


def test_pca_path_names():
  from spml_amd import _build, ops
  _build.build(verbose=False)
  assert ops.pca_path_name(32, 32, 1) == 'gram_mfma_f32_c32'
  assert ops.pca_path_name(64, 64, 1) == 'gram_mfma_f32_c64'
  assert ops.pca_path_name(32, 1, 35) == 'gram_mfma_f32_c32_nchw'
  assert ops.pca_path_name(64, 1, 130 * 130) == 'gram_mfma_f32_c64_nchw'
  assert ops.pca_path_name(64, 1, 1) == 'gram_mfma_f32_c64_nchw'           # a 1 x 1 map: either storage, same bytes
  for c in (48, 128, 16, 0):
    assert ops.pca_path_name(c, c, 1) == 'unsupported' and ops.pca_path_name(c, 1, 99) == 'unsupported'
  assert ops.pca_path_name(64, 128, 1) == 'unsupported' and ops.pca_path_name(64, 64, 2) == 'unsupported'
  from spml_amd import _ffi
  lib = _ffi.lib()
  assert lib.spml_train_summary_workspace_bytes(16, 64, 130, 130) >= 256 * 64 * 64 * 4
  assert lib.spml_train_summary_workspace_bytes(2, 48, 9, 11) == 0
  assert lib.spml_train_summary_workspace_bytes(2, 64, 32768, 32768) == 0   # P >= 2^31
  assert lib.spml_train_summary_workspace_bytes(0, 64, 9, 11) == 0


def test_embedding_to_rgb_refuses_the_random_projection():
  with pytest.raises(ValueError, match='random'):
    vis.embedding_to_rgb(torch.zeros(1, 32, 2, 2), 'random')
  with pytest.raises(NotImplementedError):
    vis.embedding_to_rgb(torch.zeros(1, 32, 2, 2), 'tsne')


def test_convert_label_to_color_masks_with_255():
  table = vis.voc_color_map()
  label = torch.tensor([[[0, 1, 255], [256 + 2, 20, 3]]])
  got = vis.convert_label_to_color(label, table)
  assert got.shape == (1, 3, 2, 3) and got.dtype == torch.uint8
  assert np.array_equal(got.numpy(), table[np.array([[[0, 1, 255], [2, 20, 3]]])].transpose(0, 3, 1, 2))
