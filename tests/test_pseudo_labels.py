"""Pseudo-label generation, the parts that need no GPU: the fixture tests/golden/n7_pseudo_labels.npz (exec'd from
pyscripts/inference/pseudo_softmaxrw_crf.py:130-170 and pseudo_softmax.py:129-173 by tools/gen_golden.py) against the
plain-torch restatement tests/pseudo_label_ref.py, the two host helpers, and the no-CPU-fallback rule of the new
wrappers and programs.

The walked maps of the six-squaring recipes are the one quantity here whose fp32 bits depend on the host's GEMM: every
squaring doubles the rounding error of the one before, so two summation orders end 2^6 roundings apart.  The fixture
was generated single-threaded, and the comparison below runs single-threaded as well (as tests/test_oracle_golden.py
does); on the generating CPU model every stored array is reproduced bit for bit at 1 thread and within 2.5e-7 relative
at 2 - 8 threads.  Measured on a host of another CPU model (other GEMM kernels of the same library): `cam_rw` of case
0, recipe `rw`, 1.98e-6 relative / 1.49e-6 absolute on 3 of 3465 values against the bar of 1e-6 / 1e-7 -- that host
misses the bar for this one array; every other stored array is within it there too.  For scale: the stored fp32
`cam_rw` of the six-squaring recipes is itself 2.2e-6 - 3.3e-6 relative (0.8e-6 - 1.3e-6 absolute) from the same walk
carried out in fp64, so 1e-6 / 1e-7 can only be met by a host whose GEMM sums in the generator's order; without
squarings (`sm0`) the distance is 3.3e-7 / 1.2e-7."""
import importlib.util
import os

import pytest
import torch

import pseudo_label_ref as ref
from conftest import load_golden

torch.set_num_threads(1)                  # the generator's setting (tools/gen_golden.py): bit-stable fp32 sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = dict(rtol=1e-6, atol=1e-7)          # oracle against golden


def load_program(name):
  spec = importlib.util.spec_from_file_location('spml_' + name, os.path.join(ROOT, 'pyscripts', 'inference', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.mark.parametrize('ci', range(ref.NUM_CASES))
def test_fixture_is_reproduced_by_plain_torch(ci):
  g = load_golden('n7_pseudo_labels')
  assert g['recipes'] == ['%s:%s:%d' % r for r in ref.RECIPES]
  outputs, meta, image_hw, tags = ref.fixture_case(g, ci)
  t = 'c%d_' % ci
  assert len(meta) == (2, 4)[ci] and [m[2] for m in meta[:2]] == [True, False]       # per scale the flipped view first
  assert any(m[0] < o[0].shape[2] for m, o in zip(meta, outputs))                    # rh < Hp
  assert len({tuple(o[0].shape) for o in outputs}) == (1, 2)[ci]                     # one padded size per scale
  assert 3 <= int(tags.sum()) <= 4 and bool(tags[0])
  for tag, combine, steps in ref.RECIPES:
    got = ref.pseudo_labels(outputs, meta, image_hw, tags, combine, steps)
    for vi, unit in enumerate(got['units']):
      torch.testing.assert_close(unit, g[t + 'unit%d' % vi], **BAR)
    torch.testing.assert_close(got['trans'], g[t + 'trans'], **BAR)
    torch.testing.assert_close(got['cam'], g[t + tag + '_cam'], **BAR)
    torch.testing.assert_close(got['cam_rw'], g[t + tag + '_cam_rw'], **BAR)
    # the stored margin is that of the stored cam_rw under the CPU yardstick, and the low-margin share is under the cap
    cam_rw = g[t + tag + '_cam_rw']
    assert tuple(cam_rw.shape) == (21, image_hw[0] // 8, image_hw[1] // 8)
    pred, margin = ref.labels_and_margin(cam_rw, image_hw)
    assert torch.equal(margin, g[t + tag + '_margin']) and tuple(margin.shape) == image_hw
    sure = margin >= ref.LOW_MARGIN * cam_rw.abs().max()
    assert (~sure).float().mean().item() <= 0.01
    assert torch.equal(got['semantic_prediction'][sure], pred[sure])
    assert pred.unique().numel() >= 3 and bool(tags[pred.unique()].all())
    # absent classes are exactly zero, present ones peak at one
    assert bool((g[t + tag + '_cam'][~tags] == 0).all())
    assert torch.equal(g[t + tag + '_cam'][tags].flatten(1).max(1).values, torch.ones(int(tags.sum())))
    # the walk is not the identity on this fixture
    assert g[t + 'trans'].diagonal().mean().item() < 0.8


def test_background_threshold_and_single_view_of_the_restatement():
  g = load_golden('n7_pseudo_labels')
  outputs, meta, image_hw, tags = ref.fixture_case(g, 0)
  got = ref.pseudo_labels(outputs[:1], meta[:1], image_hw, tags, 'prob_mean', 1, threshold=0.25)
  assert bool((got['cam'][0] == 0.25).all()) and bool((got['cam'][~tags] == 0).all())
  torch.testing.assert_close(got['trans'].sum(0), torch.ones(got['trans'].shape[0]), rtol=1e-5, atol=0)


def test_label_tags_from_map():
  from spml_amd.inference import label_tags_from_map
  label = torch.tensor([[0, 3, 255], [3, 7, 20], [21, 20, 0]])
  tags = label_tags_from_map(label, 21)
  assert tags.dtype == torch.bool and tuple(tags.shape) == (21,)
  assert tags.nonzero().view(-1).tolist() == [0, 3, 7, 20]                 # 21 and 255 are not classes
  assert label_tags_from_map(label.to(torch.uint8).numpy(), 5).nonzero().view(-1).tolist() == [0, 3]


def test_flip_scale_views_order_padding_and_sizes():
  from spml_amd.inference import flip_scale_views
  image = torch.arange(24.0).view(1, 1, 4, 6).repeat(1, 3, 1, 1) + 1.0
  views = flip_scale_views(image, [0.75, 1], True, (5, 5))
  assert [(tuple(v.shape), hw, f) for v, hw, f in views] == [
      ((1, 3, 5, 5), (3, 4), True), ((1, 3, 5, 5), (3, 4), False),        # round(4 * .75) x round(6 * .75), padded to the crop
      ((1, 3, 5, 6), (4, 6), True), ((1, 3, 5, 6), (4, 6), False)]        # wider than the crop: only the height is padded
  plain, flipped = views[3][0], views[2][0]
  assert torch.equal(plain[:, :, :4, :6], image) and torch.equal(flipped[:, :, :4, :6], torch.flip(image, dims=[3]))
  assert bool((plain[:, :, 4:] == 0).all()) and bool((flipped[:, :, 4:] == 0).all())      # zero padding, top-left image
  small, small_f = views[1][0], views[0][0]
  assert bool((small[:, :, 3:] == 0).all()) and bool((small[:, :, :, 4:] == 0).all())
  assert torch.equal(small_f[:, :, :3, :4], torch.flip(small[:, :, :3, :4], dims=[3]))
  want = torch.nn.functional.interpolate(image, size=(3, 4), mode='bilinear', align_corners=False)
  assert torch.equal(small[:, :, :3, :4], want)
  only = flip_scale_views(image, [1], False, (2, 2))
  assert len(only) == 1 and only[0][2] is False and tuple(only[0][0].shape) == (1, 3, 4, 6)
  with pytest.raises(ValueError):
    flip_scale_views(image[0], [1], True, (5, 5))


def test_no_cpu_fallback_in_the_new_wrappers():
  from spml_amd import _ffi, inference
  emb, logit = torch.randn(8, 16, 24), torch.randn(5, 16, 24)
  tags = torch.ones(5, dtype=torch.bool)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.resample_unit(emb, (12, 20), True, (2, 3), torch.empty(1, 8, 6), 0)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.resample_classes_accumulate(logit, (12, 20), False, (2, 3), torch.zeros(5, 6))
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.cam_finalize(torch.rand(5, 6), 2, tags)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.upsample_argmax(torch.rand(5, 2, 3), 16, 24)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.resample_classes_accumulate(logit, (12, 20), False, (2, 3), torch.zeros(5, 6), combine='max')

  class Net(torch.nn.Module):
    num_classes = 5

    def generate_embeddings(self, datas, targets=None, resize_as_input=False):
      raise AssertionError('a CPU view must be refused before the network runs')

    def prepare_inference(self):
      raise AssertionError('a CPU view must be refused before the head is prepared')

  views = [(torch.zeros(1, 3, 16, 24), (12, 20), False)]
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    inference.pseudo_labels_softmax(Net(), Net(), views, (12, 20), tags)


@pytest.mark.parametrize('name,constants', [('pseudo_softmax', ((0.75, 1), 'logit_mean', 0)),
                                            ('pseudo_softmaxrw', ((1,), 'prob_mean', 6))])
def test_programs_carry_the_recipe_constants_and_refuse_to_run_without_a_gpu(name, constants, tmp_path):
  from test_train_cli import YAML
  prog = load_program(name)
  assert (tuple(prog.SCALES), prog.COMBINE, prog.WALK_STEPS) == constants
  if torch.cuda.is_available():
    return
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML)
  with pytest.raises(SystemExit) as info:
    prog.main(['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--save_dir', str(tmp_path / 'o'),
               '--data_list', 'synthetic'])
  assert info.value.code not in (0, None) and 'no CPU fallback' in str(info.value.code)
