"""Instance-weighted IoU, the part that needs no GPU: the fixture (tests/golden/n11_instance_iou.npz, exec'd from
pyscripts/benchmark/benchmark_by_instance.py:27-55 / :88-116 / :139 by tools/gen_golden.py) against a numpy restatement
kept here, quirks included.  `spml_amd.utils.general.metrics` is checked against the same fixture on the GPU
(tests/test_instance_iou_gpu.py)."""
import numpy as np
import pytest

from conftest import load_golden

CASES = {21: 3, 15: 2}                 # classes -> images


def fixture_images(g, nc):
  assert g['n%d_images' % nc] == CASES[nc]
  images = []
  for ii in range(CASES[nc]):
    t = 'n%d_i%d_' % (nc, ii)
    pred, gt, inst = (g[t + k].numpy() for k in ('pred', 'gt', 'inst'))
    assert pred.dtype == gt.dtype == inst.dtype == np.uint8 and pred.shape == gt.shape == inst.shape == (40, 52)
    images.append((pred, gt, inst, g[t + 'ninst'].numpy()))
  return images


def restated_instance_counts(inst, gt, nc):
  """benchmark_by_instance.py:97-108: per occurring instance id the most frequent ground-truth class below `nc` (ties and
  an id without such a pixel: the lowest class, 0); the 256th id is dropped."""
  counts = np.zeros(nc, dtype=np.float64)
  for i, ind in enumerate(np.unique(inst)):
    if i < 255:
      classes = gt[inst == ind].astype(np.int64)
      counts[np.argmax(np.bincount(classes[classes < nc], minlength=nc))] += 1
  return counts


def restated_image_iou(pred, gt, nc):
  """benchmark_by_instance.py:27-55, :111 for predictions below `nc`."""
  locs = gt < nc
  tp_fn = np.bincount(gt[locs], minlength=nc).astype(np.float64)
  tp_fp = np.bincount(pred[locs], minlength=nc).astype(np.float64)
  tp = np.bincount(gt[locs & (pred == gt)], minlength=nc).astype(np.float64)
  return tp / (tp_fn + tp_fp - tp + 1e-12)


@pytest.mark.parametrize('nc', sorted(CASES))
def test_fixture_is_reproduced_by_numpy(nc):
  g = load_golden('n11_instance_iou')
  iou, ninst = np.zeros(nc), np.zeros(nc)
  for pred, gt, inst, want in fixture_images(g, nc):
    assert int(pred.max()) < nc
    counts = restated_instance_counts(inst, gt, nc)
    assert np.array_equal(counts, want)
    iou += restated_image_iou(pred, gt, nc) * counts
    ninst += counts
  iou = iou / (ninst + 1e-12) * 100
  assert np.abs(iou - g['n%d_iou' % nc].numpy()).max() <= 1e-12
  assert abs(iou.sum() / nc - g['n%d_mean_iou' % nc]) <= 1e-12


@pytest.mark.parametrize('nc', sorted(CASES))
def test_fixture_holds_the_quirks(nc):
  g = load_golden('n11_instance_iou')
  images = fixture_images(g, nc)
  pred, gt, inst, ninst = images[0]                           # a few instances over a blocky ground truth
  ids = np.unique(inst)
  assert {0, 3, 5, 255} <= set(ids.tolist()) and ninst.sum() == ids.size       # id 0 counts as an instance
  assert (gt[inst == 3] == 255).all()                         # an instance without a labelled pixel: counted for class 0
  without = [i for i in ids if i != 3]
  mask = np.isin(inst, without)
  assert restated_instance_counts(np.where(mask, inst, without[0]), gt, nc)[0] == ninst[0] - 1
  five = np.bincount(gt[inst == 5], minlength=256)[:nc]       # an instance tied between two classes: the lower one
  a, b = np.flatnonzero(five == five.max())
  only5 = restated_instance_counts(np.where(inst == 5, 5, 0).astype(np.uint8)[inst == 5], gt[inst == 5], nc)
  assert a < b and only5[a] == 1 and only5.sum() == 1
  assert ((gt >= nc) & (gt < 255)).any()                      # values that are neither a class nor 255
  pred, gt, inst, ninst = images[1]                           # all 256 ids: the largest is dropped
  assert np.unique(inst).size == 256 and ninst.sum() == 255
  if nc == 21:
    pred, gt, inst, ninst = images[2]                         # one id
    assert np.unique(inst).size == 1 and ninst.sum() == 1 and ninst.max() == 1


def test_histogram_bins_the_classes_as_themselves():
  """`np.histogram(bins=nc, range=(0, nc - 1))` (:104-106) has bins of width (nc - 1) / nc: the integers 0 .. nc - 1
  still fall one per bin, in order, and everything from nc on falls outside."""
  for nc in sorted(CASES):
    hist, _ = np.histogram(np.arange(nc), bins=nc, range=(0, nc - 1))
    assert hist.tolist() == [1] * nc
    for v in range(nc):
      assert int(np.argmax(np.histogram(np.array([v]), bins=nc, range=(0, nc - 1))[0])) == v
    assert np.histogram(np.array([nc, nc + 1, 254, 255]), bins=nc, range=(0, nc - 1))[0].sum() == 0
