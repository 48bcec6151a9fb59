"""Instance-weighted IoU on the GPU: `spml_amd.utils.general.metrics.instance_class_counts` (the majority-label kernel
with the instance id as the segment) and the accumulator `InstanceIoU` against the fixture exec'd from
pyscripts/benchmark/benchmark_by_instance.py (tests/golden/n11_instance_iou.npz; tests/test_instance_iou.py keeps it
honest on the CPU)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from spml_amd.utils.general import metrics
from test_instance_iou import CASES, fixture_images

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('nc', sorted(CASES))
def test_instance_counts_and_weighted_iou_match_the_reference_lines(nc):
  g = load_golden('n11_instance_iou')
  acc = metrics.InstanceIoU(nc)
  for pred, gt, inst, want in fixture_images(g, nc):
    pred, gt, inst = (torch.from_numpy(a).to(DEV) for a in (pred, gt, inst))
    counts = metrics.instance_class_counts(inst, gt, nc)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (nc,) and counts.is_cuda
    assert np.array_equal(counts.cpu().numpy(), want.astype(np.int64))
    assert np.array_equal(acc.update(pred, gt, inst), want)
  result = acc.result()
  err = np.abs(result['iou'] - g['n%d_iou' % nc].numpy()).max()
  print('%d classes: instance-weighted mean IoU %.6f (fixture %.6f), max |iou - fixture| %.3e'
        % (nc, result['mean_iou'], g['n%d_mean_iou' % nc], err))
  assert result['iou'].dtype == np.float64 and err <= 1e-12
  assert abs(result['mean_iou'] - g['n%d_mean_iou' % nc]) <= 1e-12


def test_instance_counts_take_any_integer_maps():
  """int64 maps of another shape (what the program hands over), an id that does not occur counts nowhere, and one id over
  the whole image counts once, for the class most of its labelled pixels carry."""
  gt = torch.tensor([[1, 1, 255, 4], [4, 4, 20, 255]], device=DEV)
  inst = torch.full((2, 4), 9, device=DEV)
  assert metrics.instance_class_counts(inst, gt, 5).tolist() == [0, 0, 0, 0, 1]
  inst[0, :2] = 0
  assert metrics.instance_class_counts(inst, gt, 5).tolist() == [0, 1, 0, 0, 1]
  assert metrics.instance_class_counts(inst, torch.full_like(gt, 255), 5).tolist() == [2, 0, 0, 0, 0]
