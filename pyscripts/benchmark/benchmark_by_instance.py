#!/usr/bin/env python3
"""Scores a directory of predicted label maps by the instance-weighted IoU of the tag recipe, with the reference's
command line and printed lines (`pyscripts/benchmark/benchmark_by_instance.py` of twke18/SPML):

  python3 pyscripts/benchmark/benchmark_by_instance.py --pred_dir P --gt_dir G --inst_dir I [--num_classes 21]
                                                        [--string_replace a,b]

Every file under P (`os.walk`) is paired with the files of the same path under G and I; predictions and ground truth
are read as 8-bit gray, instance masks in PIL's mode `P`.  Per file: its own IoU per class, weighted by the number of
instance ids whose most frequent ground-truth class that is.  The counts of a batch of files come from one call of
`spml_score_batch_u8` (`spml_amd.utils.general.metrics.DirectoryScorer`); the float64 accumulation is the reference's.
Printed: the directory, `class <name>: <index>, acc: <value>%` per class, `mean IOU`, then one JSON line (files,
seconds, images/s, score_path, mean_iou).  Deviations and guards as in benchmark_by_mIoU.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd import benchmark_cli
  return benchmark_cli.run(argv, with_instances=True)


if __name__ == '__main__':
  main()
