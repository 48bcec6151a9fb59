#!/usr/bin/env python3
"""Scores a directory of predicted label maps against a directory of ground truth, with the reference's command line
and printed lines (`pyscripts/benchmark/benchmark_by_mIoU.py` of twke18/SPML):

  python3 pyscripts/benchmark/benchmark_by_mIoU.py --pred_dir P --gt_dir G [--num_classes 21] [--string_replace a,b]

Every file under P (`os.walk`) is paired with the file of the same path under G (`str.replace` of the directory prefix,
then of `a` by `b`), both read as 8-bit gray.  The host only decodes; the per-file counts of a batch of files come from
one call of `spml_score_batch_u8` (`spml_amd.utils.general.metrics.DirectoryScorer`), the float64 sums and the IoU lines
are the reference's.  Printed: the directory, `class <name>: <index>, acc: <value>%` per class, `mean IOU`, `mean Pixel
Acc`, then one JSON line (files, seconds, images/s, score_path, mean_iou).  Deviation: for a class count other than 15
and 21 the reference raises NotImplementedError after computing everything; here the lines carry the index as the name.
Unlike the reference's asserts and numpy errors, a missing directory, an empty one, a prediction without its partner and
files of differing size end the program with a message that names the path; so does a machine without a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd import benchmark_cli
  return benchmark_cli.run(argv, with_instances=False)


if __name__ == '__main__':
  main()
