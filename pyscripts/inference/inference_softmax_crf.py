#!/usr/bin/env python3
"""Inference for semantic segmentation by the softmax classifier with denseCRF refinement, with the reference's command
line and config surface (`pyscripts/inference/inference_softmax_crf.py:27-176` of twke18/SPML), the last step of the box
recipe:

  python3 pyscripts/inference/inference_softmax_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the summed logits is `inference_softmax.py` (`spml_amd.inference.predict_softmax_full_resolution`).
Then the soft-max over the classes cropped to the image (:153-154), the uint8 image rebuilt from the network's input
(:158-164, `denormalized_uint8`) and `spml_amd.inference.dense_crf_refine`: the exact mean-field filter as HIP kernels
(`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:169); the JSON line
carries what `inference_softmax.py --crf` reports: the body is that program's, `run_softmax` of spml_amd/inference_cli.py,
with the CRF on and file lists refused (`inference_softmax.py --crf` reads them)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd.inference_cli import run_softmax
  run_softmax('Inference for semantic segmentation.', [1], False, argv, single_view=True, file_lists=None, crf=True)


if __name__ == '__main__':
  main()
