#!/usr/bin/env python3
"""Multi-scale + flip inference by the softmax classifier with denseCRF refinement, with the reference's command line and
config surface (`pyscripts/inference/inference_softmax_crf_msc.py:30-177` of twke18/SPML), the last step of the tag
recipe:

  python3 pyscripts/inference/inference_softmax_crf_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT \\
      --data_list L --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the sum of the ten views' class probabilities is `inference_softmax_msc.py`
(`spml_amd.inference.predict_softmax_multiscale`).  Then the mean over the views (:156), the uint8 image rebuilt from
the network's input (:159-164, `denormalized_uint8`) and `spml_amd.inference.dense_crf_refine`: the exact mean-field
filter as HIP kernels (`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals
(:168); the JSON line carries what `inference_softmax_msc.py --crf` reports: the body is that program's, `run_softmax` of
spml_amd/inference_cli.py, with the CRF on and file lists refused (`inference_softmax_msc.py --crf` reads them)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :102


def main(argv=None):
  from spml_amd.inference_cli import run_softmax
  run_softmax('Inference for semantic segmentation.', SCALES, True, argv, file_lists=None, crf=True)


if __name__ == '__main__':
  main()
