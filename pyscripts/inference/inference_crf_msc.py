#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by nearest-neighbour retrieval with denseCRF refinement, with
the reference's command line and config surface (`pyscripts/inference/inference_crf_msc.py:35-283` of twke18/SPML):

  python3 pyscripts/inference/inference_crf_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048 \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the mean of the views' vote maps is `inference_msc.py` (`spml_amd.inference.predict_knn_multiscale`,
whose `semantic_prob` is the view mean of :246-248).  That map goes with the uint8 image rebuilt from the network's input
(:251-256, `denormalized_uint8`) through `spml_amd.inference.dense_crf_refine`: the exact mean-field filter as HIP
kernels (`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:260); the
JSON line carries what `inference_msc.py --crf` reports: the body is that program's, `run_knn` of
spml_amd/inference_cli.py, with the CRF on and file lists refused (`inference_msc.py --crf` reads them)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :135


def main(argv=None):
  from spml_amd.inference_cli import run_knn
  run_knn('Inference for semantic segmentation.', SCALES, True, argv, file_lists=None, crf=True)


if __name__ == '__main__':
  main()
