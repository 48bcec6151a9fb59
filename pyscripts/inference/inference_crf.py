#!/usr/bin/env python3
"""Single-view inference for semantic segmentation by nearest-neighbour retrieval with denseCRF refinement, with the
reference's command line and config surface (`pyscripts/inference/inference_crf.py:35-280` of twke18/SPML):

  python3 pyscripts/inference/inference_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048 \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the clustering is `inference.py` (:145-229).  The retrieval then stays per segment
(`Segsort.segment_predictions`: `[m, 20]` labels and one segment id per pixel), and the vote map of :240-245 goes with the
uint8 image rebuilt from the network's input (:247-252, `denormalized_uint8`) through one fused call
(`spml_amd.inference.predict_knn_full_resolution_crf`): votes, log p and Q_0 are formed once per segment, the
CRF's first kernel gathers them per pixel, writes the label before the CRF and starts the exact mean-field filter
(`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:257), written as
`semantic_gray/<name>.npy`; the JSON line carries what `inference.py` reports, scored on the refined labels, plus
`mIoU_before_crf`, `changed_by_crf` (the share of pixels whose label the CRF changed), `crf_path`, `votes_path` and
`crf_share`, the CRF's share of the image time.  The reference's resize to `test.image_size` and the nearest-neighbour
resize of the label map back (:133-142, :258-261) are built where files are read: the body is `run_knn` of
spml_amd/inference_cli.py with the CRF on and file lists refused, and `inference.py --crf` runs the same on a list."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd.inference_cli import run_knn
  run_knn('Inference for semantic segmentation.', [1], False, argv, single_view=True, file_lists=None, crf=True)


if __name__ == '__main__':
  main()
