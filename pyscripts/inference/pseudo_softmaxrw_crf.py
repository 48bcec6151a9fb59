#!/usr/bin/env python3
"""Generate pseudo labels by the softmax classifier, a random walk over the pixel affinity and denseCRF refinement, with
the reference's command line and config surface (`pyscripts/inference/pseudo_softmaxrw_crf.py:33-204` of twke18/SPML; the
scribble / point / box recipes run it between stage 1 and stage 2):

  python3 pyscripts/inference/pseudo_softmaxrw_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the walked maps is `pseudo_softmaxrw.py` (flip pair at scale 1, softmax per view and mean of the
probabilities, WALK_STEPS = 6 squarings of the transition matrix: :29, :109-112, :143-147, :165-170).  The walked maps at
1/8 of the image then go with the uint8 image rebuilt from the network's input (:179-184, `denormalized_uint8`) through
one fused call (`spml_amd.inference.pseudo_labels_softmax_crf`): the CRF's first kernel up-samples them
(:173-175), writes the label before the CRF (:176) and starts the exact mean-field filter (`spml_amd.models.crf.DenseCRF`,
DESIGN 8j).  Label maps are the arg-max of the refined marginals (:187), written as `semantic_gray/<name>.npy`; the JSON
line carries what `pseudo_softmaxrw.py` reports, scored on the refined labels, plus `mIoU_before_crf`, `changed_by_crf`
(the share of pixels whose label the CRF changed), `crf_path` and `crf_share`, the CRF's share of the image time.  The
body is `run_pseudo_softmax` of spml_amd/inference_cli.py with the CRF on and file lists refused;
`pseudo_softmaxrw.py --crf` runs the same on a list."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES, COMBINE, WALK_STEPS = (1,), 'prob_mean', 6                                            # :109-112, :143-147, :29


def main(argv=None):
  from spml_amd.inference_cli import run_pseudo_softmax
  run_pseudo_softmax('Generate pseudo labels by softmax classifier, random walk and CRF.', SCALES, COMBINE, WALK_STEPS,
                     argv, file_lists=None, crf=True)


if __name__ == '__main__':
  main()
