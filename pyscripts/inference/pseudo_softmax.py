#!/usr/bin/env python3
"""Generate pseudo labels by the softmax classifier, with the reference's command line and config surface
(`pyscripts/inference/pseudo_softmax.py` of twke18/SPML; the tag recipe runs it between stage 1 and stage 2):

  python3 pyscripts/inference/pseudo_softmax.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Flip pairs at scales 0.75 and 1, mean of the views' logits and one softmax, WALK_STEPS = 0: the class maps go once
through the transition matrix, without squarings (:29, :108-111, :144-150).  The script's CRF lines are commented out,
so the labels written are its output: `semantic_gray/<name>.png` and `semantic_color/<name>.png` at the file's own size
under `--data_dir D --data_list L` (the reference's file list with its label columns, which give the image tags; the
folder `train_classifier.py --data_list` reads back), `semantic_gray/<name>.npy` under `--data_list synthetic`; see
`run_pseudo_softmax` of spml_amd/inference_cli.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES, COMBINE, WALK_STEPS = (0.75, 1), 'logit_mean', 0


def main(argv=None):
  from spml_amd.inference_cli import run_pseudo_softmax
  run_pseudo_softmax('Generate pseudo labels by softmax classifier.', SCALES, COMBINE, WALK_STEPS, argv)


if __name__ == '__main__':
  main()
