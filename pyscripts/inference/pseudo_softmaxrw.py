#!/usr/bin/env python3
"""Generate pseudo labels by the softmax classifier and a random walk over the pixel affinity, with the reference's
command line and config surface (`pyscripts/inference/pseudo_softmaxrw_crf.py` of twke18/SPML; the scribble / point /
box recipes run it between stage 1 and stage 2):

  python3 pyscripts/inference/pseudo_softmaxrw.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Flip pair at scale 1, softmax per view and mean of the probabilities, WALK_STEPS = 6 squarings of the transition
matrix (:29, :109-112, :143-147).  Writes the labels of :176, or with `--crf` (off by default) the labels of :187 after the denseCRF refinement
of `pseudo_softmaxrw_crf.py` (`spml_amd.inference.pseudo_labels_softmax_crf` on the guide image of the file, DESIGN 8r;
the JSON line gains `crf_path`, `crf_share`, `mIoU_before_crf` and `changed_by_crf`): `semantic_gray/<name>.png` and `semantic_color/<name>.png` at the file's own size under `--data_dir D
--data_list L` (the reference's file list with its label columns, which give the image tags), `semantic_gray/<name>.npy`
under `--data_list synthetic`; see `run_pseudo_softmax` of spml_amd/inference_cli.py.

With `--cam_dir CAMS` the program is the CAM walk of `pseudo_camrw_crf.py` (the first pseudo-label step of the image-tag
recipe; the two programs share everything but the source of the class maps), on either kind of `--data_list`:

  python3 pyscripts/inference/pseudo_softmaxrw.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_dir D \\
      --data_list L --cam_dir CAMS [--crf]

The embedding network alone is loaded; the class maps of an image come from `<cam_dir>/<name>.npy`, the reference's
pickled dict `{class - 1: [h, w]}` (`synthetic_%04d.npy` under `--data_list synthetic`), through one launch
(`spml_cam_ingest_f32`: the background `(1 - max_fg) ** ALPHA` and the 1/8 reduction, :108-111 and :151-152 there,
DESIGN 8s); the list needs no label columns (it is scored when it has them) and the JSON line carries `cam_dir`, `alpha`
and `cam_path` in place of `combine` and `head_path`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES, COMBINE, WALK_STEPS = (1,), 'prob_mean', 6
ALPHA = 6                                                                                     # pseudo_camrw_crf.py:28


def main(argv=None):
  from spml_amd.inference_cli import run_pseudo_softmax
  run_pseudo_softmax('Generate pseudo labels by softmax classifier and random walk.', SCALES, COMBINE, WALK_STEPS, argv,
                     crf=None, cam_alpha=ALPHA)


if __name__ == '__main__':
  main()
