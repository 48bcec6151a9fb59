#!/usr/bin/env python3
"""Generate the multi-scale memory banks of the kNN inference, with the reference's command line and config surface
(`pyscripts/inference/prototype_msc.py` of twke18/SPML; the recipes run it before `inference_msc.py`):

  python3 pyscripts/inference/prototype_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --kmeans_num_clusters 12,12 --label_divisor 2048

Three views per image (scales 0.5, 1, 1.5, no flip: :92-95); per view the sliding-window embedding, k-means that ignores
the padding, prototypes and their majority labels; the views' banks concatenated into
`<save_dir>/semantic_prototype/<name>.npy`; see `run_prototypes` of spml_amd/inference_cli.py.  `--data_dir D
--data_list L` reads the reference's file list with its label columns; `--data_list synthetic` feeds seeded synthetic
images."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 1, 1.5]


def main(argv=None):
  from spml_amd.inference_cli import run_prototypes
  run_prototypes('Inference for generating memory banks.', SCALES, argv)


if __name__ == '__main__':
  main()
