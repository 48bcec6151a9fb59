#!/usr/bin/env python3
"""Generate the memory banks of the kNN inference, with the reference's command line and config surface
(`pyscripts/inference/prototype.py` of twke18/SPML; the recipes run it before `inference.py`):

  python3 pyscripts/inference/prototype.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --kmeans_num_clusters 12,12 --label_divisor 2048

One view per image at its own size: the pass of `prototype_msc.py` with the scales `[1]`; the bank of every image goes
to `<save_dir>/semantic_prototype/<name>.npy`; see `run_prototypes` of spml_amd/inference_cli.py.  `--data_dir D
--data_list L` reads the reference's file list with its label columns (image and label go to `test.image_size` first,
:96-105); `--data_list synthetic` feeds seeded synthetic images."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [1]


def main(argv=None):
  from spml_amd.inference_cli import run_prototypes
  run_prototypes('Inference for generating memory banks.', SCALES, argv, single_view=True)


if __name__ == '__main__':
  main()
