#!/usr/bin/env python3
"""Stage 2 of the DensePose recipe (`pyscripts/train/train_densepose_classifier.py` of twke18/SPML): the softmax
classifier on the frozen DensePose embedding network -- the loop of train_classifier.py with the DensePose PSPNet
(`panoptic_pspnet_101` only, :75-78; `prediction_types` `softmax_classifier`, :80-83) and DenseposeClassifierDataset
(random grayscale and blur on, :53-64) bound.  "Pre-trained model is required" (:102); the same two snapshot files.

  python3 pyscripts/train/train_densepose_classifier.py --data_dir D --data_list L --snapshot_dir S --cfg_path C.yaml
  python3 pyscripts/train/train_densepose_classifier.py --snapshot_dir S --cfg_path C.yaml [--data_list synthetic]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_classifier as _train_classifier  # noqa: E402


def main(argv=None):
  _train_classifier.main(argv, dataset='densepose',
                         description='Training for softmax classifier only on DensePose.')


if __name__ == '__main__':
  main()
