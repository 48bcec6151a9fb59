#!/usr/bin/env python3
"""Inference for semantic segmentation by the softmax classifier, with the reference's command line and config
surface (`pyscripts/inference/inference_softmax.py:26-166` of twke18/SPML):

  python3 pyscripts/inference/inference_softmax.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:70-76): `embedding_model` through the reference's
name mapping (`resume=True`), `prediction_model` non-strictly -- a stage-1 `SegsortSoftmax` snapshot carries the same
`semantic_classifier.*` names next to entries this model does not have.  Every image goes through
`spml_amd.inference.predict_softmax_full_resolution` (sliding windows, HIP classifier head, summed logits, arg-max).
The evaluation file-list loader is outside this repository: `--data_list synthetic` feeds seeded
synthetic images of `test.image_size`, padded to the crop size (:97-103).  Label maps are written as
`semantic_gray/<name>.npy` (uint8; no image library is needed); one JSON line reports images/s and, where labels
exist, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'predict_softmax_full_resolution')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'softmax_classifier')   # :63-76
  num_classes, crop_size, stride, size = cli.geometry(config)
  counts, out = None, None

  def one(index):
    nonlocal counts, out
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]                   # resize_with_pad, :97-103
    out = inference.predict_softmax_full_resolution(embedding_model, prediction_model, padded, (size, size), crop_size,
                                                    stride)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    cli.save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), head_path=out['head_path'], snapshot=path, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
