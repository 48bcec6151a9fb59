#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by the softmax classifier, with the reference's command line
and config surface (`pyscripts/inference/inference_softmax_msc.py:29-167` of twke18/SPML), the form every stage-2 recipe
reports its number through:

  python3 pyscripts/inference/inference_softmax_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:70-76): `embedding_model` through the reference's
name mapping (`resume=True`), `prediction_model` non-strictly -- a stage-1 `SegsortSoftmax` snapshot carries the same
`semantic_classifier.*` names next to entries this model does not have.  Every image becomes the ten views of
`spml_amd.inference.flip_scale_views` (scales 0.5, 0.75, 1, 1.25, 1.5, each flipped and plain, zero-padded to the crop
size: :90-103) and goes through `spml_amd.inference.predict_softmax_multiscale` (sliding windows and the HIP classifier
head per view, one HIP kernel per view for counts, crop, resize, softmax, un-flip and sum, one arg-max).  The
evaluation file-list loader is outside this repository: `--data_list synthetic` feeds seeded synthetic
images of `test.image_size`.  Label maps are written as `semantic_gray/<name>.npy` (uint8; no image library is needed);
one JSON line reports images/s, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`), the number of
views and the paths taken by the classifier head and by the per-view tail."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :92


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'predict_softmax_multiscale')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'softmax_classifier')   # :63-76
  num_classes, crop_size, stride, size = cli.geometry(config)
  counts, out, views = None, None, []

  def one(index):
    nonlocal counts, out, views
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, SCALES, True, crop_size)                        # :90-103
    out = inference.predict_softmax_multiscale(embedding_model, prediction_model, views, (size, size), crop_size, stride)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    cli.save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), views=len(views), head_path=out['head_path'],
             combine_path=out['combine_path'], snapshot=path, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
