#!/usr/bin/env python3
"""Single-view inference for semantic segmentation by nearest-neighbour retrieval, with the reference's command line and
config surface (`pyscripts/inference/inference.py:35-255` of twke18/SPML):

  python3 pyscripts/inference/inference.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory and the prototype memory bank from
`--semantic_memory_dir` (the ignore class dropped: :99-111).  Every image is zero-padded to the crop size and goes through
`spml_amd.inference.predict_full_resolution` (:136-237: sliding-window embedding, k-means over the whole image with the
padding ignored, top-20 retrieval per segment, majority vote, scatter to the pixels).  The evaluation
file-list loader is outside this repository: `--data_list synthetic` feeds seeded synthetic images of `test.image_size`
(made at the network's size: the reference's resize to `test.image_size` and the nearest-neighbour resize of the label map
back, :124-133 and :238-241, are file plumbing and not built).  Without `--semantic_memory_dir` the synthetic mode builds
the bank itself, as `inference_msc.py` does.  Label maps are written as `semantic_gray/<name>.npy` (uint8); one JSON line
reports images/s, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'predict_full_resolution')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :70-90
  num_classes, crop_size, stride, size = cli.geometry(config)
  memory_dir = args.semantic_memory_dir
  if memory_dir is None:
    memory_dir = cli.build_synthetic_bank(embedding_model, config, args, device)
  prototypes, prototype_labels = cli.load_bank(memory_dir, config, device)                    # :93-111
  counts = None

  def one(index):
    nonlocal counts
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]                   # :136-142
    out = inference.predict_full_resolution(embedding_model, prediction_model, padded, (size, size), crop_size, stride,
                                            prototypes, prototype_labels, config.dataset.semantic_ignore_index)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    cli.save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), memory_prototypes=int(prototypes.shape[0]), snapshot=path,
             semantic_memory_dir=memory_dir, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
