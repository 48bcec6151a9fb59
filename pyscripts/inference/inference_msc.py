#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by nearest-neighbour retrieval, with the reference's command
line and config surface (`pyscripts/inference/inference_msc.py:35-255` of twke18/SPML), the form the recipes report
their kNN numbers through:

  python3 pyscripts/inference/inference_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory (:83-89) and the prototype memory bank from
`--semantic_memory_dir` (`segsort_others.load_memory_banks`, the ignore class dropped: :92-111).  Every image becomes
the ten views of `spml_amd.inference.flip_scale_views` (scales 0.5, 0.75, 1, 1.25, 1.5, each flipped and plain,
zero-padded to the crop size: :123-137) and goes through `spml_amd.inference.predict_knn_multiscale` (per view the
sliding-window embedding, k-means over the un-padded view, top-20 retrieval per segment and one HIP launch pair for
votes, resize, un-flip and sum; then the mean over the views and one arg-max).  The evaluation
file-list loader is outside this repository: `--data_list synthetic` feeds seeded synthetic images of
`test.image_size`.  Without `--semantic_memory_dir` the synthetic mode builds the bank itself: the prototypes of the
synthetic images (`full_resolution_prototypes`, what `prototype.py` does) are written with `save_image_memory` to
`<save_dir>/semantic_prototype` and read back from those files.  Label maps are written as `semantic_gray/<name>.npy`
(uint8; no image library is needed); one JSON line reports images/s, mIoU and pixel accuracy
(`pyscripts/benchmark/benchmark_by_mIoU.py`), the number of views and the path taken by the per-view tail."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :125


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'predict_knn_multiscale')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :70-89
  num_classes, crop_size, stride, size = cli.geometry(config)
  memory_dir = args.semantic_memory_dir
  if memory_dir is None:
    memory_dir = cli.build_synthetic_bank(embedding_model, config, args, device)
  prototypes, prototype_labels = cli.load_bank(memory_dir, config, device)                    # :94-111
  counts, out, views = None, None, []

  def one(index):
    nonlocal counts, out, views
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, SCALES, True, crop_size)                        # :123-137
    out = inference.predict_knn_multiscale(embedding_model, prediction_model, views, (size, size), crop_size, stride,
                                           prototypes, prototype_labels, num_classes)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    cli.save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), views=len(views), combine_path=out['combine_path'],
             memory_prototypes=int(prototypes.shape[0]), snapshot=path, semantic_memory_dir=memory_dir,
             save_dir=semantic_dir)


if __name__ == '__main__':
  main()
