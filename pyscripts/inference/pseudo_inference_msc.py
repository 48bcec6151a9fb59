#!/usr/bin/env python3
"""Pseudo-label generation by nearest-neighbour retrieval for the image-tag recipe, with the reference's command line and
config surface (`pyscripts/inference/pseudo_inference_crf_msc.py:38-289` of twke18/SPML) without its `--crf_*` options:
the stage ends at the arg-max of what the denseCRF (:265-273) would have been fed; `pseudo_inference_crf_msc.py` adds it.

  python3 pyscripts/inference/pseudo_inference_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory and the prototype memory bank from
`--semantic_memory_dir` (what `prototype_msc.py` writes; the ignore class dropped: :101-121).  Every image becomes the
eight views of `spml_amd.inference.flip_scale_views` (scales 0.5, 1, 1.5, 2, each flipped and plain, zero-padded to the
crop size: :133-153) and goes through `spml_amd.inference.pseudo_labels_knn_multiscale`: per view the work of
`inference_msc.py`, then one HIP launch pair that takes the mean over the views, normalises every class the image
carries by its maximum over the image (floored at 0.15) and takes the arg-max (:252-263, :275).  The image's tags are
the classes of its label map (:138-141).  As in the other inference programs the file-list loader is outside this repository:
`--data_list synthetic` feeds seeded synthetic images of `test.image_size`, and without `--semantic_memory_dir` the bank
is built from those images first, written with `save_image_memory` to `<save_dir>/semantic_prototype` and read back.
Label maps are written as `semantic_gray/<name>.npy` (uint8); one JSON line reports images/s, mIoU and pixel accuracy
(`pyscripts/benchmark/benchmark_by_mIoU.py`), the instance-weighted mIoU (`benchmark_by_instance.py`, from the synthetic
instance map), the number of views and the paths taken by the per-view tail and by the normalisation."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 1, 1.5, 2]                                                                    # :135
FLOOR = 0.15                                                                                 # :260


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'pseudo_labels_knn_multiscale')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :73-88
  num_classes, crop_size, stride, size = cli.geometry(config)
  memory_dir = args.semantic_memory_dir
  if memory_dir is None:
    memory_dir = cli.build_synthetic_bank(embedding_model, config, args, device)
  prototypes, prototype_labels = cli.load_bank(memory_dir, config, device)                    # :104-121
  counts, by_instance, out, views = None, metrics.InstanceIoU(num_classes), None, []

  def one(index):
    nonlocal counts, out, views
    image, label, instance = cli.synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, SCALES, True, crop_size)                        # :133-153
    tags = inference.label_tags_from_map(label, num_classes)                                  # :138-141
    out = inference.pseudo_labels_knn_multiscale(embedding_model, prediction_model, views, (size, size), crop_size,
                                                 stride, prototypes, prototype_labels, num_classes, tags, floor=FLOOR)
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    by_instance.update(out['semantic_prediction'], label, instance.clamp(0, 255))
    cli.save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), instance_mIoU=round(by_instance.result()['mean_iou'], 4),
             views=len(views), combine_path=out['combine_path'], normalize_path=out['normalize_path'],
             memory_prototypes=int(prototypes.shape[0]), snapshot=path, semantic_memory_dir=memory_dir,
             save_dir=semantic_dir)


if __name__ == '__main__':
  main()
