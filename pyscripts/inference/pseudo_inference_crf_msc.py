#!/usr/bin/env python3
"""Pseudo-label generation by nearest-neighbour retrieval for the image-tag recipe with denseCRF refinement, with the
reference's command line and config surface (`pyscripts/inference/pseudo_inference_crf_msc.py:38-289` of twke18/SPML):

  python3 pyscripts/inference/pseudo_inference_crf_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT \\
      --data_list L --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048 \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the tag-normalised vote map is `pseudo_inference_msc.py`
(`spml_amd.inference.pseudo_labels_knn_multiscale` with `return_prob=True`: :143-263).  That map -- per class divided by
its maximum over the image, not a distribution, zeros included -- goes with the uint8 image rebuilt from the network's
input (:266-271, `denormalized_uint8`) through `spml_amd.inference.dense_crf_refine`: the exact mean-field filter as HIP
kernels (`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:275); the
JSON line carries what `pseudo_inference_msc.py` reports plus `crf_path` and `crf_share`, the CRF's share of the image
time."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 1, 1.5, 2]                                                                    # :135
FLOOR = 0.15                                                                                 # :260


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'dense_crf_refine')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :73-88
  num_classes, crop_size, stride, size = cli.geometry(config)
  crf = cli.CrfStage(config, args)                                                            # :91-97
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
                                                 stride, prototypes, prototype_labels, num_classes, tags, floor=FLOOR,
                                                 return_prob=True)
    refined = crf(crf.image_u8(image, (size, size)), out['semantic_prob'])                    # :266-273
    counts = metrics.iou_stats(refined['semantic_prediction'], label, num_classes, counts)
    by_instance.update(refined['semantic_prediction'], label, instance.clamp(0, 255))
    cli.save_label_map(semantic_dir, index, refined['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), instance_mIoU=round(by_instance.result()['mean_iou'], 4),
             views=len(views), combine_path=out['combine_path'], normalize_path=out['normalize_path'],
             **crf.fields(seconds), memory_prototypes=int(prototypes.shape[0]), snapshot=path,
             semantic_memory_dir=memory_dir, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
