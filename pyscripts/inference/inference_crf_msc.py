#!/usr/bin/env python3
"""Multi-scale + flip inference for semantic segmentation by nearest-neighbour retrieval with denseCRF refinement, with
the reference's command line and config surface (`pyscripts/inference/inference_crf_msc.py:35-283` of twke18/SPML):

  python3 pyscripts/inference/inference_crf_msc.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048 \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the mean of the views' vote maps is `inference_msc.py` (`spml_amd.inference.predict_knn_multiscale`,
whose `semantic_prob` is the view mean of :246-248).  That map goes with the uint8 image rebuilt from the network's input
(:251-256, `denormalized_uint8`) through `spml_amd.inference.dense_crf_refine`: the exact mean-field filter as HIP
kernels (`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:260); the
JSON line carries what `inference_msc.py` reports plus `crf_path` and `crf_share`, the CRF's share of the image time."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCALES = [0.5, 0.75, 1, 1.25, 1.5]                                                           # :135


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'predict_knn_multiscale')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :71-90
  num_classes, crop_size, stride, size = cli.geometry(config)
  crf = cli.CrfStage(config, args)                                                            # :93-100
  memory_dir = args.semantic_memory_dir
  if memory_dir is None:
    memory_dir = cli.build_synthetic_bank(embedding_model, config, args, device)
  prototypes, prototype_labels = cli.load_bank(memory_dir, config, device)                    # :103-120
  counts, out, views = None, None, []

  def one(index):
    nonlocal counts, out, views
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    views = inference.flip_scale_views(image, SCALES, True, crop_size)                        # :133-153
    out = inference.predict_knn_multiscale(embedding_model, prediction_model, views, (size, size), crop_size, stride,
                                           prototypes, prototype_labels, num_classes)          # :144-248
    refined = crf(crf.image_u8(image, (size, size)), out['semantic_prob'])                    # :251-260
    counts = metrics.iou_stats(refined['semantic_prediction'], label, num_classes, counts)
    cli.save_label_map(semantic_dir, index, refined['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), views=len(views), combine_path=out['combine_path'],
             **crf.fields(seconds), memory_prototypes=int(prototypes.shape[0]), snapshot=path,
             semantic_memory_dir=memory_dir, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
