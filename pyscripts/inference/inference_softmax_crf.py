#!/usr/bin/env python3
"""Inference for semantic segmentation by the softmax classifier with denseCRF refinement, with the reference's command
line and config surface (`pyscripts/inference/inference_softmax_crf.py:27-176` of twke18/SPML), the last step of the box
recipe:

  python3 pyscripts/inference/inference_softmax_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the summed logits is `inference_softmax.py` (`spml_amd.inference.predict_softmax_full_resolution`).
Then the soft-max over the classes cropped to the image (:153-154), the uint8 image rebuilt from the network's input
(:158-164, `denormalized_uint8`) and `spml_amd.inference.dense_crf_refine`: the exact mean-field filter as HIP kernels
(`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:169); the JSON line
carries what `inference_softmax.py` reports plus `crf_path` and `crf_share`, the CRF's share of the image time."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  import torch
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'dense_crf_refine')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'softmax_classifier')   # :63-78
  num_classes, crop_size, stride, size = cli.geometry(config)
  crf = cli.CrfStage(config, args)                                                            # :81-87
  counts, out = None, None

  def one(index):
    nonlocal counts, out
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]                   # resize_with_pad, :100-106
    out = inference.predict_softmax_full_resolution(embedding_model, prediction_model, padded, (size, size), crop_size,
                                                    stride)
    prob = torch.softmax(out['semantic_logit'], dim=1)[0, :, :size, :size].contiguous()      # :153-154
    refined = crf(crf.image_u8(padded, (size, size)), prob)                                   # :158-166
    counts = metrics.iou_stats(refined['semantic_prediction'], label, num_classes, counts)
    cli.save_label_map(semantic_dir, index, refined['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), head_path=out['head_path'], **crf.fields(seconds), snapshot=path,
             save_dir=semantic_dir)


if __name__ == '__main__':
  main()
