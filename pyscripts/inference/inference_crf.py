#!/usr/bin/env python3
"""Single-view inference for semantic segmentation by nearest-neighbour retrieval with denseCRF refinement, with the
reference's command line and config surface (`pyscripts/inference/inference_crf.py:35-280` of twke18/SPML):

  python3 pyscripts/inference/inference_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048 \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

Everything up to the clustering is `inference.py` (:145-229).  The retrieval then stays per segment
(`Segsort.segment_predictions`: `[m, 20]` labels and one segment id per pixel), and the vote map of :240-245 goes with the
uint8 image rebuilt from the network's input (:247-252, `denormalized_uint8`) through one fused call
(`spml_amd.inference.predict_knn_full_resolution_crf`): votes, log p and Q_0 are formed once per segment, the
CRF's first kernel gathers them per pixel, writes the label before the CRF and starts the exact mean-field filter
(`spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals (:257), written as
`semantic_gray/<name>.npy`; the JSON line carries what `inference.py` reports, scored on the refined labels, plus
`mIoU_before_crf`, `changed_by_crf` (the share of pixels whose label the CRF changed), `crf_path`, `votes_path` and
`crf_share`, the CRF's share of the image time.  The reference's resize to `test.image_size` and the nearest-neighbour
resize of the label map back (:133-142, :258-261) are file plumbing and not built: synthetic images are made at the
network's size."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  import torch
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, 'predict_knn_full_resolution_crf')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :71-90
  num_classes, crop_size, stride, size = cli.geometry(config)
  crf = cli.CrfStage(config, args)                                                            # :92-99
  memory_dir = args.semantic_memory_dir
  if memory_dir is None:
    memory_dir = cli.build_synthetic_bank(embedding_model, config, args, device)
  prototypes, prototype_labels = cli.load_bank(memory_dir, config, device)                    # :102-120
  counts, counts_before, out = None, None, None
  changed = torch.zeros((), dtype=torch.int64, device=device)

  def one(index):
    nonlocal counts, counts_before, out
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]                   # :145-152
    out = inference.predict_knn_full_resolution_crf(embedding_model, prediction_model, padded, (size, size), crop_size,
                                                    stride, prototypes, prototype_labels, num_classes,
                                                    crf.image_u8(padded, (size, size)), crf,
                                                    config.dataset.semantic_ignore_index)     # :154-257
    refined, before = out['semantic_prediction'], out['semantic_prediction_before_crf']
    counts = metrics.iou_stats(refined, label, num_classes, counts)
    counts_before = metrics.iou_stats(before, label, num_classes, counts_before)
    changed.add_((refined != before).sum())
    cli.save_label_map(semantic_dir, index, refined)

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), mIoU_before_crf=cli.scores(counts_before)['mIoU'],
             changed_by_crf=round(int(changed) / float(max(done, 1) * size * size), 4), votes_path=out['votes_path'],
             **crf.fields(seconds), memory_prototypes=int(prototypes.shape[0]), snapshot=path,
             semantic_memory_dir=memory_dir, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
