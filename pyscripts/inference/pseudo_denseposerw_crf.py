#!/usr/bin/env python3
"""Generate pseudo labels for DensePose by tag propagation, a random walk over the pixel affinity and denseCRF
refinement, with the reference's command line and config surface (`pyscripts/inference/pseudo_denseposerw_crf.py:39-240`
of twke18/SPML; the DensePose point recipe runs it between stage 1 and the classifier training):

  python3 pyscripts/inference/pseudo_denseposerw_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --kmeans_num_clusters 6,6 --label_divisor 2048 \\
      --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

One view per image, no head: the embedding at half resolution is clustered with the image's own sparse labels (255 kept
as a class of its own so that no pixel is dropped: :121-123), every pixel takes the label of its nearest labelled segment,
the labels are counted per segment and the map of per-segment shares at 1/8 of the image is the class activation map
(:153-190; `spml_amd.inference.densepose_segment_cam`).  WALK_STEPS = 6 squarings of the transition matrix
(:30, :193-201), then the fused up-sampling + denseCRF call of the other random-walk programs (:203-218).  The
embedding network is the DensePose recipe's (:21; `--backbone_types panoptic_pspnet_101` builds
`spml_amd.models.embeddings.resnet_pspnet_densepose`).  Label maps are the arg-max of the refined marginals with the
ignored pixels of the label map set to 255 (:218-222), written as `semantic_gray/<name>.npy`; the JSON line is scored as
`pseudo_softmaxrw_crf.py` scores (mIoU and pixel accuracy of the refined labels, `mIoU_before_crf`, `changed_by_crf`,
`crf_path`, `crf_share`) and adds `cam_path` (which route formed the class maps) and the mean `num_segments`.  An image
whose half-resolution label map holds no labelled point has no tag to propagate (the reference's maps are NaN there): its
label map is written as 255 everywhere, it enters no score, and the JSON line counts it in `images_without_labels`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WALK_STEPS, BACKGROUND_THRESHOLD = 6, None                                                    # :30-31


def main(argv=None):
  import torch
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Generate pseudo labels by random walk and CRF for DensePose.', argv,
                                   'pseudo_labels_densepose_crf')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, _, path = cli.load_models(config, args, device, None, densepose=True)      # :78-93
  num_classes, crop_size, _, size = cli.geometry(config)
  crf = cli.CrfStage(config, args)                                                            # :69-75
  ignore = config.dataset.semantic_ignore_index
  counts, counts_before, cam_path, segments, unlabelled = None, None, None, [], 0
  changed = torch.zeros((), dtype=torch.int64, device=device)

  def one(index):
    nonlocal counts, counts_before, cam_path, unlabelled
    image, label, instance = cli.synthetic_image(index, size, num_classes, device)
    padded = inference.flip_scale_views(image, [1], False, crop_size)[0][0]                   # :112-119
    try:
      out = inference.pseudo_labels_densepose_crf(embedding_model, padded, (size, size), label, instance,
                                                  inference.label_tags_from_map(label, num_classes),
                                                  crf.image_u8(padded, (size, size)), crf, walk_steps=WALK_STEPS,
                                                  background_threshold=BACKGROUND_THRESHOLD)   # :121-222
    except inference.NoLabelledPrototypeError:
      unlabelled += 1
      cli.save_label_map(semantic_dir, index, torch.full_like(label, ignore))
      return
    refined, before = out['semantic_prediction'], out['semantic_prediction_before_crf']
    counts = metrics.iou_stats(refined, label, num_classes, counts)
    counts_before = metrics.iou_stats(before, label, num_classes, counts_before)
    changed.add_(((refined != before) & (label != ignore)).sum())
    cam_path = out['cam_path']
    segments.append(out['num_segments'])
    cli.save_label_map(semantic_dir, index, refined)

  done, seconds = cli.timed_images(one)
  if counts is None:
    raise SystemExit('none of the %d images carries a labelled point: nothing to propagate' % done)
  cli.report(done, seconds, **cli.scores(counts), mIoU_before_crf=cli.scores(counts_before)['mIoU'],
             changed_by_crf=round(int(changed) / float(max(len(segments), 1) * size * size), 4), walk_steps=WALK_STEPS,
             num_segments=round(sum(segments) / float(max(len(segments), 1)), 1), images_without_labels=unlabelled,
             cam_path=cam_path, **crf.fields(seconds), snapshot=path, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
