#!/usr/bin/env python3
"""Generate pseudo labels from class activation maps by a random walk over the pixel affinity and denseCRF refinement,
with the reference's command line and config surface (`pyscripts/inference/pseudo_camrw_crf.py:37-198` of twke18/SPML;
the first pseudo-label step of the image-tag recipe):

  python3 pyscripts/inference/pseudo_camrw_crf.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --cam_dir CAMS --crf_iter_max 10 --crf_pos_xy_std 1 --crf_pos_w 3 --crf_bi_xy_std 67 --crf_bi_rgb_std 3 --crf_bi_w 4

The embedding network alone (:76-91).  Per image: the CAMs of `<cam_dir>/<name>.npy` -- the reference's format, a pickled
dict `{class - 1: [h, w] float}` -- stacked with the background `(1 - max_fg) ** ALPHA` (:106-111,
`inference.cam_with_background`) and reduced to 1/8 (:151-152, `inference.downsampled_cam`); the embeddings of the flip
pair at scale 1, cropped, flipped back and resampled to 1/8 (:115-144); `inference.affinity_random_walk` with WALK_STEPS
= 6 (:145-164); then the uint8 image (:173-178, `denormalized_uint8`) and the walked maps through one fused call
(`inference.random_walk_crf_refine`, DESIGN 8k: up-sampling :167-169, the label before the CRF :170 and the exact
mean-field filter of `spml_amd.models.crf.DenseCRF`).  Label maps are the arg-max of the refined marginals
(:181), written as `semantic_gray/<name>.npy`.

With `--data_list synthetic` and no `--cam_dir` the CAMs come from the synthetic label map (`synthetic_cams`): 0.2 + 0.6 *
(label == c) for every foreground class the image carries.  A stand-in for the CAM files of another model, like
`flip_scale_views` for the loader: not parity-pinned.

This program stays on synthetic images.  The same recipe on image files (`--data_dir D --data_list L --cam_dir CAMS`) is
`pseudo_softmaxrw.py --cam_dir CAMS --crf`, which forms the class maps in one launch (`spml_cam_ingest_f32`)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ALPHA = 6                                                                                     # :28
WALK_STEPS = 6                                                                                # :29


def synthetic_cams(label, num_classes):
  """The stand-in for a CAM file: `{c - 1: 0.2 + 0.6 * (label == c)}` over the foreground classes in `label` `[h,w]`."""
  import torch
  present = torch.unique(label.reshape(-1).long())
  return {int(c) - 1: 0.2 + 0.6 * (label == c).float() for c in present.tolist() if 0 < c < num_classes}


def load_cams(cam_dir, name, device):
  """`<cam_dir>/<name>.npy`, the reference's pickled dict (:106-107), with its maps on the device."""
  import numpy as np
  import torch
  cams = np.load(os.path.join(cam_dir, name + '.npy'), allow_pickle=True).item()
  return {int(k): torch.as_tensor(np.asarray(v, dtype=np.float32)).to(device) for k, v in cams.items()}


def main(argv=None):
  import torch
  import torch.nn.functional as F
  from spml_amd import inference, inference_cli as cli
  from spml_amd.utils.general import metrics
  config, args, device = cli.parse('Generate pseudo labels from CAM by random walk and CRF.', argv,
                                   'random_walk_crf_refine')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  embedding_model, _, path = cli.load_models(config, args, device, None)                      # :76-91
  num_classes, crop_size, _, size = cli.geometry(config)
  crf = cli.CrfStage(config, args)                                                            # :67-73
  out_hw = (size // 8, size // 8)
  counts, counts_before = None, None
  changed = torch.zeros((), dtype=torch.int64, device=device)

  def one(index):
    nonlocal counts, counts_before
    image, label, _ = cli.synthetic_image(index, size, num_classes, device)
    if args.cam_dir:
      cams = load_cams(args.cam_dir, 'synthetic_{:04d}'.format(index), device)                # :106-107
    else:
      cams = synthetic_cams(label, num_classes)
    cam_full = inference.cam_with_background(cams, (size, size), num_classes, ALPHA).to(device)   # :108-112
    embs_list = []
    with torch.no_grad():
      for view, (rh, rw), flip in inference.flip_scale_views(image, [1], True, crop_size):    # :115-137
        view = view.contiguous(memory_format=torch.channels_last)
        embs = embedding_model.generate_embeddings({'image': view}, resize_as_input=True)['embedding'].float()
        embs = embs[:, :, :rh, :rw]                                                           # :140-144
        if flip:
          embs = torch.flip(embs, dims=[3])
        embs_list.append(F.interpolate(embs, size=out_hw, mode='bilinear'))
      cam_rw = inference.affinity_random_walk(embs_list, inference.downsampled_cam(cam_full), WALK_STEPS)   # :145-164
    # (the stage stands in for its DenseCRF: its events enclose the fused call alone)
    out = inference.random_walk_crf_refine(crf.image_u8(image, (size, size)), cam_rw.contiguous(), crf)   # :166-181
    counts = metrics.iou_stats(out['semantic_prediction'], label, num_classes, counts)
    counts_before = metrics.iou_stats(out['semantic_prediction_before_crf'], label, num_classes, counts_before)
    changed.add_((out['semantic_prediction'] != out['semantic_prediction_before_crf']).sum())
    cli.save_label_map(semantic_dir, index, out['semantic_prediction'])

  done, seconds = cli.timed_images(one)
  cli.report(done, seconds, **cli.scores(counts), mIoU_before_crf=cli.scores(counts_before)['mIoU'],
             changed_by_crf=round(int(changed) / float(max(done, 1) * size * size), 4), alpha=ALPHA,
             walk_steps=WALK_STEPS, cam_dir=args.cam_dir, **crf.fields(seconds), snapshot=path, save_dir=semantic_dir)


if __name__ == '__main__':
  main()
