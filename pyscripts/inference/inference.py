#!/usr/bin/env python3
"""Single-view inference for semantic segmentation by nearest-neighbour retrieval, with the reference's command line and
config surface (`pyscripts/inference/inference.py:35-255` of twke18/SPML):

  python3 pyscripts/inference/inference.py --snapshot_dir S --cfg_path C.yaml --save_dir OUT --data_list L \\
      --semantic_memory_dir BANK --kmeans_num_clusters 12,12 --label_divisor 2048

Loads `model-{max_iteration-1}.pth` from the snapshot directory and the prototype memory bank from
`--semantic_memory_dir` (the ignore class dropped: :99-111).  Every image is zero-padded to the crop size and goes through
`spml_amd.inference.predict_full_resolution` (:136-237: sliding-window embedding, k-means over the whole image with the
padding ignored, top-20 retrieval per segment, majority vote, scatter to the pixels).  `--data_dir D --data_list L`
reads the reference's file list (`ListDataset`): the view of every file is made on the GPU from its decoded bytes
(`spml_amd.inference.device_views`: normalised, resized to `test.image_size`, padded, :124-142), the label map goes back
to the file's own size (:238-241) as `semantic_gray/<name>.png` and `semantic_color/<name>.png`
(`spml_amd.inference.export_label_map`), and `--semantic_memory_dir` is required.  `--data_list synthetic` feeds seeded
synthetic images of `test.image_size` (made at the network's size) and writes `semantic_gray/<name>.npy` (uint8); without
`--semantic_memory_dir` it builds the bank itself, as `inference_msc.py` does.  One JSON line
reports images/s, mIoU and pixel accuracy (`pyscripts/benchmark/benchmark_by_mIoU.py`)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
  from spml_amd import inference, inference_cli as cli
  api = 'predict_full_resolution'
  config, args, device = cli.parse('Inference for semantic segmentation.', argv, api, file_lists='images')
  semantic_dir = cli.output_dir(args, 'semantic_gray')
  source = cli.ImageSource.for_program(config, args, device, [1], False, api, single_view=True)   # :124-142
  embedding_model, prediction_model, path = cli.load_models(config, args, device, 'segsort')   # :70-90
  _, crop_size, stride, _ = cli.geometry(config)
  memory_dir = cli.memory_bank_dir(embedding_model, config, args, device)
  prototypes, prototype_labels = cli.load_bank(memory_dir, config, device)                    # :93-111

  def one(image):
    padded, valid_hw, _ = image.views[0]
    out = inference.predict_full_resolution(embedding_model, prediction_model, padded, valid_hw, crop_size, stride,
                                            prototypes, prototype_labels, config.dataset.semantic_ignore_index)
    source.emit(image, out['semantic_prediction'], semantic_dir)

  done, seconds = source.timed(one)
  cli.report(done, seconds, **source.scores(), memory_prototypes=int(prototypes.shape[0]), snapshot=path,
             semantic_memory_dir=memory_dir, save_dir=semantic_dir, **source.fields())


if __name__ == '__main__':
  main()
