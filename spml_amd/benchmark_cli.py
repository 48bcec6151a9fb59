"""The shared body of pyscripts/benchmark/benchmark_by_mIoU.py and benchmark_by_instance.py: the reference's command
line, the guards, the scoring (`spml_amd.utils.general.metrics.DirectoryScorer`) and the reference's printed lines."""
import argparse
import json
import time

import torch

from spml_amd.utils.general import metrics

# benchmark_by_mIoU.py:92-103
DENSEPOSE_NAMES = ['Background', 'Torso', 'R. Hand', 'L. Hand', 'L. Foot', 'R. Foot', 'R. Thigh', 'L. Thigh', 'R. Leg',
                   'L. Leg', 'L. Arm', 'R. Arm', 'L. Forearm', 'R. Forearm', 'Head']
VOC_NAMES = ['Background', 'Aero', 'Bike', 'Bird', 'Boat', 'Bottle', 'Bus', 'Car', 'Cat', 'Chair', 'Cow', 'Table', 'Dog',
             'Horse', 'MBike', 'Person', 'Plant', 'Sheep', 'Sofa', 'Train', 'TV']


def class_names(num_classes):
  """The reference's names for 15 (MSCOCO-DensePose) and 21 (VOC12) classes.  For any other count the reference
  computes everything and then raises NotImplementedError (:104-105); here the index stands in for the name."""
  if num_classes == 15:
    return DENSEPOSE_NAMES
  if num_classes == 21:
    return VOC_NAMES
  return ['%d' % i for i in range(num_classes)]


def parse_args(argv, with_instances):
  parser = argparse.ArgumentParser(description='Benchmark segmentation predictions')
  parser.add_argument('--pred_dir', type=str, default='', help='/path/to/prediction.')
  parser.add_argument('--gt_dir', type=str, default='', help='/path/to/ground-truths')
  if with_instances:
    parser.add_argument('--inst_dir', type=str, default='', help='/path/to/instance-mask')
  parser.add_argument('--num_classes', type=int, default=21, help='number of segmentation classes')
  parser.add_argument('--string_replace', type=str, default=',', help='replace the first string with the second one')
  return parser.parse_args(argv)


def class_lines(iou):
  """benchmark_by_mIoU.py:108-114, character for character."""
  names = class_names(len(iou))
  lines = ['class {:10s}: {:02d}, acc: {:4.4f}%'.format(names[i], i, iou[i]) for i in range(len(iou))]
  lines.append('mean IOU: {:4.4f}%'.format(iou.sum() / len(iou)))
  return lines


def run(argv, with_instances):
  args = parse_args(argv, with_instances)
  if not 1 <= args.num_classes <= 64:
    raise SystemExit('--num_classes %d is outside [1, 64]' % args.num_classes)
  inst_dir = args.inst_dir if with_instances else None
  try:
    triples = metrics.directory_triples(args.pred_dir, args.gt_dir, inst_dir, args.string_replace)
    metrics.check_sizes(triples)
  except metrics.ScoreInputError as e:
    raise SystemExit(str(e))
  if not torch.cuda.is_available():
    raise SystemExit('%s needs an MI355X (the HIP path has no CPU fallback)'
                     % ('benchmark_by_instance.py' if with_instances else 'benchmark_by_mIoU.py'))
  print(args.pred_dir)
  start = time.perf_counter()
  try:
    result = metrics.DirectoryScorer(args.num_classes).score(triples).result()
  except metrics.ScoreInputError as e:
    raise SystemExit(str(e))
  seconds = time.perf_counter() - start
  iou = result['inst_iou'] if with_instances else result['iou']
  for line in class_lines(iou):
    print(line)
  if not with_instances:
    print('mean Pixel Acc: {:4.4f}%'.format(result['pixel_acc']))          # :116-117 (a fraction printed with a % sign)
  print(json.dumps({'files': result['files'], 'seconds': round(seconds, 3),
                    'images_per_s': round(result['files'] / max(seconds, 1e-9), 3), 'score_path': result['score_path'],
                    'mean_iou': result['inst_mean_iou'] if with_instances else result['mean_iou']}))
  return result
