#!/usr/bin/env python3
"""Times the picture of a training summary at the recipe's size: embedding 16 x 64 x 130 x 130 (channels-last), labels
513 x 513.  One JSON line:

  moments_ms, project_ms, panels_ms   the three library calls (csrc/train_summary.hip), device events
  eigh_ms                             the 64 x 64 eigenproblem on the host with the copy of the covariance, wall clock
  write_ms                            TrainingSummary.write up to the pinned copy (the PNG is the writer thread's), wall clock
  framework_ms                        the same picture as framework ops on the device, torch.svd of the P x C matrix as the
                                      reference takes it; one run in a child process under --framework-timeout, null if
                                      it does not finish
  host_ms                             the reference's chain on the host (normalise, centre, torch.svd, project, stretch,
                                      colour, nearest resize) as torch on the CPU, one run

  --train-steps K (default 0: skipped) adds the cost inside the training loop, on the benchmarked configuration of
  bench.py (VOC12 scribble recipe, ResNet-101 DeepLab-v2, batch 16, 513 x 513, channels-last): step_ms_plain (K steps
  without a summary), step_ms_with_summary (K steps with tensorboard_step = 1), their difference summary_step_cost_ms
  and share_at_step_100 = cost / 100 / step_ms_plain.  Wall clock around K steps, device synchronised.

Device times are medians over --repeats after --warmup calls."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(n, c, h, w, size, device):
  g = torch.Generator().manual_seed(235)
  emb = torch.randn(n, c, h, w, generator=g)
  yy = torch.linspace(-1, 1, h).view(1, 1, h, 1)
  xx = torch.linspace(-1, 1, w).view(1, 1, 1, w)
  emb = 0.3 * emb + torch.randn(1, c, 1, 1, generator=g) * yy + torch.randn(1, c, 1, 1, generator=g) * xx
  sem = torch.randint(0, 21, (n, size, size), generator=g)
  ins = torch.randint(0, 30, (n, size, size), generator=g)
  return (emb.to(device).contiguous(memory_format=torch.channels_last), sem.to(device), ins.to(device))


def device_ms(fn, warmup, repeats):
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return sorted(times)[len(times) // 2]


def reference_chain(emb, sem, ins, table):
  """The reference's lines with torch ops on the tensors' device: vis.py:62-101, common.py:29-73, vis.py:41-48, :23-29."""
  import torch.nn.functional as F
  n, c, h, w = emb.shape
  rows = emb.permute(0, 2, 3, 1).contiguous()
  norm = rows.norm(dim=-1, keepdim=True)
  rows = rows / torch.where(norm >= 1e-12, norm, torch.full_like(norm, 1e-12))
  flat = rows.view(-1, c)
  _, _, v = torch.svd(flat - flat.mean(0, keepdim=True))
  rgb = torch.mm(flat, v[:, :3]).view(n, -1, 3)
  rgb = rgb - rgb.min(1, keepdim=True)[0]
  rgb = rgb / rgb.max(1, keepdim=True)[0]
  rgb = (rgb * 255).byte().view(n, h, w, 3).permute(0, 3, 1, 2)
  panels = []
  for lab in (sem, ins):
    colour = table[(lab & 255).view(-1)].view(n, lab.shape[1], lab.shape[2], 3).permute(0, 3, 1, 2)
    panels.append(F.interpolate(colour.float(), size=(h, w), mode='nearest').byte())
  return torch.cat(panels + [rgb], dim=3)


def framework_child(args):
  dev = torch.device('cuda', 0)
  from spml_amd.utils.general import vis
  emb, sem, ins = inputs(args.batch, args.dim, args.side, args.side, args.labels, dev)
  table = torch.from_numpy(vis.voc_color_map()).to(dev)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  reference_chain(emb, sem, ins, table)
  torch.cuda.synchronize()
  print(json.dumps({'framework_ms': 1e3 * (time.perf_counter() - t0)}))


def train_steps(steps, warmup, device):
  from spml_amd import synth
  from spml_amd.summary import TrainingSummary
  from spml_amd.train import Trainer, voc12_scribble_config
  from spml_amd.utils.general import vis
  cfg = voc12_scribble_config(batch_size=16, crop=513)
  torch.manual_seed(235)
  trainer = Trainer(cfg, device, softmax_head=True, channels_last=True)
  batches = [synth.make_batch(16, 513, num_classes=21, seed=235 + i, device=device, palette=(1, 3)) for i in range(2)]
  for d, _ in batches:
    d['image'] = d['image'].contiguous(memory_format=torch.channels_last)
  out = {}
  with tempfile.TemporaryDirectory() as tmp:
    summary = TrainingSummary(os.path.join(tmp, 'summary'), vis.voc_color_map(), 16)
    for name, every in (('step_ms_plain', 0), ('step_ms_with_summary', 1), ('step_ms_plain_again', 0)):
      cfg.train.tensorboard_step = every
      for i in range(warmup):
        trainer.step(*batches[i % 2], summary=summary)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for i in range(steps):
        trainer.step(*batches[i % 2], summary=summary)
      torch.cuda.synchronize()
      out[name] = 1e3 * (time.perf_counter() - t0) / steps
    summary.close()
  plain = 0.5 * (out['step_ms_plain'] + out['step_ms_plain_again'])
  out['summary_step_cost_ms'] = out['step_ms_with_summary'] - plain
  out['share_at_step_100'] = out['summary_step_cost_ms'] / 100.0 / plain
  out['train_steps'] = steps
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--dim', type=int, default=64)
  ap.add_argument('--side', type=int, default=130)
  ap.add_argument('--labels', type=int, default=513)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--framework-timeout', type=float, default=120.0)
  ap.add_argument('--train-steps', type=int, default=0, help='also time K training steps without and with a summary')
  ap.add_argument('--framework-child', action='store_true', help=argparse.SUPPRESS)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_train_summary needs an MI355X (no CPU fallback)')
  if args.framework_child:
    return framework_child(args)
  from spml_amd import ops
  from spml_amd.summary import TrainingSummary
  from spml_amd.utils.general import vis
  dev = torch.device('cuda', 0)
  emb, sem, ins = inputs(args.batch, args.dim, args.side, args.side, args.labels, dev)
  table = torch.from_numpy(vis.voc_color_map()).to(dev)
  res = {'shape': [args.batch, args.dim, args.side, args.side], 'labels': args.labels,
         'path': ops.pca_path_name(args.dim, args.dim, 1), 'repeats': args.repeats}
  res['moments_ms'] = device_ms(lambda: ops.pca_moments(emb), args.warmup, args.repeats)
  basis = vis.principal_components(emb, 3)[0]
  res['project_ms'] = device_ms(lambda: ops.pca_project_minmax(emb, basis), args.warmup, args.repeats)
  proj, minmax = ops.pca_project_minmax(emb, basis)
  res['panels_ms'] = device_ms(lambda: ops.summary_panels(sem, ins, proj, minmax, table), args.warmup, args.repeats)
  cov = ops.pca_moments(emb)[1]
  torch.cuda.synchronize()
  times = []
  for _ in range(args.repeats):
    t0 = time.perf_counter()
    vis.leading_components(cov.cpu(), 3)
    times.append(1e3 * (time.perf_counter() - t0))
  res['eigh_ms'] = sorted(times)[len(times) // 2]
  with tempfile.TemporaryDirectory() as tmp:
    summary = TrainingSummary(os.path.join(tmp, 'summary'), vis.voc_color_map(), args.batch)
    times = []
    for it in range(args.warmup + args.repeats):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      summary.write(it, sem, ins, emb, {'loss': 1.0, 'lr': 1e-3})
      torch.cuda.synchronize()
      times.append(1e3 * (time.perf_counter() - t0))
    summary.close()
    res['write_ms'] = sorted(times[args.warmup:])[args.repeats // 2]
  # the framework route on the device: once, in a child of its own, under its own time limit
  try:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--framework-child', '--batch', str(args.batch),
                            '--dim', str(args.dim), '--side', str(args.side), '--labels', str(args.labels)],
                           capture_output=True, text=True, timeout=args.framework_timeout)
    lines = [line for line in child.stdout.splitlines() if line.startswith('{')]
    res['framework_ms'] = json.loads(lines[-1])['framework_ms'] if child.returncode == 0 and lines else None
  except subprocess.TimeoutExpired:
    res['framework_ms'] = None
  # the reference's chain on the host
  emb_c, sem_c, ins_c = emb.cpu().contiguous(), sem.cpu(), ins.cpu()
  t0 = time.perf_counter()
  reference_chain(emb_c, sem_c, ins_c, torch.from_numpy(vis.voc_color_map()))
  res['host_ms'] = 1e3 * (time.perf_counter() - t0)
  if args.train_steps > 0:
    del emb, sem, ins, proj, minmax, cov
    torch.cuda.empty_cache()
    res.update(train_steps(args.train_steps, args.warmup, dev))
  print(json.dumps(res))


if __name__ == '__main__':
  main()
