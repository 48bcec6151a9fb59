"""`spml_score_batch_u8` (csrc/score_batch.hip), `metrics.DirectoryScorer` and the two benchmark programs on the GPU:
against the fixture exec'd from the reference's programs (tests/golden/n15_score_dirs.npz) and, on the shapes the fixture
does not hold, against the numpy restatement tests/score_ref.py (which tests/test_score_dirs.py holds to the fixture)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import score_ref
from conftest import load_golden
from spml_amd import _ffi
from spml_amd.utils.general import metrics
from test_score_dirs import CASES, LDS_ENTRIES, fixture_files, program, table_entries, write_png

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# csrc/score_batch.hip
VEC = 16                               # kVec: pixels of one 16-byte load
RUN = 256 * VEC * 2                    # kRun = kBlock * kVec * kVecsPerThread: pixels of one workgroup
GLOBAL_NCLS = 28                       # the first class count whose tables leave LDS
SENTINEL = -7777777


def run(files, ncls, garbage=None, out=None, one_by_one=False):
  """stats `[B, 4, ncls]` (numpy) of a list of (pred, gt, inst or None)."""
  if one_by_one:
    return np.concatenate([run([f], ncls, garbage) for f in files])
  packed, records = score_ref.pack(files, garbage)
  stats = _ffi.score_batch(torch.from_numpy(packed).to(DEV), records, ncls, out=out)
  assert stats.dtype == torch.int64 and tuple(stats.shape) == (len(files), 4, ncls) and stats.is_cuda
  return stats.cpu().numpy()


def random_file(rng, n, ncls, with_inst=True, ids=(0, 1, 7, 200, 255), coherent=False):
  """uint8 planes of n pixels with every kind of value: classes, the class count, values above it, 255."""
  gt_values = np.array(list(range(ncls)) * 3 + [ncls, min(ncls + 2, 254), 255, 255])
  pred_values = np.array(list(range(ncls)) * 3 + [ncls, ncls + 1, 255])
  if coherent:                                               # runs of equal values: the wave merges equal keys
    runs = lambda values: np.repeat(rng.choice(values, size=n // 37 + 1), 37)[:n].astype(np.uint8)
    gt, pred = runs(gt_values), runs(pred_values)
    pred = np.where(rng.random(n) < 0.5, np.minimum(gt, ncls - 1), pred).astype(np.uint8)
    inst = np.repeat(rng.choice(np.array(ids), size=n // 101 + 1), 101)[:n].astype(np.uint8)
  else:
    gt, pred = rng.choice(gt_values, size=n).astype(np.uint8), rng.choice(pred_values, size=n).astype(np.uint8)
    inst = rng.choice(np.array(ids), size=n).astype(np.uint8)
  return pred, gt, (inst if with_inst else None)


@pytest.mark.parametrize('nc', sorted(CASES))
def test_fixture_rows_exactly_as_one_batch_and_file_by_file(nc):
  g = load_golden('n15_score_dirs')
  files = fixture_files(g, nc)
  want = np.stack([rows for _, _, _, rows in files])
  triples = [(p, t, s) for p, t, s, _ in files]
  assert _ffi.score_batch_path_name(score_ref.pack(triples)[1], score_ref.pack(triples)[0].size, nc) == 'lds_table'
  for one_by_one in (False, True):
    got = run(triples, nc, one_by_one=one_by_one)
    assert np.array_equal(got, want), (nc, one_by_one, np.argwhere(got != want)[:5])
  iou, mean, acc = score_ref.miou_result(got)
  assert np.abs(iou - g['n%d_iou' % nc].numpy()).max() <= 1e-12 and abs(mean - float(g['n%d_mean_iou' % nc])) <= 1e-12


# n: the vector width and its tail; one under, at and over a workgroup's run
@pytest.mark.parametrize('n', [1, VEC - 1, VEC, VEC + 1, 2 * VEC + 1, RUN - 1, RUN, RUN + 1])
@pytest.mark.parametrize('nc', [21, GLOBAL_NCLS])
def test_sizes_around_the_vector_and_the_run(n, nc):
  rng = np.random.default_rng(1000 * nc + n)
  files = [random_file(rng, n, nc), random_file(rng, n, nc, with_inst=False, coherent=True)]
  assert np.array_equal(run(files, nc), score_ref.batch_stats(files, nc))


@pytest.mark.parametrize('nc', [1, 15, 27, GLOBAL_NCLS, 64])
def test_workgroup_prefix_mixed_batches_and_both_tables(nc):
  """A file spanning three runs next to a 1-pixel file (the prefix over the records' run counts); batches of 1, 2 and 5
  files with and without instance planes in one call; the last class count in LDS, the first on the global table, 64."""
  rng = np.random.default_rng(77 + nc)
  assert (table_entries(nc) <= LDS_ENTRIES) == (nc < GLOBAL_NCLS)
  five = [random_file(rng, 2 * RUN + 5, nc, coherent=True), random_file(rng, 1, nc),
          random_file(rng, RUN + 3, nc, with_inst=False), random_file(rng, 3 * 256 + 7, nc),
          random_file(rng, 2 * RUN, nc, with_inst=False, coherent=True)]
  five[3] = five[3][:2] + (rng.permutation(np.arange(3 * 256 + 7) % 256).astype(np.uint8),)       # all 256 ids
  assert np.unique(five[3][2]).size == 256
  want = score_ref.batch_stats(five, nc)
  for batch in ([0], [1], [0, 1], [1, 0], [2, 3], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
    files = [five[i] for i in batch]
    packed, records = score_ref.pack(files)
    assert _ffi.score_batch_path_name(records, packed.size, nc) == ('lds_table' if nc < GLOBAL_NCLS else 'global_table')
    got = run(files, nc)
    # batch independence: a file's rows are the same in every position and company
    assert np.array_equal(got, want[batch]), (nc, batch)


def test_two_calls_give_identical_bits_in_either_mode():
  rng = np.random.default_rng(5)
  for nc in (21, GLOBAL_NCLS):
    files = [random_file(rng, RUN + 100, nc), random_file(rng, 700, nc, coherent=True)]
    first = run(files, nc)
    was = _ffi.set_deterministic(True)
    try:
      assert np.array_equal(run(files, nc), first)
    finally:
      _ffi.set_deterministic(was)
    assert np.array_equal(run(files, nc), first) and np.array_equal(first, score_ref.batch_stats(files, nc))


@pytest.mark.parametrize('nc', [15, 21])
def test_agrees_with_the_per_image_route_on_in_range_predictions(nc):
  rng = np.random.default_rng(9 + nc)
  files = []
  for n in (40 * 52, RUN + 17):
    pred, gt, inst = random_file(rng, n, nc, coherent=True)
    files.append((np.minimum(pred, nc - 1), gt, inst))
  got = run(files, nc)
  for (pred, gt, inst), rows in zip(files, got):
    pred, gt, inst = (torch.from_numpy(a).to(DEV) for a in (pred, gt, inst))
    assert np.array_equal(metrics.iou_stats(pred, gt, nc).cpu().numpy(), rows[:3])
    assert np.array_equal(metrics.instance_class_counts(inst, gt, nc).cpu().numpy(), rows[3])


def test_padding_content_and_sentinel():
  """Garbage in the plane padding changes nothing; an output pre-filled with a sentinel is fully overwritten."""
  rng = np.random.default_rng(11)
  nc = 21
  files = [random_file(rng, n, nc, with_inst=i != 1) for i, n in enumerate((1, 17, RUN + 1, 33))]
  want = score_ref.batch_stats(files, nc)
  assert np.array_equal(run(files, nc, garbage=np.random.default_rng(12)), want)
  out = torch.full((len(files), 4, nc), SENTINEL, dtype=torch.int64, device=DEV)
  got = run(files, nc, garbage=np.random.default_rng(13), out=out)
  assert np.array_equal(got, want) and np.array_equal(out.cpu().numpy(), want) and not want[1, 3].any()


def test_limits_raise_with_their_status_and_leave_stats_untouched():
  nc = 21
  rng = np.random.default_rng(21)
  files = [random_file(rng, 100, nc), random_file(rng, 40, nc, with_inst=False)]
  packed_np, records = score_ref.pack(files)
  packed = torch.from_numpy(packed_np).to(DEV)

  def status(records, ncls=nc, packed=packed, out=None, shape=None):
    shape = (len(records), 4, max(ncls, 1)) if shape is None else shape
    out = torch.full(shape, SENTINEL, dtype=torch.int64, device=DEV) if out is None else out
    with pytest.raises(_ffi.SpmlHipError) as e:
      _ffi.score_batch(packed, records, ncls, out=out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    return str(e.value)

  def changed(**fields):
    rec = records.copy()
    for k, v in fields.items():
      rec[0][k] = v
    return rec

  unsupported, invalid = 'status -2', 'status -1'
  assert unsupported in status(records, ncls=65, shape=(2, 4, 65))
  many = np.zeros(257, dtype=_ffi.SCORE_PARAMS)
  many['n'], many['inst_off'] = 1, -1
  many['pred_off'], many['gt_off'] = np.arange(257) * 32, np.arange(257) * 32 + 16
  big = torch.zeros(257 * 32, dtype=torch.uint8, device=DEV)
  assert unsupported in status(many, packed=big)
  assert _ffi.score_batch(big, many[:256], nc).shape[0] == 256               # ... 256 files are taken
  for bad in (changed(n=0), changed(n=1 << 31), changed(pred_off=8), changed(inst_off=records[0]['gt_off']),
              changed(gt_off=packed_np.size - 96), changed(inst_off=-2), changed(gt_off=records[1]['gt_off'])):
    assert unsupported in status(bad)
  assert invalid in status(records, packed=torch.cat([packed[:1], packed])[1:])          # a misaligned pointer
  buf = torch.full((packed_np.size // 8 + 2 * 4 * nc,), SENTINEL, dtype=torch.int64, device=DEV)
  assert invalid in status(records, packed=buf.view(torch.uint8)[:packed_np.size], out=buf[:2 * 4 * nc].view(2, 4, nc))
  # the workspace, which the wrapper sizes itself: the entry called directly
  lib, host = _ffi.lib(), ctypes.c_void_p(records.ctypes.data)
  rec_dev = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).to(DEV)
  out = torch.full((2, 4, nc), SENTINEL, dtype=torch.int64, device=DEV)
  need = lib.spml_score_batch_workspace_bytes(2, nc)
  ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
  call = lambda ws_ptr, ws_bytes, stats=out: lib.spml_score_batch_u8(
      _ffi.ptr(packed), packed.numel(), host, _ffi.ptr(rec_dev), 2, nc, _ffi.ptr(stats), ws_ptr, ws_bytes, _ffi.stream_ptr())
  assert call(ctypes.c_void_p(0), need) == -3 and call(_ffi.ptr(ws), need - 1) == -3
  assert call(_ffi.ptr(ws), need, stats=ws[:2 * 4 * nc * 8].view(torch.int64).view(2, 4, nc)) == -1      # stats inside ws
  torch.cuda.synchronize()
  assert (out == SENTINEL).all()
  assert call(_ffi.ptr(ws), need) == 0
  assert np.array_equal(out.cpu().numpy(), score_ref.batch_stats(files, nc))


def test_directory_scorer_batches_and_bytes():
  """Files as in-memory PNG bytes through the scorer: batches capped by count and by bytes give the same sums; three
  bytes per pixel (plus padding and the records) go up, `[B, 4, ncls]` int64 comes back."""
  import io
  from PIL import Image
  nc = 21
  g = load_golden('n15_score_dirs')
  files = fixture_files(g, nc)

  def png(a):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format='PNG')
    return f.getvalue()

  triples = [(png(p), png(t), png(s)) for p, t, s, _ in files]
  results = []
  for args in (dict(), dict(batch_files=2), dict(batch_bytes=1), dict(batch_files=1, decode_threads=1)):
    scorer = metrics.DirectoryScorer(nc, **args)
    r = scorer.score(triples).result()
    results.append(r)
    assert r['files'] == len(files) and r['score_path'] == 'lds_table'
    assert np.abs(r['iou'] - g['n%d_iou' % nc].numpy()).max() <= 1e-12
    assert abs(r['pixel_acc'] - float(g['n%d_pixel_acc' % nc])) <= 1e-12
    assert np.abs(r['inst_iou'] - g['n%d_inst_iou' % nc].numpy()).max() <= 1e-12
    assert abs(r['inst_mean_iou'] - float(g['n%d_inst_mean_iou' % nc])) <= 1e-12
    planes = sum((p.size + 15) // 16 * 16 * 3 for p, _, _, _ in files)
    assert r['upload_bytes'] == planes + 32 * len(files) and r['download_bytes'] == len(files) * 4 * nc * 8
  assert [r['batches'] for r in results] == [1, 3, 5, 5]
  no_inst = metrics.DirectoryScorer(nc).score([(p, t, None) for p, t, _ in triples]).result()
  assert np.array_equal(no_inst['iou'], results[0]['iou']) and not no_inst['ninst'].any() and not no_inst['inst_iou'].any()


@pytest.mark.parametrize('nc', sorted(CASES))
def test_programs_end_to_end(nc, tmp_path, capsys):
  from spml_amd import benchmark_cli as cli
  g = load_golden('n15_score_dirs')
  files = fixture_files(g, nc)
  pred_dir, gt_dir, inst_dir = (str(tmp_path / d) for d in ('out' + os.sep + 'semantic_gray', 'segcls', 'inst'))
  for fi, (pred, gt, inst, _) in enumerate(files):
    rel = os.path.join('sub', 'deeper', 'f1') if fi == 1 else 'f%d' % fi     # one file sits in a sub-directory
    write_png(os.path.join(pred_dir, rel + '_pred.png'), pred)
    write_png(os.path.join(gt_dir, rel + '.png'), gt)
    write_png(os.path.join(inst_dir, rel + '.png'), inst, 'P' if fi == 0 else 'L')       # one mask in mode P
  common = ['--pred_dir', pred_dir, '--gt_dir', gt_dir, '--num_classes', str(nc), '--string_replace', '_pred,']
  names = cli.class_names(nc)

  result = program('benchmark_by_mIoU').main(common)
  lines = capsys.readouterr().out.splitlines()
  iou = g['n%d_iou' % nc].numpy()
  want = [pred_dir] + ['class {:10s}: {:02d}, acc: {:4.4f}%'.format(names[i], i, iou[i]) for i in range(nc)]
  want += ['mean IOU: {:4.4f}%'.format(float(g['n%d_mean_iou' % nc])), 'mean Pixel Acc: {:4.4f}%'.format(float(g['n%d_pixel_acc' % nc]))]
  assert lines[:-1] == want
  report = json.loads(lines[-1])
  assert report['files'] == len(files) and report['score_path'] == 'lds_table' and report['seconds'] >= 0
  assert abs(report['mean_iou'] - float(g['n%d_mean_iou' % nc])) <= 1e-12 and report['images_per_s'] > 0
  assert np.abs(result['iou'] - iou).max() <= 1e-12

  result = program('benchmark_by_instance').main(common + ['--inst_dir', inst_dir])
  lines = capsys.readouterr().out.splitlines()
  iou = g['n%d_inst_iou' % nc].numpy()
  want = [pred_dir] + ['class {:10s}: {:02d}, acc: {:4.4f}%'.format(names[i], i, iou[i]) for i in range(nc)]
  want += ['mean IOU: {:4.4f}%'.format(float(g['n%d_inst_mean_iou' % nc]))]
  assert lines[:-1] == want
  report = json.loads(lines[-1])
  assert report['files'] == len(files) and report['score_path'] == 'lds_table'
  assert abs(report['mean_iou'] - float(g['n%d_inst_mean_iou' % nc])) <= 1e-12
  assert np.abs(result['inst_iou'] - iou).max() <= 1e-12
