"""Scoring label directories, the part that needs no GPU: the fixture (tests/golden/n15_score_dirs.npz, exec'd from
pyscripts/benchmark/benchmark_by_mIoU.py:25-53 / :80-90 / :113-116 and benchmark_by_instance.py:27-55 / :88-116 / :139 by
tools/gen_golden.py) against the numpy restatement of tests/score_ref.py; the host-only functions of
`spml_score_batch_u8` (path names, workspace size); the name mapping, the guards and the PIL conversions of the two
programs.  The kernel itself is checked in tests/test_score_dirs_gpu.py."""
import importlib.util
import io
import os

import numpy as np
import pytest

import score_ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {21: 5, 15: 4}                 # classes -> files
KINDS = {21: ('blocky', 'all_ids', 'one_id', 'one_pixel', 'no_counted'), 15: ('blocky', 'all_ids', 'no_counted', 'one_pixel')}

# csrc/score_batch.hip / csrc/segment_count.hpp
LDS_ENTRIES = 8192                     # segcount::kLdsEntries
NUM_IDS = 256


def table_entries(ncls):
  return ncls * (ncls + 2) + NUM_IDS * (ncls + 1)


def fixture_files(g, nc):
  assert g['n%d_files' % nc] == CASES[nc]
  files = []
  for fi in range(CASES[nc]):
    t = 'n%d_f%d_' % (nc, fi)
    pred, gt, inst, rows = (g[t + k].numpy() for k in ('pred', 'gt', 'inst', 'rows'))
    assert pred.dtype == gt.dtype == inst.dtype == np.uint8 and pred.shape == gt.shape == inst.shape and pred.ndim == 2
    assert rows.dtype == np.int64 and rows.shape == (4, nc)
    files.append((pred, gt, inst, rows))
  return files


def program(name):
  path = os.path.join(ROOT, 'pyscripts', 'benchmark', name + '.py')
  spec = importlib.util.spec_from_file_location('score_program_' + name, path)
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


def write_png(path, array, mode='L'):
  from PIL import Image
  os.makedirs(os.path.dirname(path), exist_ok=True)
  im = Image.fromarray(array)                                # uint8 [h, w]: mode L
  if mode == 'P':                                            # (a palette turns the L image into a P image, indices kept)
    im.putpalette([v for i in range(256) for v in ((i * 7) % 256, (i * 13) % 256, (i * 29) % 256)])
  im.save(path)


@pytest.mark.parametrize('nc', sorted(CASES))
def test_restatement_reproduces_the_fixture(nc):
  g = load_golden('n15_score_dirs')
  files = fixture_files(g, nc)
  stats = score_ref.batch_stats([(p, t, s) for p, t, s, _ in files], nc)
  assert stats.dtype == np.int64
  for fi, (_, _, _, rows) in enumerate(files):
    assert np.array_equal(stats[fi], rows), (nc, fi)
  iou, mean, acc = score_ref.miou_result(stats)
  assert np.abs(iou - g['n%d_iou' % nc].numpy()).max() <= 1e-12
  assert abs(mean - float(g['n%d_mean_iou' % nc])) <= 1e-12 and abs(acc - float(g['n%d_pixel_acc' % nc])) <= 1e-12
  iou, mean, _ = score_ref.instance_result(stats)
  assert np.abs(iou - g['n%d_inst_iou' % nc].numpy()).max() <= 1e-12
  assert abs(mean - float(g['n%d_inst_mean_iou' % nc])) <= 1e-12
  # without an instance plane: the same three rows, row 3 zero
  no_inst = score_ref.batch_stats([(p, t, None) for p, t, _, _ in files], nc)
  assert np.array_equal(no_inst[:, :3], stats[:, :3]) and not no_inst[:, 3].any()


@pytest.mark.parametrize('nc', sorted(CASES))
def test_fixture_holds_the_quirks(nc):
  g = load_golden('n15_score_dirs')
  files = dict(zip(KINDS[nc], fixture_files(g, nc)))
  assert len({f[0].shape for f in files.values()}) >= 3                       # files of different sizes in one case
  pred, gt, inst, rows = files['blocky']
  counted = gt < nc
  for value in (nc, nc + 3, 255):                                             # predictions at, above the class count, 255
    assert (pred[counted] == value).any()
  # ... of which only those AT the class count are counted, for the last class
  in_range = np.bincount(pred[counted & (pred < nc)], minlength=nc)
  assert rows[1, nc - 1] == in_range[nc - 1] + (pred[counted] == nc).sum() and (pred[counted] == nc).sum() > 0
  assert np.array_equal(rows[1, :nc - 1], in_range[:nc - 1])
  assert rows[1].sum() == counted.sum() - (pred[counted] > nc).sum() < rows[0].sum() == counted.sum()
  at_last = (gt == nc - 1) & (pred == nc)                                     # ... and are no true positive of it
  assert at_last.any() and rows[2, nc - 1] == ((gt == nc - 1) & (pred == nc - 1)).sum()
  assert ((gt >= nc) & (gt < 255)).any() and (gt == 255).any()                # ground truth in [ncls, 254] and at 255
  ids = np.unique(inst)
  assert {0, 3, 5, 255} <= set(ids.tolist()) and rows[3].sum() == ids.size
  assert (gt[inst == 3] >= nc).all()                                          # an id with only uncounted pixels: class 0
  without3 = score_ref.file_stats(pred[inst != 3], gt[inst != 3], inst[inst != 3], nc)
  assert without3[3, 0] == rows[3, 0] - 1 and np.array_equal(without3[3, 1:], rows[3, 1:])
  five = np.bincount(gt[inst == 5], minlength=256)[:nc]                       # an id tied between two classes: the lower
  a, b = np.flatnonzero(five == five.max())
  only5 = score_ref.file_stats(pred[inst == 5], gt[inst == 5], inst[inst == 5], nc)[3]
  assert a < b and only5[a] == 1 and only5.sum() == 1
  pred, gt, inst, rows = files['all_ids']                                     # all 256 ids: the largest is dropped
  assert np.unique(inst).size == 256 and rows[3].sum() == 255
  pred, gt, inst, rows = files['no_counted']                                  # no counted pixel at all
  assert (gt >= nc).all() and not rows[:3].any() and rows[3].tolist() == [np.unique(inst).size] + [0] * (nc - 1)
  pred, gt, inst, rows = files['one_pixel']                                   # 1 x 1
  assert pred.shape == (1, 1) and rows[0].sum() == 1 and rows[2].sum() == 1 and rows[3].sum() == 1
  if nc == 21:
    pred, gt, inst, rows = files['one_id']                                    # a single id
    assert np.unique(inst).size == 1 and rows[3].sum() == 1 and pred.size % 16 != 0


def records_of(planes, n=100):
  """SCORE_PARAMS records from [(pred_off, gt_off, inst_off)]."""
  from spml_amd import _ffi
  rec = np.zeros(len(planes), dtype=_ffi.SCORE_PARAMS)
  for b, (p, t, s) in enumerate(planes):
    rec[b] = (p, t, s, n)
  return rec


def test_path_name_table():
  from spml_amd import _ffi
  one = records_of([(0, 112, 224)])                                           # 100 pixels: planes padded to 112 bytes
  assert _ffi.SCORE_PARAMS.itemsize == _ffi.lib().spml_score_params_bytes() == 32
  for nc in (1, 15, 21):
    assert table_entries(nc) <= LDS_ENTRIES and _ffi.score_batch_path_name(one, 336, nc) == 'lds_table'
  first_global = next(nc for nc in range(1, 65) if table_entries(nc) > LDS_ENTRIES)
  assert first_global == 28
  assert _ffi.score_batch_path_name(one, 336, first_global - 1) == 'lds_table'
  assert _ffi.score_batch_path_name(one, 336, first_global) == 'global_table'
  assert _ffi.score_batch_path_name(one, 336, 64) == 'global_table'
  assert _ffi.score_batch_path_name(one, 336, 65) == 'unsupported'
  assert _ffi.score_batch_path_name(one, 336, 0) == 'unsupported'
  many = records_of([(i * 224, i * 224 + 112, -1) for i in range(257)])
  assert _ffi.score_batch_path_name(many[:256], 257 * 224, 21) == 'lds_table'
  assert _ffi.score_batch_path_name(many, 257 * 224, 21) == 'unsupported'    # 257 files
  assert _ffi.score_batch_path_name(many[:0], 257 * 224, 21) == 'unsupported'
  assert _ffi.score_batch_path_name(records_of([(0, 112, -1)]), 224, 21) == 'lds_table'       # no instance plane
  for bad in ([(8, 112, 224)], [(0, 120, 224)], [(0, 112, 232)],              # a misaligned offset
              [(0, 96, 224)], [(0, 112, 0)], [(0, 0, -1)],                    # overlapping planes (the padding counts)
              [(0, 112, 240)], [(240, 0, 112)], [(0, 112, -16)], [(-16, 0, 112)],   # a plane that leaves the buffer
              [(0, 112, -2)]):
    assert _ffi.score_batch_path_name(records_of(bad), 336, 21) == 'unsupported', bad
  assert _ffi.score_batch_path_name(records_of([(0, 112, 224)]), 335, 21) == 'unsupported'    # the PADDED plane must fit
  two = records_of([(0, 112, -1), (224, 112, -1)])                            # two files sharing a ground-truth plane
  assert _ffi.score_batch_path_name(two, 336, 21) == 'unsupported'
  for n, ok in ((0, False), (1, True), (-5, False), (1 << 31, False), ((1 << 31) - 1, True)):
    pad = (max(n, 0) + 15) // 16 * 16
    rec = records_of([(0, pad, -1)], n=n)
    assert (_ffi.score_batch_path_name(rec, 2 * pad, 21) == 'lds_table') == ok, n


def test_workspace_size_is_zero_outside_the_limits():
  from spml_amd import _ffi
  lib = _ffi.lib()
  for b, nc in ((1, 21), (64, 21), (256, 64), (5, 15), (1, 1)):
    assert lib.spml_score_batch_workspace_bytes(b, nc) == b * table_entries(nc) * 4
  for b, nc in ((0, 21), (257, 21), (-1, 21), (1, 0), (1, 65), (1, -3)):
    assert lib.spml_score_batch_workspace_bytes(b, nc) == 0


def test_cpu_tensors_are_refused():
  import torch
  from spml_amd import _ffi
  packed, records = score_ref.pack([(np.zeros((3, 5), np.uint8),) * 2 + (None,)])
  with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
    _ffi.score_batch(torch.from_numpy(packed), records, 21)
  if not torch.cuda.is_available():
    from spml_amd.utils.general import metrics
    with pytest.raises(_ffi.SpmlHipError, match='no CPU fallback'):
      metrics.DirectoryScorer(21)


def test_name_mapping_and_string_replace(tmp_path):
  from spml_amd.utils.general import metrics
  pred_dir, gt_dir, inst_dir = (str(tmp_path / d) for d in ('run' + os.sep + 'semantic_gray', 'segcls', 'inst'))
  plane = np.zeros((2, 3), np.uint8)
  for rel in ('a_pred.png', os.path.join('2008', 'nested', 'b_pred.png')):
    write_png(os.path.join(pred_dir, rel), plane)
    write_png(os.path.join(gt_dir, rel.replace('_pred', '')), plane)
    write_png(os.path.join(inst_dir, rel.replace('_pred', '')), plane, 'P')
  assert metrics.mapped_name('/p/x/p/y.png', '/p', '/g') == '/g/x/g/y.png'   # str.replace: every occurrence, as there
  assert metrics.mapped_name('/p/y_pred.png', '/p', '/g', '_pred,') == '/g/y.png'
  assert metrics.mapped_name('/p/y.png', '/p', '/g', '.png,.gif') == '/g/y.gif'
  assert metrics.mapped_name('/p/y.png', '/p', '/g', '') == '/g/y.png'
  with pytest.raises(metrics.ScoreInputError, match="'a,b'"):
    metrics.mapped_name('/p/y.png', '/p', '/g', 'a,b,c')
  triples = metrics.directory_triples(pred_dir, gt_dir, inst_dir, '_pred,')
  assert [t[0] for t in triples] == [os.path.join(d, f) for d, _, fs in os.walk(pred_dir) for f in fs] and len(triples) == 2
  for pred, gt, inst in triples:
    rel = os.path.relpath(pred, pred_dir).replace('_pred', '')
    assert gt == os.path.join(gt_dir, rel) and inst == os.path.join(inst_dir, rel)
  assert {os.path.dirname(os.path.relpath(t[0], pred_dir)) for t in triples} == {'', os.path.join('2008', 'nested')}
  assert [t[2] for t in metrics.directory_triples(pred_dir, gt_dir, None, '_pred,')] == [None, None]
  metrics.check_sizes(triples)
  with pytest.raises(metrics.ScoreInputError, match='has no ground truth'):
    metrics.directory_triples(pred_dir, gt_dir, inst_dir)                     # without the replacement nothing matches


@pytest.mark.parametrize('name', ['benchmark_by_mIoU', 'benchmark_by_instance'])
def test_every_guard_names_the_path(name, tmp_path, monkeypatch, capsys):
  import torch
  main = program(name).main
  with_inst = name == 'benchmark_by_instance'
  pred_dir, gt_dir, inst_dir, empty = (str(tmp_path / d) for d in ('pred', 'gt', 'inst', 'empty'))
  os.makedirs(empty)
  plane = np.arange(12, dtype=np.uint8).reshape(3, 4)
  for rel in ('a.png', os.path.join('sub', 'b.png')):
    write_png(os.path.join(pred_dir, rel), plane)
    write_png(os.path.join(gt_dir, rel), plane)
    write_png(os.path.join(inst_dir, rel), plane, 'P')

  def refused(**dirs):
    args = dict(pred_dir=pred_dir, gt_dir=gt_dir, **({'inst_dir': inst_dir} if with_inst else {}))
    args.update(dirs)
    argv = [a for k, v in args.items() for a in ('--' + k, v)]
    with pytest.raises(SystemExit) as e:
      main(argv)
    return str(e.value)

  missing = str(tmp_path / 'nowhere')
  assert refused(pred_dir=missing) == "--pred_dir '%s' is not a directory" % missing
  assert refused(gt_dir=missing) == "--gt_dir '%s' is not a directory" % missing
  a_file = os.path.join(gt_dir, 'a.png')
  assert refused(gt_dir=a_file) == "--gt_dir '%s' is not a directory" % a_file
  if with_inst:
    assert refused(inst_dir=missing) == "--inst_dir '%s' is not a directory" % missing
    assert refused(inst_dir='') =="--inst_dir '' is not a directory"       # the reference's default
  assert refused(pred_dir=empty) == "prediction directory '%s' holds no file" % empty
  assert refused(num_classes='65') == '--num_classes 65 is outside [1, 64]'
  assert "--string_replace takes 'a,b'" in refused(string_replace='a,b,c')
  # a prediction without its ground truth / instance mask
  gt_b = os.path.join(gt_dir, 'sub', 'b.png')
  os.rename(gt_b, gt_b + '.away')
  assert refused() == "prediction '%s' has no ground truth '%s'" % (os.path.join(pred_dir, 'sub', 'b.png'), gt_b)
  os.rename(gt_b + '.away', gt_b)
  if with_inst:
    inst_b = os.path.join(inst_dir, 'sub', 'b.png')
    os.rename(inst_b, inst_b + '.away')
    assert refused() == "prediction '%s' has no instance mask '%s'" % (os.path.join(pred_dir, 'sub', 'b.png'), inst_b)
    os.rename(inst_b + '.away', inst_b)
  # files of one triple that differ in size
  write_png(gt_b, np.zeros((3, 5), np.uint8))
  assert refused() == "prediction '%s' is 3 x 4 but its ground truth '%s' is 3 x 5" % (os.path.join(pred_dir, 'sub', 'b.png'), gt_b)
  write_png(gt_b, plane)
  if with_inst:
    write_png(inst_b, np.zeros((4, 4), np.uint8), 'P')
    assert refused() == "prediction '%s' is 3 x 4 but its instance mask '%s' is 4 x 4" % (os.path.join(pred_dir, 'sub', 'b.png'), inst_b)
    write_png(inst_b, plane, 'P')
  # a machine without a GPU: after the path guards, the refusal of the other programs
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  assert refused() == name + '.py needs an MI355X (the HIP path has no CPU fallback)'
  assert refused(pred_dir=missing) == "--pred_dir '%s' is not a directory" % missing
  assert capsys.readouterr().out == ''                                        # nothing is printed before a refusal


def test_class_names_and_lines():
  from spml_amd import benchmark_cli as cli
  assert len(cli.class_names(21)) == 21 and len(cli.class_names(15)) == 15
  assert cli.class_names(21)[15] == 'Person' and cli.class_names(15)[14] == 'Head'
  assert cli.class_names(3) == ['0', '1', '2']                                # the stated deviation: no NotImplementedError
  lines = cli.class_lines(np.array([12.5, 0.0, 100.0]))
  assert lines == ['class 0         : 00, acc: 12.5000%', 'class 1         : 01, acc: 0.0000%',
                   'class 2         : 02, acc: 100.0000%', 'mean IOU: 37.5000%']
  assert cli.class_lines(np.arange(21) * 1.0)[20] == 'class TV        : 20, acc: 20.0000%'


def test_pil_round_trip_of_the_modes_the_tests_write(tmp_path):
  """`L` and `P` PNGs come back byte for byte through the conversions the scorer uses (convert('L') for predictions and
  ground truth, convert('P') for instance masks) -- from a path and from the file's bytes."""
  from spml_amd.utils.general import metrics
  rng = np.random.default_rng(15)
  plane = rng.integers(0, 256, size=(7, 13), dtype=np.uint8)
  plane[0, :4] = (0, 21, 254, 255)
  for mode, read_as in (('L', 'L'), ('P', 'P'), ('L', 'P')):
    path = str(tmp_path / ('%s_%s.png' % (mode, read_as)))
    write_png(path, plane, mode)
    assert np.array_equal(metrics.decode_label(path, read_as), plane), (mode, read_as)
    assert np.array_equal(metrics.decode_label(open(path, 'rb').read(), read_as), plane), (mode, read_as)
  one = str(tmp_path / 'one.png')
  write_png(one, plane[:1, :1])
  assert metrics.decode_label(one, 'L').shape == (1, 1)
