"""The dense CRF on image lists, as far as it runs without a GPU: the lossy round trip the guide kernel reproduces, the
`--crf` option of the five programs that have a `*_crf*` sibling, and the host-side refusals of `spml_crf_guide_u8` and
`spml_label_export_scored_u8`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import crf_lists_ref as crf_ref
import inference_io_cases as cases
from spml_amd import _ffi, inference
from test_inference_io import NOT_WIRED, WIRED, common_args, load_program, write_files

CRF_PROGRAMS = ['inference_softmax', 'inference_softmax_msc', 'inference', 'inference_msc', 'pseudo_softmaxrw']


def test_round_trip_lowers_129_of_768_pairs_by_one():
  """inference_softmax_crf_msc.py:159-164 on the normalised float32 byte: not the identity, so a kernel that passes the
  file's bytes through cannot equal it."""
  table = crf_ref.byte_table(cases.MEAN, cases.STD).astype(np.int64)
  diff = table - np.arange(256)[:, None]
  assert set(np.unique(diff)) == {-1, 0}
  assert [int((diff[:, c] == -1).sum()) for c in range(3)] == [66, 53, 10] and int((diff != 0).sum()) == 129
  # the project's own statement of the chain (torch, on the CPU here) gives the same table
  image = torch.from_numpy(np.arange(256, dtype=np.float32)[None, :].repeat(3, 0).reshape(3, 16, 16))
  norm = (image / 255.0 - torch.tensor(cases.MEAN).view(3, 1, 1)) / torch.tensor(cases.STD).view(3, 1, 1)
  got = inference.denormalized_uint8(norm, cases.MEAN, cases.STD).numpy().reshape(256, 3)
  assert np.array_equal(got, table.astype(np.uint8))


def test_crf_option_is_on_the_five_programs_and_no_others(tmp_path):
  assert set(CRF_PROGRAMS) <= {w[0] for w in WIRED}
  for name in [w[0] for w in WIRED] + NOT_WIRED:
    with pytest.raises(SystemExit) as info:
      load_program(name).main(common_args(tmp_path) + ['--crf'])
    if name in CRF_PROGRAMS:
      assert str(info.value.code) == '--save_dir is required', name
    else:
      assert info.value.code == 2, name                                 # argparse: unrecognized arguments: --crf


@pytest.mark.parametrize('name', CRF_PROGRAMS)
def test_guards_keep_their_order_with_crf(name, tmp_path):
  prog, common = load_program(name), common_args(tmp_path) + ['--crf']
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'train.txt'])
  assert str(info.value.code).startswith("data list 'train.txt' does not exist")
  full, _ = write_files(str(tmp_path / 'full'), ['a.png'])
  listed = common + ['--data_dir', str(tmp_path / 'full'), '--data_list', full]
  with pytest.raises(SystemExit) as info:
    prog.main(listed)
  assert str(info.value.code) == '--save_dir is required'
  if not torch.cuda.is_available():
    with pytest.raises(SystemExit) as info:
      prog.main(listed + ['--save_dir', str(tmp_path / 'o')])
    assert 'no CPU fallback' in str(info.value.code) and not os.path.exists(str(tmp_path / 'o'))


def test_guide_and_scored_export_refusals():
  """Decided on the host before any launch: no GPU is needed, and the pointers below are never read."""
  lib = _ffi.lib()
  assert _ffi.crf_guide_path_name((23, 37)) == 'guide_table' and _ffi.crf_guide_path_name((23, 37), (23, 37)) == 'guide_table'
  assert _ffi.crf_guide_path_name((23, 37), (40, 64)) == 'guide_resized'
  assert _ffi.crf_guide_path_name((23, 43), (23, 42)) == 'guide_resized'
  assert _ffi.crf_guide_path_name((16384, 16384), (16384, 16384)) == 'guide_table'
  for src, dst in (((0, 37), (5, 5)), ((23, 16385), (5, 5)), ((23, 37), (0, 5)), ((23, 37), (5, 16385)), ((-1, 37), (5, 5))):
    assert _ffi.crf_guide_path_name(src, dst) == 'unsupported', (src, dst)
  assert lib.spml_export_scores_bytes(21) == 127 * 8 and lib.spml_export_scores_bytes(1) == 7 * 8
  assert lib.spml_export_scores_bytes(256) == 1537 * 8
  assert lib.spml_export_scores_bytes(0) == 0 and lib.spml_export_scores_bytes(257) == 0 and lib.spml_export_scores_bytes(-3) == 0

  arena = (ctypes.c_ubyte * (1 << 16))()
  base = (ctypes.addressof(arena) + 63) // 64 * 64
  P = ctypes.c_void_p
  rgb, mean, std, guide = base, base + 4096, base + 4160, base + 8192
  stats = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

  def guide_call(rgb=rgb, hw=(5, 7), mean=mean, std=std, mean64=stats, std64=stats, new=(5, 7), guide=guide):
    return lib.spml_crf_guide_u8(P(rgb), hw[0], hw[1], P(mean), P(std), mean64, std64, new[0], new[1], P(guide), None)
  for kw in (dict(hw=(0, 7)), dict(hw=(5, 16385)), dict(new=(0, 7)), dict(new=(16385, 7)), dict(new=(5, 0))):
    assert guide_call(**kw) == -2, kw                                   # SPML_ERR_UNSUPPORTED
  for kw in (dict(rgb=None), dict(mean=None), dict(std=None), dict(mean64=None), dict(std64=None), dict(guide=None),
             dict(rgb=rgb + 1), dict(guide=guide + 2), dict(mean=mean + 2), dict(std=std + 1),
             dict(guide=rgb), dict(guide=rgb + 4 * 26), dict(rgb=guide + 4 * 26, guide=guide),      # 3 * 5 * 7 = 105 bytes
             dict(guide=mean - 104), dict(guide=std + 8)):
    assert guide_call(**kw) == -1, kw                                   # SPML_ERR_INVALID_ARG

  refined, before, table, truth = base, base + 4096, base + 8192, base + 9216
  gray, color, scores = base + 16384, base + 20480, base + 32768

  def export_call(refined=refined, before=before, pred=(9, 9), valid=(9, 9), out=(5, 5), table=table, truth=truth,
                  ncls=21, gray=gray, color=color, scores=scores):
    return lib.spml_label_export_scored_u8(P(refined), P(before), pred[0], pred[1], valid[0], valid[1], out[0], out[1],
                                           P(table), P(truth), ncls, P(gray), P(color), P(scores), None)
  for kw in (dict(ncls=0), dict(ncls=257), dict(ncls=-1), dict(pred=(0, 9)), dict(pred=(9, 16385)), dict(valid=(10, 9)),
             dict(valid=(0, 9)), dict(out=(0, 5)), dict(out=(5, 16385))):
    assert export_call(**kw) == -2, kw
  for kw in (dict(refined=None), dict(table=None), dict(gray=None), dict(color=None), dict(scores=None),
             dict(refined=refined + 4), dict(before=before + 4), dict(scores=scores + 4),
             dict(gray=refined + 8), dict(color=before + 640), dict(gray=table + 700), dict(color=truth),
             dict(scores=refined), dict(scores=gray - 1008), dict(gray=color + 74), dict(scores=color + 72)):
    assert export_call(**kw) == -1, kw


def test_no_cpu_path():
  with pytest.raises(_ffi.SpmlHipError):
    inference.crf_guide(torch.zeros((5, 7, 3), dtype=torch.uint8), cases.MEAN, cases.STD)
  with pytest.raises(_ffi.SpmlHipError):
    inference.export_scored_label_map(torch.zeros((5, 7), dtype=torch.int64), None, (5, 7), (5, 7),
                                      torch.zeros((256, 3), dtype=torch.uint8), None, 21)
