"""Multi-scale memory-bank generation, the parts that need no GPU: the library's new exports and the limits its host
functions state, `label_views` against `flip_scale_views`, the fixture (tests/golden/n10_prototype_msc.npz, exec'd from
pyscripts/inference/prototype_msc.py:126-197 / :204-206 by tools/gen_golden.py) against the oracle's tail, and the
refusals of the two programs.  The GPU side is tests/test_prototype_msc_gpu.py."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from conftest import load_golden
from oracle import spml_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [0.5, 1, 1.5]
NEW_SYMBOLS = ('spml_segment_majority_workspace_bytes', 'spml_segment_majority_i64', 'spml_segment_majority_path_name')


def n10_case(g, ci):
  """(cfg dict, image [1,3,h,w], views) of fixture case `ci`; views = list of dicts with `pad_hw`, `crop_hw`, the
  reference's `label` [rh,rw], `embedding` [1,C,rh,rw] (the un-padded region), `cluster_index` [rh * rw], `prototypes`
  [m,C] and `labels` [m], in the order of the scales 0.5, 1, 1.5."""
  t = 'c%d_' % ci
  c, ncls, h, w, ch, cw, sh, sw, ky, kx = [int(v) for v in g[t + 'cfg']]
  cfg = dict(c=c, ncls=ncls, image=(h, w), crop=(ch, cw), stride=(sh, sw), grid=[ky, kx])
  views = []
  for vi, (pad_h, pad_w, rh, rw, m) in enumerate(g[t + 'views'].tolist()):
    clu, lab = g[t + 'cluster_index%d' % vi], g[t + 'label%d' % vi]
    assert clu.dtype == torch.int16 and tuple(clu.shape) == (rh * rw,) and int(clu.max()) + 1 == m
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (rh, rw)
    assert tuple(g[t + 'embedding%d' % vi].shape) == (1, c, rh, rw) and pad_h == max(rh, ch) and pad_w == max(rw, cw)
    views.append(dict(pad_hw=(pad_h, pad_w), crop_hw=(rh, rw), label=lab.long(), embedding=g[t + 'embedding%d' % vi],
                      cluster_index=clu.long(), prototypes=g[t + 'prototypes%d' % vi],
                      labels=g[t + 'prototype_labels%d' % vi].long()))
  return cfg, g[t + 'image'], views


def load_program(name):
  spec = importlib.util.spec_from_file_location('spml_%s_cli' % name,
                                                os.path.join(ROOT, 'pyscripts', 'inference', name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_library_exports_the_majority_entries_and_the_version_stays_8():
  from spml_amd import _build, _ffi
  _build.build(verbose=False)
  handle = ctypes.CDLL(_build.LIB_PATH)
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  for name in NEW_SYMBOLS:
    assert hasattr(handle, name), name
    assert name in _ffi.EXPORTS and re.search(r'\b%s\(' % name, hdr), name
  assert int(re.search(r'#define SPML_ABI_VERSION (\d+)', hdr).group(1)) == 8 == _ffi.ABI_VERSION
  decl = re.search(r'int spml_segment_majority_i64\(([^)]*)\);', hdr)
  args = [' '.join(a.split()) for a in decl.group(1).split(',')]
  assert args == ['const int64_t* clu', 'const int64_t* sem', 'int64_t P', 'int m', 'int ncls', 'int64_t* major',
                  'int64_t* hist', 'void* ws', 'size_t ws_bytes', 'void* stream']
  want = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}
  res, argtypes = _ffi._SIGNATURES['spml_segment_majority_i64']
  assert res is ctypes.c_int and len(argtypes) == len(args)
  for a, ty in zip(args, argtypes):
    assert ty is (ctypes.c_void_p if '*' in a else want[a.split()[0]]), a
  assert 'prototype_msc.py:189-192' in hdr                    # the declaration cites the reference lines


def test_host_functions_state_the_limits_and_the_two_count_paths():
  """Host functions only: 4096 segments x 256 classes are inside, the next value of either is outside; a table of at
  most 8192 counters is counted in LDS, a larger one (144 x 256, the bank pass of a 12 x 12 k-means) in global memory."""
  from spml_amd import _build, _ffi
  _build.build(verbose=False)
  lib = _ffi.lib()
  assert (_ffi.MAX_MAJORITY_SEGMENTS, _ffi.MAX_MAJORITY_CLASSES) == (4096, 256)
  assert lib.spml_segment_majority_workspace_bytes(144, 256) == 144 * 256 * 4
  assert lib.spml_segment_majority_workspace_bytes(4096, 256) == 4096 * 256 * 4
  for m, ncls in ((4097, 21), (144, 257), (0, 21), (144, 0), (-1, 21)):
    assert lib.spml_segment_majority_workspace_bytes(m, ncls) == 0
  name = _ffi.segment_majority_path_name
  assert name(2640, 16, 5) == name(10 ** 6, 32, 256) == name(0, 1, 1) == 'lds_table'
  assert name(7200, 144, 256) == name(20000, 4096, 21) == name(5, 33, 256) == 'global_table'
  assert name(7200, 4097, 21) == name(7200, 144, 257) == name(2 ** 31, 16, 5) == 'unsupported'
  assert name(2 ** 31 - 1, 16, 5) == 'lds_table' and name(-1, 16, 5) == name(5, 0, 5) == 'invalid'
  with pytest.raises(_ffi.SpmlHipError):                      # CPU tensors: no fallback
    _ffi.segment_majority(torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long), 2, 3)
  import spml_amd.utils.segsort.common as sc
  with pytest.raises(_ffi.SpmlHipError):
    sc.segment_majority_labels(torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long), 2, 3)
  with pytest.raises(_ffi.SpmlHipError):                      # ... outside the limits as well
    sc.segment_majority_labels(torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long), 5000, 3)


@pytest.mark.parametrize('hw,crop', [((44, 60), (48, 48)), ((40, 52), (48, 48)), ((65, 65), (65, 65)), ((7, 5), (4, 4))])
def test_label_views_have_the_sizes_of_flip_scale_views(hw, crop):
  from spml_amd import inference
  gen = torch.Generator().manual_seed(hw[0])
  image = torch.randn(1, 3, *hw, generator=gen)
  label = torch.randint(0, 6, hw, generator=gen)
  label[0, :2] = 255
  views = inference.flip_scale_views(image, SCALES, False, crop)
  assert [v[2] for v in views] == [False] * 3
  labels = inference.label_views(label, [v[1] for v in views])
  assert len(labels) == len(views) == 3
  for (padded, (rh, rw), _), lab in zip(views, labels):
    assert tuple(lab.shape) == (rh, rw) and lab.dtype == torch.int64
    assert padded.shape[-2] >= rh and padded.shape[-1] >= rw
    assert set(lab.unique().tolist()) <= set(label.unique().tolist())        # nearest neighbour makes no new value
  assert torch.equal(labels[1], label)                                        # scale 1 is the map itself
  # nearest neighbour: output (y, x) takes input (floor(y * h / rh), floor(x * w / rw))
  rh, rw = views[2][1]
  iy = (torch.arange(rh).float() * (hw[0] / rh)).floor().long().clamp(max=hw[0] - 1)
  ix = (torch.arange(rw).float() * (hw[1] / rw)).floor().long().clamp(max=hw[1] - 1)
  assert torch.equal(labels[2], label[iy][:, ix])
  with pytest.raises(ValueError):
    inference.label_views(label.unsqueeze(0), [(3, 3)])


@pytest.mark.parametrize('ci', [0, 1])
def test_fixture_views_are_the_views_the_host_functions_make(ci):
  """The fixture stores the image once: its views are rebuilt with `flip_scale_views` / `label_views`, which must give the
  stored sizes and label maps."""
  from spml_amd import inference
  g = load_golden('n10_prototype_msc')
  cfg, image, views = n10_case(g, ci)
  made = inference.flip_scale_views(image, SCALES, False, cfg['crop'])
  assert [tuple(v[0].shape[-2:]) for v in made] == [v['pad_hw'] for v in views]
  assert [v[1] for v in made] == [v['crop_hw'] for v in views]
  labels = inference.label_views(views[1]['label'], [v[1] for v in made])
  for lab, v in zip(labels, views):
    assert torch.equal(lab, v['label'])
  if ci == 0:                                                  # one window; 1 x 2 windows; 2 x 3 windows
    assert [v['pad_hw'] for v in views] == [(48, 48), (48, 60), (66, 90)] and cfg['stride'] == (32, 32)
  else:                                                        # the label cells include the ignore value
    assert int(views[1]['label'].max()) == 255
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'n10_prototype_msc.npz')) < 880 * 1024


@pytest.mark.parametrize('ci', [0, 1])
def test_oracle_tail_on_the_stored_segments_reproduces_the_stored_labels(ci):
  """Per view, the tail of `oracle.full_resolution_prototypes` (prototypes and majority labels of a given clustering)
  on the stored `cluster_index`: labels exactly, prototypes to 1e-6; the bank is the views' concatenation in order; no
  segment's top two class counts tie (the reference's GPU tie order is unspecified)."""
  g = load_golden('n10_prototype_msc')
  cfg, _, views = n10_case(g, ci)
  t = 'c%d_' % ci
  for v in views:
    clu, lab = v['cluster_index'], v['label'].reshape(-1)
    _, major = O.find_majority_label_index(lab, clu)
    assert torch.equal(major, v['labels'])
    emb = O.normalize_embedding(v['embedding'].permute(0, 2, 3, 1).contiguous()).reshape(clu.shape[0], -1)
    protos = O.calculate_prototypes_from_labels(emb, clu)
    assert protos.shape == v['prototypes'].shape
    assert (protos - v['prototypes']).abs().max().item() <= 1e-6
    m, width = v['labels'].shape[0], int(lab.max()) + 1
    hist = torch.bincount(clu * width + lab, minlength=m * width).view(m, width)
    top2 = torch.cat([hist, torch.full((m, 1), -1)], 1).topk(2, dim=1).values
    assert (top2[:, 0] > top2[:, 1]).all()
  assert torch.equal(g[t + 'bank'], torch.cat([v['prototypes'] for v in views], 0))
  assert torch.equal(g[t + 'bank_lab'].long(), torch.cat([v['labels'] for v in views], 0))
  ignored = int((g[t + 'bank_lab'] == 255).sum())
  assert (ignored > 0) == (ci == 1) and g[t + 'bank_lab'].unique().numel() >= 3


def test_multiscale_prototypes_argument_errors():
  from spml_amd import _ffi, inference
  conv = torch.nn.Conv2d(3, 16, 5, padding=2)
  with pytest.raises(ValueError):
    inference.multiscale_prototypes(conv, [], [], (8, 8), (5, 5))
  views = inference.flip_scale_views(torch.zeros(1, 3, 8, 8), [1], False, (8, 8))
  label = torch.zeros(8, 8, dtype=torch.long)
  with pytest.raises(ValueError):                             # one label map per view
    inference.multiscale_prototypes(conv, views, [], (8, 8), (5, 5))
  with pytest.raises(ValueError):                             # a label map of another size
    inference.multiscale_prototypes(conv, views, [label[:4]], (8, 8), (5, 5))
  with pytest.raises(_ffi.SpmlHipError):                      # CPU tensors
    inference.multiscale_prototypes(conv, views, [label], (8, 8), (5, 5))


@pytest.mark.parametrize('name,scales', [('prototype', [1]), ('prototype_msc', [0.5, 1, 1.5])])
def test_programs_refuse_a_file_list_and_a_machine_without_a_gpu(name, scales, tmp_path):
  from test_train_cli import YAML
  prog = load_program(name)
  assert prog.SCALES == scales
  cfg = tmp_path / 'config.yaml'
  cfg.write_text(YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101'))
  common = ['--snapshot_dir', str(tmp_path / 's'), '--cfg_path', str(cfg), '--save_dir', str(tmp_path / 'o'),
            '--kmeans_num_clusters', '3,5', '--label_divisor', '2048']
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'train.txt'])
  assert info.value.code not in (0, None) and 'ListDataset' in str(info.value.code)
  from spml_amd.config.default import config
  assert config.network.kmeans_num_clusters == [3, 5]         # the reference's own arguments are taken
  if torch.cuda.is_available():
    return
  with pytest.raises(SystemExit) as info:
    prog.main(common + ['--data_list', 'synthetic'])
  assert info.value.code not in (0, None) and 'no CPU fallback' in str(info.value.code)
  assert not os.path.exists(str(tmp_path / 'o'))              # nothing was written
