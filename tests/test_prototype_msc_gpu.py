"""Multi-scale memory-bank generation on the GPU: the majority-label kernel of csrc/segment_majority.hip alone, exact
against `torch.bincount` / `torch.argmax` on the CPU (counts are integers: no tolerance anywhere), its edge behaviour and
limits, then `multiscale_prototypes` against the fixture exec'd from the reference's own lines
(tests/golden/n10_prototype_msc.npz; tests/test_prototype_msc.py keeps that fixture honest on the CPU) and the two
command-line programs.  Measured figures: profiles/prototype_msc.md."""
import ctypes
import functools
import json
import os

import pytest
import torch

from conftest import load_golden
from spml_amd import _ffi, inference
import spml_amd.utils.segsort.common as sc
import spml_amd.utils.segsort.others as so
from test_prototype_msc import SCALES, load_program, n10_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (P, m, ncls): one pixel; less than one wave; several workgroups with an LDS table; the bank pass of a 12 x 12 k-means
# on a label map with the ignore value (147 KiB of counters: the global table); the largest segment count
KERNEL_CASES = [(1, 1, 1), (37, 3, 5), (2640, 16, 5), (7200, 144, 256), (20000, 4096, 21)]


def cpu_reference(clu, sem, m, ncls):
  """(major, hist) on the CPU: bincount of the pixels inside [0, m) x [0, ncls), arg-max per row (first maximum)."""
  clu, sem = clu.cpu().reshape(-1), sem.cpu().reshape(-1)
  valid = (clu >= 0) & (clu < m) & (sem >= 0) & (sem < ncls)
  hist = torch.bincount(clu[valid] * ncls + sem[valid], minlength=m * ncls).view(m, ncls)
  return torch.argmax(hist, dim=1), hist


def random_maps(p, m, ncls, seed):
  gen = torch.Generator().manual_seed(seed)
  clu = torch.randint(0, m, (p,), generator=gen)
  sem = torch.randint(0, ncls, (p,), generator=gen)
  clu[-1], sem[0] = m - 1, ncls - 1                          # the largest id and the largest class occur
  return clu, sem


@functools.lru_cache(maxsize=None)
def kernel_case(index):
  p, m, ncls = KERNEL_CASES[index]
  clu, sem = random_maps(p, m, ncls, 1000 + index)
  major, hist = _ffi.segment_majority(clu.to(DEV), sem.to(DEV), m, ncls, want_hist=True)
  alone = _ffi.segment_majority(clu.to(DEV), sem.to(DEV), m, ncls)
  return dict(clu=clu, sem=sem, major=major.cpu(), hist=hist.cpu(), alone=alone.cpu(),
              want=cpu_reference(clu, sem, m, ncls))


@pytest.mark.parametrize('index', range(len(KERNEL_CASES)))
def test_kernel_is_exact_against_bincount_and_argmax(index):
  (p, m, ncls), r = KERNEL_CASES[index], kernel_case(index)
  want_major, want_hist = r['want']
  assert r['major'].dtype == r['hist'].dtype == torch.int64
  assert tuple(r['major'].shape) == (m,) and tuple(r['hist'].shape) == (m, ncls)
  assert int(r['hist'].sum()) == p
  assert torch.equal(r['hist'], want_hist) and torch.equal(r['major'], want_major)
  assert torch.equal(r['alone'], want_major)                  # (without the histogram output)


def test_kernel_cases_cover_both_count_paths():
  names = [_ffi.segment_majority_path_name(*case) for case in KERNEL_CASES]
  assert names == ['lds_table', 'lds_table', 'lds_table', 'global_table', 'global_table']


@pytest.mark.parametrize('m,ncls', [(4, 256), (40, 256)])     # LDS table; global table
def test_ties_resolve_to_the_lowest_class(m, ncls):
  """Constructed ties, also between classes that different lanes and different strides of the arg-max wave hold."""
  rows = {0: {2: 5, 4: 5},                                    # two classes tie
          1: {0: 3, 3: 3, 200: 3},                            # class 0 among them
          2: {70: 9, 200: 9, 6: 8},                           # both beyond the first 64 classes, a lower class with less
          3: {5: 4, 69: 4, 133: 4, 255: 4}}                   # all four in one lane of the wave (c % 64 == 5)
  clu = torch.tensor([s for s, row in rows.items() for c, n in row.items() for _ in range(n)])
  sem = torch.tensor([c for s, row in rows.items() for c, n in row.items() for _ in range(n)])
  perm = torch.randperm(clu.numel(), generator=torch.Generator().manual_seed(4))
  clu, sem = clu[perm], sem[perm]
  major, hist = _ffi.segment_majority(clu.to(DEV), sem.to(DEV), m, ncls, want_hist=True)
  want_major, want_hist = cpu_reference(clu, sem, m, ncls)
  assert want_major[:4].tolist() == [2, 0, 70, 5]
  assert torch.equal(major.cpu(), want_major) and torch.equal(hist.cpu(), want_hist)


@pytest.mark.parametrize('m', [6, 500])                       # LDS table; global table
def test_ids_and_labels_outside_the_ranges_count_nowhere(m):
  ncls = 21
  clu, sem = random_maps(3000, m, ncls, 77)
  gen = torch.Generator().manual_seed(78)
  pick = torch.randperm(3000, generator=gen)
  for chunk, value in zip(pick[:600].view(3, 200), (-1, ncls, 255)):
    sem[chunk] = value
  for chunk, value in zip(pick[600:1000].view(2, 200), (-1, m)):
    clu[chunk] = value
  clu[clu == 3] = 2
  clu[:40], sem[:40] = 3, torch.tensor([-1, ncls, 255, 2 ** 40]).repeat(10)      # segment 3 holds ignored pixels only
  major, hist = _ffi.segment_majority(clu.to(DEV), sem.to(DEV), m, ncls, want_hist=True)
  want_major, want_hist = cpu_reference(clu, sem, m, ncls)
  assert torch.equal(hist.cpu(), want_hist) and torch.equal(major.cpu(), want_major)
  assert int(hist.sum()) < 3000 - 900 and int(hist[3].sum()) == 0 and int(major[3]) == 0
  # with 256 classes the label 255 is a class like any other (the bank keeps such prototypes)
  major256, hist256 = _ffi.segment_majority(clu.to(DEV), sem.to(DEV), m, 256, want_hist=True)
  want_major, want_hist = cpu_reference(clu, sem, m, 256)
  assert torch.equal(hist256.cpu(), want_hist) and torch.equal(major256.cpu(), want_major)
  assert int(hist256[:, 255].sum()) == int(((sem == 255) & (clu >= 0) & (clu < m)).sum()) > 0


@pytest.mark.parametrize('m,ncls', [(3, 21), (144, 256)])     # LDS table; global table
def test_one_bin_holding_every_pixel_counts_them_all(m, ncls):
  """All 513 x 513 pixels in one segment and one class: the hottest bin there is, and more than 16 bits of count."""
  p = 513 * 513
  clu = torch.full((p,), m - 2, dtype=torch.int64, device=DEV)
  sem = torch.full((p,), 7, dtype=torch.int64, device=DEV)
  major, hist = _ffi.segment_majority(clu, sem, m, ncls, want_hist=True)
  assert int(hist[m - 2, 7]) == p == int(hist.sum()) and p > 65535
  want = torch.zeros(m, dtype=torch.int64)
  want[m - 2] = 7
  assert torch.equal(major.cpu(), want)


def raw_call(clu, sem, m, ncls, ws, major=None, hist=None, ws_bytes=None, p=None):
  """spml_segment_majority_i64 through the C-ABI with a workspace of the caller's -> (status, major, hist)."""
  lib = _ffi.lib()
  major = torch.full((max(m, 1),), -7, dtype=torch.int64, device=DEV) if major is None else major
  hist = torch.full((max(m, 1), max(ncls, 1)), -7, dtype=torch.int64, device=DEV) if hist is None else hist
  P = lambda t: ctypes.c_void_p(0 if t is False else t.data_ptr())
  rc = lib.spml_segment_majority_i64(P(clu), P(sem), clu.numel() if p is None else p, m, ncls, P(major), P(hist), P(ws),
                                     ws.numel() if ws_bytes is None else ws_bytes, _ffi.stream_ptr())
  return rc, major, hist


@pytest.mark.parametrize('index', [2, 3])                     # LDS table; global table
def test_dirty_workspace_and_repeated_calls_change_nothing(index):
  (p, m, ncls), r = KERNEL_CASES[index], kernel_case(index)
  clu, sem = r['clu'].to(DEV), r['sem'].to(DEV)
  need = _ffi.lib().spml_segment_majority_workspace_bytes(m, ncls)
  assert need == m * ncls * 4
  ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
  rc, major, hist = raw_call(clu, sem, m, ncls, ws)
  assert rc == 0 and torch.equal(major.cpu(), r['major']) and torch.equal(hist.cpu(), r['hist'])
  assert bool((ws[need:] == 0xAB).all())                      # nothing is written behind the stated size
  rc, major2, hist2 = raw_call(clu, sem, m, ncls, ws)         # the workspace now holds the counts of the first call
  assert rc == 0 and torch.equal(major2, major) and torch.equal(hist2, hist)
  was = _ffi.set_deterministic(True)
  try:
    rc, major3, hist3 = raw_call(clu, sem, m, ncls, ws)
  finally:
    _ffi.set_deterministic(was)
  assert rc == 0 and torch.equal(major3, major) and torch.equal(hist3, hist)


def test_limits_and_argument_errors_through_the_c_abi():
  """The entry's own checks: nothing is launched for any of them."""
  INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
  clu = torch.zeros(64, dtype=torch.int64, device=DEV)
  sem = torch.zeros(64, dtype=torch.int64, device=DEV)
  ws = torch.zeros(4097 * 257 * 4, dtype=torch.uint8, device=DEV)
  assert raw_call(clu, sem, 4096, 256, ws)[0] == 0
  assert raw_call(clu, sem, 4097, 21, ws)[0] == UNSUPPORTED and raw_call(clu, sem, 144, 257, ws)[0] == UNSUPPORTED
  assert raw_call(clu, sem, 144, 21, ws, p=2 ** 31)[0] == UNSUPPORTED
  assert raw_call(clu, sem, 0, 21, ws)[0] == INVALID and raw_call(clu, sem, 144, 0, ws)[0] == INVALID
  assert raw_call(clu, sem, 144, 21, ws, p=-1)[0] == INVALID
  assert raw_call(False, sem, 144, 21, ws, p=64)[0] == INVALID and raw_call(clu, False, 144, 21, ws, p=64)[0] == INVALID
  assert raw_call(clu, sem, 144, 21, ws, major=False)[0] == INVALID
  assert raw_call(clu, sem, 144, 21, ws, hist=False)[0] == 0                       # the histogram is optional
  assert raw_call(clu, sem, 8, 8, ws, major=clu)[0] == INVALID                     # an output aliases an input
  assert raw_call(clu, sem, 2, 2, ws, hist=sem)[0] == INVALID
  assert raw_call(clu, sem, 8, 8, clu.view(torch.uint8))[0] == INVALID             # ... the workspace does
  assert raw_call(clu, sem, 144, 21, False, ws_bytes=1 << 20)[0] == WORKSPACE
  assert raw_call(clu, sem, 144, 21, ws, ws_bytes=144 * 21 * 4 - 1)[0] == WORKSPACE
  assert raw_call(clu, sem, 3, 4, ws, p=0)[0] == 0                                 # no pixels: every row gives 0
  torch.cuda.synchronize()
  # the wrapper
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.segment_majority(clu, sem, 4097, 21)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.segment_majority(clu, sem[:10], 4, 21)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.segment_majority(clu, sem.int(), 4, 21)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.segment_majority(clu.cpu(), sem.cpu(), 4, 21)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.segment_majority(clu, sem, 0, 21)
  strided = (torch.arange(128, device=DEV) % 8 // 2).view(64, 2)[:, 0]            # ids 0..3; made contiguous by the wrapper
  assert not strided.is_contiguous()
  assert torch.equal(_ffi.segment_majority(strided, strided, 4, 4).cpu(), torch.arange(4))
  rc, major, _ = raw_call(clu, sem, 3, 4, ws, p=0)
  assert rc == 0 and torch.equal(major.cpu(), torch.zeros(3, dtype=torch.int64))


@pytest.mark.parametrize('m,ncls', [(4097, 5), (10, 257)])
def test_outside_the_limits_the_framework_formulation_answers(m, ncls):
  """Every segment holds its majority class twice and its neighbour class once (no ties, no empty row: the arg-max of
  the framework ops on a GPU is then the CPU's), plus pixels outside the ranges, which the framework path ignores too."""
  ids = torch.arange(m)
  top = ids % ncls if ncls <= 5 else (ids * 29 + 250) % ncls     # (with 257 classes: the classes 250 .. 256 and lower ones)
  clu = torch.cat([ids, ids, ids, torch.tensor([-1, m, 0, 1])])
  sem = torch.cat([top, top, (top + 1) % ncls, torch.tensor([0, 0, -1, ncls])])
  perm = torch.randperm(clu.numel(), generator=torch.Generator().manual_seed(m))
  clu, sem = clu[perm], sem[perm]
  want_major, _ = cpu_reference(clu, sem, m, ncls)
  assert torch.equal(want_major, top)
  labels, path = sc.segment_majority_labels(sem.to(DEV), clu.to(DEV), m, ncls)
  assert path == sc.FRAMEWORK_MAJORITY_PATH == 'framework_majority'
  assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), want_major)
  # ... and inside them the same inputs (those that fit) take the kernel, with equal labels
  m_in, ncls_in = min(m, 4096), min(ncls, 256)
  labels, path = sc.segment_majority_labels(sem.to(DEV), clu.to(DEV), m_in, ncls_in)
  assert path == sc.HIP_MAJORITY_PATH == 'hip_majority'
  assert torch.equal(labels.cpu(), cpu_reference(clu, sem, m_in, ncls_in)[0])


def test_majority_labels_are_those_of_find_majority_label_index():
  """On maps inside the ranges the new function gives the labels of the existing one (which reads both sizes back)."""
  clu, sem = random_maps(5000, 30, 21, 5)
  sem[sem == 20] = 255
  _, want = sc.find_majority_label_index(sem.to(DEV), clu.to(DEV))
  labels, path = sc.segment_majority_labels(sem.view(50, 100).to(DEV), clu.view(50, 100).to(DEV), 30)
  want_major, want_hist = cpu_reference(clu, sem, 30, 256)
  assert path == 'hip_majority' and torch.equal(labels.cpu(), want_major)
  top2 = want_hist.topk(2, dim=1).values
  clear = top2[:, 0] > top2[:, 1]                             # (the existing function's arg-max runs on the GPU: its tie
  assert clear.sum() >= 20                                    # order is not pinned, so tied rows are left out)
  assert torch.equal(labels.cpu()[clear], want.cpu()[clear])


# ---------------------------------------------------------------------------
# multiscale_prototypes against tests/golden/n10_prototype_msc.npz
@pytest.mark.parametrize('ci', [0, 1])
def test_tail_on_the_fixtures_own_segments_matches_reference_lines(ci):
  """Prototypes and majority labels given the reference's own clustering, per view and for the bank: labels equal,
  prototypes within the atol = 1e-5 of test_inference_gpu.py::test_full_resolution_pass_matches_reference_lines."""
  from oracle import spml_oracle as O
  g = load_golden('n10_prototype_msc')
  cfg, _, views = n10_case(g, ci)
  bank, bank_lab = [], []
  for v in views:
    clu = v['cluster_index'].to(DEV)
    emb = O.normalize_embedding(v['embedding'].permute(0, 2, 3, 1).contiguous()).reshape(clu.shape[0], -1)
    protos = sc.calculate_prototypes_from_labels(emb.to(DEV), clu)
    torch.testing.assert_close(protos.cpu(), v['prototypes'], rtol=0, atol=1e-5)
    labels, path = sc.segment_majority_labels(v['label'].to(DEV), clu, protos.shape[0], 256)
    assert path == 'hip_majority' and torch.equal(labels.cpu(), v['labels'])
    bank.append(protos)
    bank_lab.append(labels)
  t = 'c%d_' % ci
  torch.testing.assert_close(torch.cat(bank, 0).cpu(), g[t + 'bank'], rtol=0, atol=1e-5)
  assert torch.equal(torch.cat(bank_lab, 0).cpu(), g[t + 'bank_lab'].long())


@pytest.mark.parametrize('ci', [0, 1])
def test_multiscale_end_to_end_matches_reference_lines(ci, tmp_path):
  """Stub embedder and k-means on the GPU, with the bounds of the N2 test (k-means near ties on a GPU convolution's output
  may flip): cluster maps agree on more than 0.97 of the pixels of every view, labels on more than 0.85 of the
  prototypes; bank shapes and view order are the reference's; the bank file is read back identically."""
  from test_inference_gpu import TinyEmbedder
  g = load_golden('n10_prototype_msc')
  cfg, image, views = n10_case(g, ci)
  t = 'c%d_' % ci
  model = TinyEmbedder(cfg['c'], cfg['grid']).to(DEV)
  model.conv.load_state_dict({'weight': g[t + 'conv_w'].to(DEV), 'bias': g[t + 'conv_b'].to(DEV)})
  made = inference.flip_scale_views(image.to(DEV), SCALES, False, cfg['crop'])
  labels = inference.label_views(views[1]['label'].to(DEV), [v[1] for v in made])
  out = inference.multiscale_prototypes(model, made, labels, cfg['crop'], cfg['stride'])
  assert out['majority_path'] == 'hip_majority'
  assert out['segment_counts'] == [v['labels'].shape[0] for v in views]             # view order and sizes
  assert tuple(out['prototype'].shape) == tuple(g[t + 'bank'].shape)
  assert tuple(out['prototype_label'].shape) == tuple(g[t + 'bank_lab'].shape) and out['prototype_label'].dtype == torch.int64
  for vi, v in enumerate(views):
    (_, (rh, rw), _), emb_want = made[vi], v['embedding']
    emb = inference.embed_full_resolution(model, made[vi][0], cfg['crop'], cfg['stride'])[..., :rh, :rw]
    torch.testing.assert_close(emb.cpu(), emb_want, rtol=1e-4, atol=2e-6)          # (the N2 test's bound)
    agree = (out['cluster_index'][vi].cpu() == v['cluster_index']).float().mean().item()
    print('case %d view %d: cluster maps agree on %.4f' % (ci, vi, agree))
    assert agree > 0.97, (vi, agree)
  same = (out['prototype_label'].cpu() == g[t + 'bank_lab'].long()).float().mean().item()
  print('case %d: labels agree on %.4f of the prototypes' % (ci, same))
  assert same > 0.85, same
  # the labels are the majority of this run's own segments, exactly
  off = 0
  for vi, m in enumerate(out['segment_counts']):
    want = cpu_reference(out['cluster_index'][vi], labels[vi], m, 256)[0]
    assert torch.equal(out['prototype_label'][off:off + m].cpu(), want)
    off += m
  # memory-bank file in the reference's format, read back by the loader
  inference.save_image_memory(str(tmp_path / 'img0.npy'), out['prototype'], out['prototype_label'])
  p2, l2 = so.load_memory_banks(str(tmp_path))
  assert torch.equal(p2, out['prototype'].cpu()) and torch.equal(l2, out['prototype_label'].cpu())
  kept, kept_lab = inference.drop_ignored_memory(out['prototype'], out['prototype_label'])
  ignored = out['prototype_label'] == 255
  assert kept.shape[0] == int((~ignored).sum()) and not bool((kept_lab == 255).any())
  assert torch.equal(kept, out['prototype'][~ignored]) and torch.equal(kept_lab, out['prototype_label'][~ignored])
  if ci == 1:
    assert 0 < int(ignored.sum()) < ignored.numel()
  else:
    assert int(ignored.sum()) == 0


@pytest.fixture(scope='module')
def tiny_snapshot(tmp_path_factory):
  """A two-class config with crop 65 and a snapshot of a freshly initialised network, written once for both programs."""
  from test_train_cli import YAML
  root = tmp_path_factory.mktemp('prototype_cli')
  yaml = (YAML.replace('panoptic_deeplab_50', 'panoptic_deeplab_101').replace('num_classes: 21', 'num_classes: 2')
          .replace('image_size: 97', 'image_size: 65').replace('- 97', '- 65'))
  yaml = yaml.replace('stride:\n    - 65\n    - 65', 'stride:\n    - 43\n    - 43')
  assert 'num_classes: 2' in yaml and yaml.count('- 65') == 4 and yaml.count('- 43') == 2
  cfg = root / 'config.yaml'
  cfg.write_text(yaml)
  from spml_amd.config.default import config, update_config
  from spml_amd.models.embeddings.resnet_deeplab import resnet_101_deeplab
  update_config(str(cfg))
  torch.manual_seed(9)
  snap = root / 'snapshot'
  os.makedirs(str(snap))
  torch.save({'embedding_model': resnet_101_deeplab(config).state_dict()},
             str(snap / 'model-{:d}.pth'.format(config.train.max_iteration - 1)))
  return cfg, snap


@pytest.mark.parametrize('name,num_views', [('prototype', 1), ('prototype_msc', 3)])
def test_programs_write_banks_the_loader_reads(name, num_views, tiny_snapshot, tmp_path, capsys, monkeypatch):
  import spml_amd.inference_cli as cli
  cfg, snap = tiny_snapshot
  monkeypatch.setattr(cli, 'NUM_SYNTHETIC_IMAGES', 2)
  prog = load_program(name)
  save = tmp_path / 'results'
  capsys.readouterr()
  prog.main(['--snapshot_dir', str(snap), '--cfg_path', str(cfg), '--save_dir', str(save), '--data_list', 'synthetic',
             '--kmeans_num_clusters', '4,4', '--label_divisor', '2048'])
  line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
  result = json.loads(line)
  for key in ('images', 'images_per_s', 'prototypes_per_image', 'views', 'scales', 'majority_path', 'snapshot', 'save_dir'):
    assert key in result, key
  assert result['images'] == 2 and result['images_per_s'] > 0 and result['views'] == num_views
  assert result['majority_path'] == 'hip_majority' and result['scales'] == prog.SCALES
  assert result['save_dir'] == str(save / 'semantic_prototype')
  files = sorted(os.listdir(result['save_dir']))
  assert files == ['synthetic_0000.npy', 'synthetic_0001.npy']
  protos, labels = so.load_memory_banks(result['save_dir'])
  per_image = result['prototypes_per_image']
  assert len(per_image) == 2 and all(0 < n <= 16 * num_views for n in per_image)
  assert protos.shape == (sum(per_image), 32) and labels.shape == (sum(per_image),)
  assert set(labels.tolist()) <= {0, 1, 255}
  torch.testing.assert_close(protos.norm(dim=1), torch.ones(protos.shape[0]), rtol=0, atol=1e-5)
