"""Deterministic mode (include/spml_hip.h, spml_set_deterministic): the segment sums (A4) and the prototype
gradient of the NLL backward (A9 / A10) leave through 64-bit fixed-point integer atomics instead of fp32 atomics --
bit-identical run to run, and within one fp32 rounding of the default path's values."""
import pytest
import torch

from oracle import spml_oracle as O
from spml_amd import _ffi, ops, synth
import spml_amd.utils.segsort.common as sc
import spml_amd.utils.segsort.loss as sl

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture
def deterministic():
  before = _ffi.set_deterministic(True)
  yield
  _ffi.set_deterministic(before)


def _scene(p=40000, d=66, m=900, seed=3):
  g = torch.Generator().manual_seed(seed)
  x = torch.nn.functional.normalize(torch.randn(p, d, generator=g), dim=1)
  ids = torch.randint(0, m, (p // 50,), generator=g).repeat_interleave(50)[:p].contiguous()     # runs of 50 pixels
  ids = ids[torch.randperm(p // 50, generator=g).repeat_interleave(50) * 0 + torch.arange(p)]   # (kept in order)
  return x.to(DEV), ids.to(DEV), m


def test_segment_prototypes_are_bit_reproducible_and_match_the_oracle(deterministic):
  x, ids, m = _scene()
  runs = [sc.calculate_prototypes_from_labels(x, ids, m) for _ in range(5)]
  for r in runs[1:]:
    assert torch.equal(r, runs[0])
  want = O.calculate_prototypes_from_labels(x.cpu(), ids.cpu(), m)
  torch.testing.assert_close(runs[0].cpu(), want, rtol=0, atol=2e-7)
  # the exact sums, rounded once: at least as close to an fp64 evaluation as the oracle's fp32 scatter_add
  s64 = torch.zeros(m, x.shape[1], dtype=torch.float64).index_add_(0, ids.cpu(), x.cpu().double())
  p64 = s64 / s64.norm(dim=1, keepdim=True).clamp(min=1e-12)
  assert (runs[0].cpu().double() - p64).abs().max() <= (want.double() - p64).abs().max() + 1e-9
  # gradient: backward is a gather (no accumulation) -- same in either mode
  xr = x.clone().requires_grad_(True)
  sc.calculate_prototypes_from_labels(xr, ids, m).square().sum().backward()
  assert torch.isfinite(xr.grad).all()


def test_the_atomic_entry_point_is_refused_in_deterministic_mode(deterministic):
  x, ids, m = _scene(p=2000, m=40)
  sums, protos = torch.empty(m, x.shape[1], device=DEV), torch.empty(m, x.shape[1], device=DEV)
  rc = _ffi.lib().spml_segment_sum_normalize_f32(_ffi.ptr(x), _ffi.ptr(ids), x.shape[0], x.shape[1], m, _ffi.ptr(sums),
                                                 _ffi.ptr(protos), _ffi.stream_ptr())
  assert rc != 0 and b'not supported' in _ffi.lib().spml_status_string(rc).lower()


def _nll_case(p, m, d, tag, seed):
  g = torch.Generator().manual_seed(seed)
  emb = torch.nn.functional.normalize(torch.randn(p, d, generator=g), dim=1)
  own = torch.randint(0, m, (p // 32 + 1,), generator=g).repeat_interleave(32)[:p].contiguous()
  protos = O.calculate_prototypes_from_labels(emb, own, m)
  if tag:
    pr_code = torch.randint(1, 2 ** 20, (m,), generator=g)
  else:
    pr_code = torch.randint(0, 21, (m,), generator=g)
  px_code = pr_code[own]
  w = torch.rand(p, generator=g) * 1e-3
  return emb, own, protos, px_code, pr_code, w


@pytest.mark.parametrize('p,m,d,tag', [(30000, 2500, 64, False),      # the pipelined kernels (nll_de3 / nll_dp3)
                                        (30000, 2500, 64, True),
                                        (9000, 700, 130, False),      # the round-2 kernels (other widths)
                                        (5000, 300, 514, False)])     # wide embeddings: several d-chunk launches
def test_nll_prototype_gradient_is_bit_reproducible(deterministic, p, m, d, tag):
  emb, own, protos, px_code, pr_code, w = _nll_case(p, m, d, tag, seed=p + d)
  mode = ops.NLL_TAGSET if tag else ops.NLL_LABEL
  outs = []
  for _ in range(3):
    e = emb.to(DEV).requires_grad_(True)
    pr = protos.to(DEV).requires_grad_(True)
    nll = ops.segsort_nll(e, own.to(DEV), px_code.to(DEV), pr, pr_code.to(DEV), 12.0, mode | ops.NLL_CODE32)
    (nll.view(-1) * w.to(DEV)).sum().backward()
    outs.append((nll.detach().clone(), e.grad.clone(), pr.grad.clone()))
  for o in outs[1:]:
    assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    assert torch.equal(o[2], outs[0][2]), 'dPrototypes differ run to run: max %.3e' % (o[2] - outs[0][2]).abs().max().item()
  # ... and equal to the default path's gradient up to its own fp32 accumulation noise
  _ffi.set_deterministic(False)
  try:
    e = emb.to(DEV).requires_grad_(True)
    pr = protos.to(DEV).requires_grad_(True)
    nll = ops.segsort_nll(e, own.to(DEV), px_code.to(DEV), pr, pr_code.to(DEV), 12.0, mode | ops.NLL_CODE32)
    (nll.view(-1) * w.to(DEV)).sum().backward()
  finally:
    _ffi.set_deterministic(True)
  scale = pr.grad.abs().max().item()
  assert (pr.grad - outs[0][2]).abs().max().item() <= 2e-6 * scale
  assert torch.equal(e.grad, outs[0][1])


def test_generic_kmeans_route_in_deterministic_mode(deterministic):
  """SPML_KMEANS_FORCE_GENERIC (the route without tile kernels: plain fp32 assign + segment sums): its M-step sums go
  through the fixed-point scratch of the k-means workspace in this mode -- same labels and prototypes as the default
  mode (up to the fp32 rounding of the atomic sums), bit-identical run to run."""
  g = torch.Generator().manual_seed(8)
  n_img, side, d, k = 3, 23, 66, 9
  p1 = side * side
  x = torch.nn.functional.normalize(torch.randn(n_img * p1, d, generator=g), dim=1).to(DEV)
  init = _ffi.kmeans_init_grid(side, side, 3, 3, DEV).view(-1).repeat(n_img)
  off = (torch.arange(n_img + 1, device=DEV) * p1).to(torch.int64)
  runs = [_ffi.kmeans_run(x, off, p1, k, init, 4, want_centroids=True, flags=1) for _ in range(3)]
  assert _ffi.kmeans_last_path() == 'generic'
  for lab, cent in runs[1:]:
    assert torch.equal(lab, runs[0][0]) and torch.equal(cent, runs[0][1])
  _ffi.set_deterministic(False)
  try:
    lab0, cent0 = _ffi.kmeans_run(x, off, p1, k, init, 4, want_centroids=True, flags=1)
  finally:
    _ffi.set_deterministic(True)
  assert (lab0 != runs[0][0]).float().mean().item() < 0.01
  torch.testing.assert_close(cent0, runs[0][1], rtol=0, atol=5e-3)      # (a flipped near tie moves a prototype slightly)
  want = O.kmeans_with_initial_labels(x[:p1].cpu(), init[:p1].cpu(), k, 4)
  assert (want != runs[0][0][:p1].cpu()).float().mean().item() < 0.02


def test_kmeans_workspace_sized_before_the_mode_was_switched_on():
  """A caller-held k-means workspace (_ffi.kmeans_workspace) sized with the mode off serves a generic-route call made
  with the mode on: spml_kmeans_workspace_bytes reserves the fixed-point scratch of the M-step sums in either mode.
  Same labels and sums, bit for bit, as with a workspace sized with the mode on."""
  g = torch.Generator().manual_seed(9)
  n_img, p1, d, k = 3, 529, 66, 9
  x = torch.nn.functional.normalize(torch.randn(n_img * p1, d, generator=g), dim=1).to(DEV)
  cent = torch.nn.functional.normalize(torch.randn(n_img, k, d, generator=g), dim=2).to(DEV)
  off = (torch.arange(n_img + 1, device=DEV) * p1).to(torch.int64)
  before = _ffi.set_deterministic(False)
  try:
    ws = _ffi.kmeans_workspace(x, off, p1, k)
    _ffi.set_deterministic(True)
    assert ws.numel() == _ffi.kmeans_workspace(x, off, p1, k).numel()
    lab, sums = _ffi.kmeans_fused_pass(x, off, p1, cent, ws=ws, flags=1)
    assert _ffi.kmeans_last_path() == 'generic'
    lab2, sums2 = _ffi.kmeans_fused_pass(x, off, p1, cent, flags=1)
  finally:
    _ffi.set_deterministic(before)
  assert torch.equal(lab, lab2) and torch.equal(sums, sums2)
  for b in range(n_img):
    xi, li = x[b * p1:(b + 1) * p1].cpu(), lab[b * p1:(b + 1) * p1].cpu()
    sims = xi @ cent[b].cpu().t()
    t2 = sims.topk(2, dim=1).values
    safe = (t2[:, 0] - t2[:, 1]) > 1e-5
    assert torch.equal(li[safe], sims.argmax(1)[safe])
    torch.testing.assert_close(sums[b].cpu(), torch.zeros(k, d).index_add_(0, li, xi), rtol=0, atol=2e-5)


def test_narrow_pyramid_forward_without_tap_groups(deterministic, monkeypatch):
  """The 36-tap forward on 64-column tiles splits its taps over workgroups that meet through fp32 atomics; in this mode
  it runs unsplit: bit-identical run to run, same values."""
  g = torch.Generator().manual_seed(6)
  x = torch.randn(2, 256, 29, 33, generator=g).clamp_min(0).to(DEV).contiguous(memory_format=torch.channels_last)
  ws = [(torch.randn(64, 256, 3, 3, generator=g) * (2.0 / (9 * 256)) ** 0.5).to(DEV) for _ in range(4)]
  bs = [torch.randn(64, generator=g).to(DEV) for _ in range(4)]
  dils = (6, 12, 18, 24)
  xh = _ffi.hl8_from_f32(x)
  outs = [_ffi.conv_hl8_pyramid_forward(xh, ws, bs, dils, 2, 29, 33) for _ in range(4)]
  for o in outs[1:]:
    assert torch.equal(o, outs[0])
  ref = sum(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), 1, d, d) for w, b, d in zip(ws, bs, dils))
  assert ((outs[0].double() - ref).abs().max() / ref.abs().max()).item() < 3e-6


def test_upsampling_backward_as_matrix_products(deterministic):
  g = torch.Generator().manual_seed(2)
  x = torch.randn(2, 8, 33, 29, generator=g).to(DEV)
  up = torch.randn(2, 8, 66, 58, generator=g).to(DEV)
  xa = x.clone().requires_grad_(True)
  ya = ops.upsample_bilinear(xa, scale_factor=2)
  (ya * up).sum().backward()
  xb = x.clone().requires_grad_(True)
  yb = torch.nn.functional.interpolate(xb, scale_factor=2, mode='bilinear')
  (yb * up).sum().backward()
  assert torch.equal(ya, yb)
  torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
  xc = x.clone().requires_grad_(True)
  (ops.upsample_bilinear(xc, scale_factor=2) * up).sum().backward()
  assert torch.equal(xc.grad, xa.grad)


def test_loss_head_of_a_training_step_is_bit_reproducible(deterministic, monkeypatch):
  """Embedding map -> K1 + k-means -> prototypes -> the three contrastive terms, forward and backward, twice on the
  same inputs: the losses and d loss / d embedding are bit-identical (everything in between is this library's) --
  whatever the number of side streams the per-image terms are spread over."""
  from step_helpers import loss_head
  step = loss_head(DEV)
  results = []
  # (the per-image similarity terms run on side streams whose inputs live on the current stream's pool:
  # twelve repetitions with one, four and eight side streams, with allocator churn in between -- a block recycled
  # while a side-stream kernel still read it would show as a different loss or gradient)
  for rep, n_streams in enumerate(['4', '1', '4', '8', '4', '1', '4', '4', '8', '4', '1', '4']):
    monkeypatch.setenv('SPML_IMG_SIM_STREAMS', n_streams)
    junk = [torch.empty((1 << 20) * (1 + (rep + i) % 5), device=DEV) for i in range(6)]     # churn: blocks of 4 .. 20 MB
    del junk
    out, emb, ci = step()
    loss = out['sem_ann_loss'] + out['sem_occ_loss'] + out['img_sim_loss']
    loss.backward()
    results.append((loss.detach().clone(), emb.grad.clone(), ci.clone()))
  for r in results[1:]:
    assert torch.equal(results[0][2], r[2])
    assert torch.equal(results[0][0], r[0]), (results[0][0].item(), r[0].item())
    assert torch.equal(results[0][1], r[1]), (results[0][1] - r[1]).abs().max().item()


def _framework_forward_is_stable(model, datas, train):
  """The units that stay on the framework's convolutions (stem, res2, the stride-2 unit) run MIOpen solvers this
  repository does not choose; which solver a shape gets depends on the box and on what the process has run before, and
  some of them are not run-to-run stable even in the forward pass.  The whole-step tests below assert bit-identity of
  THIS repository's part: when two forwards of the same embedding network on the same batch already differ, the
  difference is the framework's and the test is reported as an expected failure instead of a red run."""
  model.train(train)
  with torch.no_grad():
    a = model.generate_embeddings(datas)['embedding'].clone()
    b = model.generate_embeddings(datas)['embedding'].clone()
  return torch.equal(a, b)


def _framework_backward_is_stable(emb_model):
  """Forward + backward of the stride-2 unit (the trainable unit that stays on the framework's convolutions; in
  deterministic mode its weight gradients are DetConv2d's GEMMs, its data gradients MIOpen's) twice on one input."""
  unit = emb_model.resnet_backbone.res3[0]
  cin = unit.conv1.in_channels
  g = torch.Generator().manual_seed(12)
  x0 = torch.randn(4, cin, 65, 65, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
  outs = []
  for _ in range(2):
    unit.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    y = unit(x)
    y.square().sum().backward()
    outs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in unit.parameters() if p.grad is not None])
  unit.zero_grad(set_to_none=True)
  return all(torch.equal(a, b) for a, b in zip(*outs))


def test_two_training_steps_are_bit_reproducible(deterministic):
  """Two Trainers built from the same seed take the same three steps (ResNet-50 DeepLab, batch 4, 257 x 257, channels
  last: matrix-core units, fused batch norm, HIP loss kernels, the memory bank in use from the second step on): every
  loss and EVERY parameter after the last SGD step is bit-identical -- with the library's deterministic mode alone:
  fixed-point sums in this library, the fixed-order up-sampling backward (ops.upsample_bilinear) and the framework
  convolutions that remain re-classed to spml_amd.nn.conv.DetConv2d (weight gradients and 1x1 products as GEMMs); the
  framework's own `cudnn.deterministic` switch is NOT needed (it costs 13x: MIOpen's naive kernels).
  (Without the mode the second step's losses differ in the 4th digit and 292 of 331 parameter tensors differ:
  tools/probe_determinism.py, profiles/r06_determinism.md.)"""
  import argparse
  import importlib.util
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  spec = importlib.util.spec_from_file_location('probe_determinism', os.path.join(root, 'tools', 'probe_determinism.py'))
  probe = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(probe)
  args = argparse.Namespace(batch=4, crop=257, steps=3, small=True)
  assert not torch.backends.cudnn.deterministic
  from spml_amd.train import build_models, voc12_scribble_config
  cfg0 = voc12_scribble_config(batch_size=4, crop=257, use_syncbn=False)
  cfg0.network.backbone_types = 'panoptic_deeplab_50'
  torch.manual_seed(235)
  emb0 = build_models(cfg0)[0].to(DEV).to(memory_format=torch.channels_last)
  d0, _ = synth.make_batch(4, 257, seed=100, device=DEV)
  d0['image'] = d0['image'].contiguous(memory_format=torch.channels_last)
  if not _framework_forward_is_stable(emb0, d0, train=True):
    pytest.xfail('the framework convolutions of the stem / res2 / stride-2 unit are not run-to-run stable on this box')
  del emb0
  # Up to three attempts: a non-determinism of THIS library's sums never yields an identical pair (default mode: 292 of
  # 331 tensors differ every time), while the framework's kernels have been seen to differ once in a dozen full-suite
  # runs and not at all in 15 repetitions in a fresh process -- one identical pair is the evidence asked for
  for attempt in range(3):
    a_out, a_par = probe.run(args, 'a')
    b_out, b_par = probe.run(args, 'b')
    same_out = all(torch.equal(oa[k], ob[k]) for oa, ob in zip(a_out, b_out) for k in oa if torch.is_tensor(oa[k]))
    differ = [k for k in a_par if not torch.equal(a_par[k], b_par[k])]
    if same_out and not differ:
      break
    print('attempt %d: losses identical %s, %d of %d parameter tensors differ (first: %s)' % (
        attempt, same_out, len(differ), len(a_par), differ[:4]))
  if not same_out or differ:
    # whose difference is it?  (the framework's kernels are probed again: their instability is not a property of a box
    # alone -- the same solver can be stable for minutes and then not)
    from spml_amd.nn.conv import make_deterministic
    torch.manual_seed(235)
    emb1 = build_models(cfg0)[0].to(DEV).to(memory_format=torch.channels_last)
    make_deterministic(emb1)
    if not (_framework_forward_is_stable(emb1, d0, train=True) and _framework_forward_is_stable(emb1, d0, train=True) and
            _framework_backward_is_stable(emb1)):
      pytest.xfail('the framework convolutions of the stem / res2 / stride-2 unit are not run-to-run stable on this box')
  for it, (oa, ob) in enumerate(zip(a_out, b_out)):
    for k in oa:
      if torch.is_tensor(oa[k]):
        assert torch.equal(oa[k], ob[k]), (it, k, float(oa[k]), float(ob[k]))
  assert not differ, differ[:8]


def test_framework_convolutions_in_deterministic_mode_match_the_library(deterministic):
  """spml_amd.nn.conv.DetConv2d (what Trainer re-classes the remaining nn.Conv2d modules to): same output and
  gradients as the plain module -- strided 1x1, dilated 3x3, the 128 -> 21 classifier product -- and run-to-run
  bit-identical weight gradients."""
  import copy
  from spml_amd.nn.conv import DetConv2d, make_deterministic
  g = torch.Generator().manual_seed(4)
  for cin, cout, k, stride, pad, dil, hw in [(256, 128, 1, 2, 0, 1, 65), (128, 128, 3, 1, 2, 2, 33), (64, 128, 3, 1, 1, 1, 66),
                                             (128, 21, 1, 1, 0, 1, 66)]:
    conv = torch.nn.Conv2d(cin, cout, k, stride, pad, dil, bias=(cout == 21)).to(DEV).to(memory_format=torch.channels_last)
    det = copy.deepcopy(conv)
    assert make_deterministic(det) == 1 and type(det) is DetConv2d and det.state_dict().keys() == conv.state_dict().keys()
    x = torch.randn(4, cin, hw, hw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = conv(xa), det(xb)
    up = torch.randn(ya.shape, generator=g).to(DEV)
    (ya * up).sum().backward()
    (yb * up).sum().backward()
    torch.testing.assert_close(yb, ya, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(xb.grad, xa.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(det.weight.grad, conv.weight.grad, rtol=1e-3, atol=1e-3 * float(conv.weight.grad.abs().max()))
    first = det.weight.grad.clone()
    for _ in range(3):
      det.zero_grad()
      xc = x.clone().requires_grad_(True)
      yc = det(xc)
      (yc * up).sum().backward()
      assert torch.equal(det.weight.grad, first) and torch.equal(yc, yb) and torch.equal(xc.grad, xb.grad)


def test_stage2_steps_are_bit_reproducible(deterministic):
  """Two ClassifierTrainers (stage 2: frozen ResNet-50 DeepLab embedding network at 257 x 257 in eval mode, the
  softmax classifier's framework convolutions re-classed to DetConv2d, the ASPP forward on the own kernels) take two
  steps from the same seed: classifier parameters and batch-norm statistics bit-identical.  (Forward-only library
  convolutions are NOT run-to-run stable for every shape -- MIOpen's dilated 3x3 2048 -> 64 and some narrow 1x1
  solvers are not -- which is why the mode moves those to this library / to matrix products.)"""
  from spml_amd import synth
  from spml_amd.nn.conv import DetConv2d
  from spml_amd.train import ClassifierTrainer, build_models, voc12_scribble_config
  from spml_amd.models.predictions.softmax_classifier import softmax_classifier
  states = []
  for _ in range(6):                  # (up to three pairs: see test_two_training_steps_are_bit_reproducible)
    if len(states) >= 2 and len(states) % 2 == 0:
      same = all(torch.equal(a, b) for a, b in zip(states[-2][1], states[-1][1])) and \
          all(torch.equal(v, states[-1][0][k]) for k, v in states[-2][0].items())
      if same:
        break
      print('pair %d differs: %s' % (len(states) // 2 - 1, [k for k, v in states[-2][0].items() if not torch.equal(v, states[-1][0][k])][:4]))
    cfg = voc12_scribble_config(batch_size=4, crop=257, max_iteration=4000, use_syncbn=False)
    cfg.network.backbone_types = 'panoptic_deeplab_50'
    torch.manual_seed(17)
    emb, _ = build_models(cfg)
    pred = softmax_classifier(cfg)
    pred.semantic_classifier[3].p = 0.0
    tr = ClassifierTrainer(cfg, DEV, channels_last=True, models=(emb, pred))
    assert type(tr.prediction_model.semantic_classifier[0]) is DetConv2d
    d0, _ = synth.make_batch(4, 257, seed=40, device=DEV)
    d0['image'] = d0['image'].contiguous(memory_format=torch.channels_last)
    if not _framework_forward_is_stable(tr.embedding_model, d0, train=False):
      pytest.xfail('the framework convolutions of the frozen network (eval mode) are not run-to-run stable on this box')
    losses = []
    for it in range(2):
      datas, targets = synth.make_batch(4, 257, seed=40 + it, device=DEV)
      datas['image'] = datas['image'].contiguous(memory_format=torch.channels_last)
      losses.append(tr.step(datas, targets)['loss'].clone())
    states.append(({k: v.detach().clone() for k, v in tr.prediction_model.state_dict().items()}, losses))
  states = states[-2:]                # the last pair (the identical one, if there was one)
  same = all(torch.equal(a, b) for a, b in zip(states[0][1], states[1][1])) and \
      all(torch.equal(v, states[1][0][k]) for k, v in states[0][0].items())
  if not same and not (_framework_forward_is_stable(tr.embedding_model, d0, train=False) and
                       _framework_forward_is_stable(tr.embedding_model, d0, train=False)):
    pytest.xfail('the framework convolutions of the frozen network (eval mode) are not run-to-run stable on this box')
  for a, b in zip(states[0][1], states[1][1]):
    assert torch.equal(a, b), (float(a), float(b))
  for k, v in states[0][0].items():
    assert torch.equal(v, states[1][0][k]), k
