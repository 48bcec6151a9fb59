"""Fused training-mode batch norm + ReLU + residual (spml_amd/csrc/bn_act.hip) against the
framework ops it replaces in the bottleneck unit (spml/models/backbones/resnet.py:42-63)."""
import pytest
import torch

from spml_amd import ops

DEV = 'cuda:0'


def test_rank_statistics_merge_is_the_pooled_variance():
  """merge_bn_statistics (the SyncBatchNorm combination of per-rank statistics) on CPU."""
  g = torch.Generator().manual_seed(0)
  parts = [torch.randn(n, 7, generator=g) * (i + 1) + i for i, n in enumerate((50, 31, 64))]
  counts = torch.tensor([[float(p.shape[0])] * 7 for p in parts])
  means = torch.stack([p.mean(0) for p in parts])
  m2s = torch.stack([((p - p.mean(0)) ** 2).sum(0) for p in parts])
  total, mean, m2 = ops.merge_bn_statistics(counts, means, m2s)
  allx = torch.cat(parts)
  torch.testing.assert_close(mean, allx.mean(0), rtol=1e-5, atol=1e-6)
  torch.testing.assert_close(m2 / total, allx.var(0, unbiased=False), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('n,c,h,w,relu,res', [(4, 64, 17, 19, True, False), (2, 256, 9, 33, True, True),
                                              (3, 2048, 5, 7, True, True), (2, 128, 12, 12, False, False),
                                              (16, 512, 33, 33, True, True), (1, 4, 3, 3, True, True)])
def test_fused_bn_act_matches_framework_ops(n, c, h, w, relu, res):
  gen = torch.Generator().manual_seed(n * 1000 + c)
  x = (torch.randn(n, c, h, w, generator=gen) * 2.0 + 0.7).to(DEV).contiguous(memory_format=torch.channels_last)
  r = torch.randn(n, c, h, w, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last) if res else None
  up = torch.randn(n, c, h, w, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)

  def run(fused):
    bn = torch.nn.BatchNorm2d(c, momentum=3e-4).to(DEV)
    with torch.no_grad():
      bn.weight.copy_(torch.linspace(0.5, 1.5, c))
      bn.bias.copy_(torch.linspace(-0.3, 0.3, c))
    bn.train()
    xi = x.clone().requires_grad_(True)
    ri = r.clone().requires_grad_(True) if res else None
    if fused:
      assert ops.fused_bn_act_available(xi, bn)
      y = ops.batch_norm_act(xi, bn, relu=relu, residual=ri)
    else:
      y = bn(xi)
      if res:
        y = y + ri
      if relu:
        y = torch.relu(y)
    (y * up).sum().backward()
    return (y.detach(), xi.grad, ri.grad if res else None, bn.weight.grad, bn.bias.grad,
            bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))

  got, want = run(True), run(False)
  assert got[0].is_contiguous(memory_format=torch.channels_last)
  torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=1e-5)
  scale = want[1].abs().max().item()
  torch.testing.assert_close(got[1], want[1], rtol=1e-4, atol=1e-5 * max(1.0, scale))
  if res:
    torch.testing.assert_close(got[2], want[2], rtol=0, atol=0)
  for i in (3, 4):
    torch.testing.assert_close(got[i], want[i], rtol=1e-4, atol=1e-4 * max(1.0, want[i].abs().max().item()))
  torch.testing.assert_close(got[5], want[5], rtol=1e-5, atol=1e-7)
  torch.testing.assert_close(got[6], want[6], rtol=1e-5, atol=1e-7)
  assert got[7] == want[7] == 1


@pytest.mark.gpu
def test_fused_bn_falls_back_outside_its_domain():
  bn = torch.nn.BatchNorm2d(8).to(DEV)
  x = torch.randn(2, 8, 5, 5, device=DEV)                     # NCHW: framework ops
  assert not ops.fused_bn_act_available(x, bn)
  y = ops.batch_norm_act(x, bn)
  assert y.shape == x.shape and (y >= 0).all()
  bn.eval()                                                   # eval mode: running statistics
  xl = x.contiguous(memory_format=torch.channels_last)
  assert not ops.fused_bn_act_available(xl, bn)
  torch.testing.assert_close(ops.batch_norm_act(xl, bn, relu=False), bn(xl))


@pytest.mark.gpu
def test_large_mean_small_variance_is_stable():
  """Chunked statistics merged with Chan's formula: no E[x^2] - E[x]^2 cancellation."""
  gen = torch.Generator().manual_seed(1)
  x = (100.0 + 1e-2 * torch.randn(8, 16, 40, 40, generator=gen)).to(DEV).contiguous(memory_format=torch.channels_last)
  bn = torch.nn.BatchNorm2d(16).to(DEV).train()
  y = ops.batch_norm_act(x, bn, relu=False)
  ref = torch.nn.functional.batch_norm(x.double(), None, None, bn.weight.double(), bn.bias.double(), True, 0.1, bn.eps)
  assert (y.double() - ref).abs().max().item() < 5e-2       # fp32 input resolution at |x| ~ 100 is ~1e-5 / 1e-2
  var = x.double().var(dim=(0, 2, 3), unbiased=True)
  torch.testing.assert_close(bn.running_var.double(), 0.9 + 0.1 * var, rtol=5e-3, atol=0)


@pytest.mark.gpu
def test_two_call_and_single_call_forms_agree():
  """The split form (statistics -> finalisation -> apply, what SyncBatchNorm interleaves with its
  collectives) and the single-call form of the hl8-producing batch norm give the same tensors, bounds,
  masks and running statistics; the gathered-ranks finalisation with one rank equals the plain one."""
  from spml_amd import _ffi
  g = torch.Generator().manual_seed(9)
  n, c, h, w = 3, 256, 9, 11
  rows = n * h * w
  x = (torch.randn(n, c, h, w, generator=g) * 1.7 + 0.3).to(DEV).contiguous(memory_format=torch.channels_last)
  res = torch.randn(n, c, h, w, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
  gamma = torch.linspace(0.5, 1.5, c, device=DEV)
  beta = torch.linspace(-0.2, 0.2, c, device=DEV)
  resb = res.abs().max().reshape(1).clone()
  rm1, rv1 = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
  y1, yh1, b1, m1, saved1 = _ffi.bn_fwd_hl8(x, rows, c, res, resb, gamma, beta, rm1, rv1, 0.1, 1e-5, True, True, True,
                                            True)
  st = _ffi.bn_stats_ext(x, rows, c)
  rm2, rv2 = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
  invstd = _ffi.bn_finalize(st[1], st[2], rows, 1e-5, 0.1, rm2, rv2)
  y2, yh2, b2, m2 = _ffi.bn_act_apply_hl8(x, rows, c, res, resb, st[1], invstd, gamma, beta, st[3], st[4], True, True,
                                          True, want_mask=True)
  torch.testing.assert_close(y2, y1, rtol=1e-6, atol=1e-6)
  torch.testing.assert_close(b2, b1, rtol=1e-6, atol=0)
  assert torch.equal(m2, m1)
  assert (yh2.data != yh1.data).float().mean().item() < 1e-3           # last-bit differences at most
  torch.testing.assert_close(rm2, rm1, rtol=1e-6, atol=1e-7)
  torch.testing.assert_close(rv2, rv1, rtol=1e-6, atol=1e-7)
  rm3, rv3 = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
  mean3, invstd3, total3 = _ffi.bn_finalize_ranks(st[:3].unsqueeze(0).contiguous(), 1e-5, 0.1, rm3, rv3)
  torch.testing.assert_close(mean3, st[1], rtol=1e-6, atol=1e-7)
  torch.testing.assert_close(invstd3, invstd, rtol=1e-6, atol=1e-7)
  torch.testing.assert_close(rv3, rv2, rtol=1e-6, atol=1e-7)
  # against the framework
  bn = torch.nn.BatchNorm2d(c, momentum=0.1).to(DEV).train()
  with torch.no_grad():
    bn.weight.copy_(gamma)
    bn.bias.copy_(beta)
  want = torch.relu(bn(x) + res)
  torch.testing.assert_close(y1, want, rtol=1e-5, atol=1e-5)
  assert float(b1) >= float(want.abs().max()) * 0.9999
  assert float(total3) == float(rows)


def _unequal_ranks_worker(rank, port, x_all, r_all, up_all, out_q):
  import os
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  dist.init_process_group('gloo', rank=rank, world_size=2)
  try:
    lo, hi = (0, 1) if rank == 0 else (1, x_all.shape[0])
    c = x_all.shape[1]
    bn = torch.nn.SyncBatchNorm(c, momentum=0.1).to(DEV).train()
    with torch.no_grad():
      bn.weight.copy_(torch.linspace(0.5, 1.5, c))
      bn.bias.copy_(torch.linspace(-0.3, 0.3, c))
    cl = dict(memory_format=torch.channels_last)
    x = x_all[lo:hi].to(DEV).contiguous(**cl).requires_grad_(True)
    r = r_all[lo:hi].to(DEV).contiguous(**cl).requires_grad_(True)
    up = up_all[lo:hi].to(DEV).contiguous(**cl)
    assert ops.fused_bn_act_available(x, bn)
    y = ops.batch_norm_act(x, bn, relu=True, residual=r)
    (y * up).sum().backward()
    out_q.put((rank, 'ok', y.detach().cpu().numpy(), x.grad.cpu().numpy(), r.grad.cpu().numpy(),
               bn.weight.grad.cpu().numpy(), bn.bias.grad.cpu().numpy(), bn.running_var.cpu().numpy()))
  except Exception as e:       # noqa: BLE001 -- reported to the parent
    import traceback
    out_q.put((rank, traceback.format_exc() + repr(e)))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.gpu
def test_sync_batchnorm_with_unequal_rank_batches():
  """SyncBatchNorm through the fused kernels with 1 image on rank 0 and 3 on rank 1 (sharing this GPU
  over gloo) == one rank on the joint batch: the backward uses the SUM of the gathered row counts
  (lib/nn/sync_batchnorm/batchnorm.py:124-145), read on the device."""
  import socket
  import torch.multiprocessing as mp
  g = torch.Generator().manual_seed(12)
  n, c, h, w = 4, 64, 9, 7
  x_all = torch.randn(n, c, h, w, generator=g) * 1.5 + 0.4
  r_all = torch.randn(n, c, h, w, generator=g)
  up_all = torch.randn(n, c, h, w, generator=g)
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  sk = socket.socket()
  sk.bind(('127.0.0.1', 0))
  port = sk.getsockname()[1]
  sk.close()
  procs = [ctx.Process(target=_unequal_ranks_worker, args=(k, port, x_all, r_all, up_all, q)) for k in range(2)]
  for p in procs:
    p.start()
  got = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
  for p in procs:
    p.join(60)
  for t in got:
    assert t[1] == 'ok', t[1]
  T = torch.from_numpy
  bn = torch.nn.BatchNorm2d(c, momentum=0.1).to(DEV).train()
  with torch.no_grad():
    bn.weight.copy_(torch.linspace(0.5, 1.5, c))
    bn.bias.copy_(torch.linspace(-0.3, 0.3, c))
  x = x_all.to(DEV).requires_grad_(True)
  r = r_all.to(DEV).requires_grad_(True)
  y = torch.relu(bn(x) + r)
  (y * up_all.to(DEV)).sum().backward()
  torch.testing.assert_close(torch.cat([T(got[0][2]), T(got[1][2])]), y.detach().cpu(), rtol=1e-5, atol=1e-5)
  torch.testing.assert_close(torch.cat([T(got[0][3]), T(got[1][3])]), x.grad.cpu(), rtol=1e-4, atol=1e-5)
  torch.testing.assert_close(torch.cat([T(got[0][4]), T(got[1][4])]), r.grad.cpu(), rtol=1e-5, atol=1e-6)
  torch.testing.assert_close(T(got[0][5]) + T(got[1][5]), bn.weight.grad.cpu(), rtol=1e-4, atol=1e-4)
  torch.testing.assert_close(T(got[0][6]) + T(got[1][6]), bn.bias.grad.cpu(), rtol=1e-4, atol=1e-4)
  torch.testing.assert_close(T(got[0][7]), bn.running_var.cpu(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# Branch-by-branch cases of csrc/bn_act.hip against the float64 reference (tests/bn_act_ref.py).  Yardstick of every
# floating-point output: `lib`, the error of the framework's own fp32 op (F.batch_norm in training mode + autograd,
# torch.var_mean) against the same reference on the same inputs; a case asserts error <= max(4 * lib, floor) -- 4 is
# the margin this project gives another summation order of the same fp32 terms (test_kernel_branches_gpu.py).
# Floors: 2e-6 of the largest magnitude for per-element and per-channel values; sums are taken relative to sum |term|
# of their channel (test_conv_bn_bwd_stats_gpu.py) with the same 2e-6 -- 32 half-ulps, where the worst case of a
# chunked fp32 sum as deep as these (128 rows + 16 slots + 64 lanes) is ~200 of them.  Exact relations get no tolerance.
# `pytest -s` prints every figure; profiles/bn_branch_parity.md keeps one run of them.
import functools
import math

import torch.nn.functional as F

import bn_act_ref as ref
from spml_amd import _ffi

EPS, MOM = 1e-5, 0.1
FLOOR = 2e-6
FULL_DESTINATIONS = ((300, 40), (133, 264))            # the shapes that run every destination combination
_GEO = {(g[0], g[1]): g for g in ref.GEOMETRY}
_CASES = [(r, c, False) for r, c in ref.SHAPES] + [ref.OUTLIER_SHAPE + (True,)]
_CASES_F32 = _CASES + [(r, c, False) for r, c in ref.FP32_ONLY_SHAPES]


def _pin_chunks(r, c, chunks):
  """The case sits on its branch only while the library cuts (R, C) into this many statistics chunks."""
  assert _ffi.lib().spml_bn_workspace_bytes(r, c) == 16 * chunks * c + 256, 'bn_chunks(%d, %d) moved' % (r, c)


@functools.lru_cache(maxsize=None)
def _case(r, c, outlier=False, constant=False):
  t = {k: v.to(DEV) for k, v in ref.make_inputs(r, c, outlier=outlier, constant=constant).items()}
  t['resb'] = t['res'].abs().max().reshape(1).clone()
  return t


@functools.lru_cache(maxsize=None)
def _ref_fwd(r, c, outlier, relu, res):
  """The float64 forward of a case: computed once, shared, never written to."""
  t = _case(r, c, outlier)
  return ref.forward(t['x'], t['gamma'], t['beta'], EPS, MOM, relu, t['res'] if res else None,
                     torch.zeros(c, device=DEV), torch.ones(c, device=DEV))


def _rel(got, want):
  """Largest absolute error over the largest magnitude of the reference."""
  return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def _sum_rel(got, want, scale):
  """Largest error of a per-channel sum relative to sum |term| of its channel."""
  return float(((got.double() - want).abs() / scale.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def _lib(r, c, outlier, relu, res):
  """Errors of the framework's fp32 ops on the case's inputs against the float64 reference (the yardstick)."""
  t = _case(r, c, outlier)
  f = _ref_fwd(r, c, outlier, relu, res)
  x = t['x'].clone().requires_grad_(True)
  w = t['gamma'].clone().requires_grad_(True)
  b = t['beta'].clone().requires_grad_(True)
  rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
  y = F.batch_norm(x, rm, rv, w, b, True, MOM, EPS)
  if res:
    y = y + t['res']
  if relu:
    y = torch.relu(y)
  y.backward(t['dy'])
  bw = ref.backward(t['dy'], t['x'], f['mean'], f['invstd'], t['gamma'], (y.detach() > 0) if relu else None)
  var, mean = torch.var_mean(t['x'], 0, unbiased=False)
  return dict(y=_rel(y.detach(), f['y']), dx=_rel(x.grad, bw['dx']), s0=_sum_rel(b.grad, bw['s0'], bw['abs0']),
              s1=_sum_rel(w.grad, bw['s1'], bw['abs1']), mean=_rel(mean, f['mean']),
              m2=_sum_rel(var * r, f['m2'], f['m2']), invstd=_rel(1.0 / torch.sqrt(var + EPS), f['invstd']),
              running_mean=_rel(rm, f['running_mean']), running_var=_rel(rv, f['running_var']))


def _hold(entry, case, what, err, lib, floor=FLOOR):
  bound = max(4.0 * lib, floor)
  print('bn-parity | %s | %s | %s | %.3e | %.3e | %.3e%s' % (entry, case, what, err, lib, bound,
                                                          ' (floor)' if bound == floor else ''))
  assert err <= bound, '%s %s %s: error %.3e above max(4 x %.3e, %.1e)' % (entry, case, what, err, lib, floor)


def _bits(t):
  return t.contiguous().view(torch.int32)


def _same(a, b):
  """Bit-identical tensors (or tuples of them; Hl8 by data and bound)."""
  if a is None or b is None:
    return a is None and b is None
  if isinstance(a, (tuple, list)):
    return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
  if isinstance(a, _ffi.Hl8):
    return torch.equal(a.data, b.data) and _same(a.bound, b.bound)
  return torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)


def _check_hl8(hl8, v32, entry, case):
  """The split-f16 output decoded against the fp32 output of the same arithmetic: the format's width, 2^-22 |v| (two
  11-bit significands) + 2^-25 / S (half the f16 subnormal step of the scaled value) -- derived, not measured."""
  halves = ref.hl8_halves(hl8)
  assert bool(torch.isfinite(halves).all()), '%s %s: non-finite half' % (entry, case)
  s = ref.pow2_scale(hl8.bound.item())
  v = v32.double().reshape(hl8.rows, hl8.channels)
  err = (ref.decode_hl8(hl8) - v).abs()
  tol = 2.0 ** -22 * v.abs() + 2.0 ** -25 / s
  print('bn-parity | %s | %s | hl8 | %.3f of the format bound | - | 1' % (entry, case, float((err / tol).max())))
  assert bool((err <= tol).all()), '%s %s: hl8 decode off the fp32 output' % (entry, case)


def _check_bound(bound, truth, formula, entry, case):
  """Sound (>= max |float64 output|) and the formula (<= formula x 1.0002 + 4 ulp: 1.0001 is the kernel's own slack,
  the rest the fp32 rounding of its ~6 operations), the formula in float64 from the kernel's own returned statistics."""
  b = float(bound)
  assert math.isfinite(b) and b > 0.0
  ulp = 2.0 ** (math.frexp(b)[1] - 24)
  print('bn-parity | %s | %s | bound | %.6e | max %.6e | formula %.6e' % (entry, case, b, truth, formula))
  assert b >= truth, '%s %s: bound %.6e below max |output| %.6e' % (entry, case, b, truth)
  assert b <= formula * 1.0002 + 4.0 * ulp, '%s %s: bound %.6e looser than its formula %.6e' % (entry, case, b, formula)


def _dres_exact(dres, dy, mask, entry, case):
  """d_residual = dy where the mask bit is set and +0 elsewhere, bit for bit."""
  want = torch.where(mask, dy, torch.zeros_like(dy))
  assert torch.equal(_bits(dres), _bits(want)), '%s %s: d_residual' % (entry, case)


def _name(r, c, outlier=False):
  return '(%d, %d)%s' % (r, c, ' outlier' if outlier else '')


@pytest.mark.gpu
@pytest.mark.parametrize('r,c,outlier', _CASES_F32)
def test_fp32_entries_against_float64(r, c, outlier):
  """bn_partial<0, 0> / bn_partial<1, 0|1> / bn_merge<0|1> (register path) / bn_apply<false|true> /
  bn_bwd_apply<0|1> without hl8 destinations, through bn_stats, bn_act_fwd, bn_act_apply, bn_act_bwd_reduce,
  bn_act_bwd_apply and bn_act_bwd; the row of GEOMETRY says which guards, lanes and ragged tiles the shape reaches
  (the fp32-only shapes: C & 3 only -- one quad, and three quads of the four of a block)."""
  geo = ref.host_geometry(r, c)
  assert (r, c) not in _GEO or _GEO[(r, c)] == geo
  _pin_chunks(r, c, geo[6])
  t, case = _case(r, c, outlier), _name(r, c, outlier)
  x, dy, gamma, beta = t['x'], t['dy'], t['gamma'], t['beta']
  mean, m2 = _ffi.bn_stats(x)                                  # bn_partial<0, 0> without extremes, bn_merge<0> fin = 0
  assert _same(_ffi.bn_stats(x), (mean, m2))
  f0, lib0 = _ref_fwd(r, c, outlier, False, False), _lib(r, c, outlier, False, False)
  _hold('bn_stats', case, 'mean', _rel(mean, f0['mean']), lib0['mean'])
  _hold('bn_stats', case, 'M2', _sum_rel(m2, f0['m2'], f0['m2']), lib0['m2'])
  for relu in (False, True):
    for res in (False, True):
      sub = '%s relu=%d res=%d' % (case, relu, res)
      f, lib = _ref_fwd(r, c, outlier, relu, res), _lib(r, c, outlier, relu, res)
      rs = t['res'] if res else None

      def fwd():
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        return _ffi.bn_act_fwd(x, rs, gamma, beta, rm, rv, MOM, EPS, relu) + (rm, rv)
      y, mean1, invstd1, rm, rv = fwd()                        # bn_merge<0> fin = 1 without a bound, bn_apply<res>
      assert _same(fwd(), (y, mean1, invstd1, rm, rv))
      assert _same(mean1, mean)
      _hold('bn_act_fwd', sub, 'y', _rel(y, f['y']), lib['y'])
      _hold('bn_act_fwd', sub, 'invstd', _rel(invstd1, f['invstd']), lib['invstd'])
      _hold('bn_act_fwd', sub, 'running mean', _rel(rm, f['running_mean']), lib['running_mean'])
      _hold('bn_act_fwd', sub, 'running var', _rel(rv, f['running_var']), lib['running_var'])
      assert _same(_ffi.bn_act_apply(x, rs, mean1, invstd1, gamma, beta, relu), y)       # the split form: same kernel
      mask = (y > 0) if relu else None
      yk = y if relu else None                                 # MASK 1 (fp32 y) / MASK 0
      bw = ref.backward(dy, x, f['mean'], f['invstd'], gamma, mask)
      s0, s1 = _ffi.bn_act_bwd_reduce(dy, yk, x, mean1, invstd1)
      assert _same(_ffi.bn_act_bwd_reduce(dy, yk, x, mean1, invstd1), (s0, s1))
      _hold('bn_act_bwd_reduce', sub, 'sum dz', _sum_rel(s0, bw['s0'], bw['abs0']), lib['s0'])
      _hold('bn_act_bwd_reduce', sub, 'sum dz xhat', _sum_rel(s1, bw['s1'], bw['abs1']), lib['s1'])
      dx, dres = _ffi.bn_act_bwd_apply(dy, yk, x, mean1, invstd1, gamma, s0, s1, r, True, res)
      assert _same(_ffi.bn_act_bwd_apply(dy, yk, x, mean1, invstd1, gamma, s0, s1, r, True, res), (dx, dres))
      _hold('bn_act_bwd_apply', sub, 'dx', _rel(dx, bw['dx']), lib['dx'])
      count = torch.full((1,), float(r), device=DEV)           # the device-side row count
      dxc, _ = _ffi.bn_act_bwd_apply(dy, yk, x, mean1, invstd1, gamma, s0, s1, count, True, False)
      _hold('bn_act_bwd_apply', sub, 'dx (device count)', _rel(dxc, bw['dx']), lib['dx'])
      one = _ffi.bn_act_bwd(dy, yk, x, mean1, invstd1, gamma, True, res)       # (dx, dres, d_gamma, d_beta)
      assert _same(one, (dx, dres, s1, s0))
      if res:
        full = mask if relu else torch.ones_like(dy, dtype=torch.bool)
        _dres_exact(dres, dy, full, 'bn_act_bwd_apply', sub)
        only = _ffi.bn_act_bwd_apply(dy, yk, None, None, None, None, None, None, r, False, True)
        assert only[0] is None and _same(only[1], dres)


def _forward_checks(entry, sub, out, f, lib, t, r, c, res, relu, base):
  """out = (y|None, Hl8|None, bound, mask|None, (mean, invstd, cmax, cmin)) of one hl8-producing forward call; base =
  the same call with every destination on (None: this one)."""
  y, yh, bound, mask, saved = out
  y_ref = y if y is not None else base[0]
  if y is not None:
    _hold(entry, sub, 'y', _rel(y, f['y']), lib['y'])
  if base is not None and y is not None:
    assert _same(y, base[0])
  if mask is not None:                                         # exact: the mask of the fp32 y of the same arithmetic
    assert torch.equal(ref.mask_bits(mask, r, c), y_ref > 0), '%s %s: mask bytes' % (entry, sub)
  if yh is not None:
    _check_hl8(yh, y_ref, entry, sub)
  mean, invstd, cmax, cmin = saved
  assert torch.equal(cmax, t['x'].max(0).values) and torch.equal(cmin, t['x'].min(0).values)
  formula = ref.bound_fwd(mean, invstd, t['gamma'], t['beta'], cmax, cmin, float(t['resb']) if res else 0.0)
  _check_bound(bound, float(f['y'].abs().max()), formula, entry, sub)


@pytest.mark.gpu
@pytest.mark.parametrize('r,c,outlier', _CASES)
def test_hl8_forward_entries_against_float64(r, c, outlier):
  """bn_partial<0, 0> with extremes (and the bound reset), bn_merge<0> with extremes / fin / publish_bound,
  bn_bound_fwd, bn_finalize, bn_apply<false|true> with the fp32 / hl8 / mask destinations each on and off
  (store_hl8_quad's lane pairs: GEOMETRY's partial column blocks have dead pairs beside live ones), through
  bn_stats_ext + bn_finalize + bn_act_apply_hl8 and through bn_fwd_hl8."""
  geo = _GEO[(r, c)]
  assert ref.host_geometry(r, c) == geo
  _pin_chunks(r, c, geo[6])
  t, case = _case(r, c, outlier), _name(r, c, outlier)
  x, gamma, beta = t['x'], t['gamma'], t['beta']
  st = _ffi.bn_stats_ext(x, r, c)
  assert _same(_ffi.bn_stats_ext(x, r, c), st)
  f0, lib0 = _ref_fwd(r, c, outlier, False, False), _lib(r, c, outlier, False, False)
  assert bool((st[0] == float(r)).all())
  _hold('bn_stats_ext', case, 'mean', _rel(st[1], f0['mean']), lib0['mean'])
  _hold('bn_stats_ext', case, 'M2', _sum_rel(st[2], f0['m2'], f0['m2']), lib0['m2'])
  assert torch.equal(st[3], x.max(0).values) and torch.equal(st[4], x.min(0).values)       # exact: fp32 max / min
  if (r, c) in FULL_DESTINATIONS and not outlier:
    combos = [(a, b, m, s, True) for s in (True, False) for a in (True, False) for b in (True, False)
              for m in (True, False) if a or b]
  else:
    combos = [(True, True, True, True, True), (True, True, True, False, True)]
  combos.append((True, True, False, False, False))             # relu off
  bases = {}
  for want_f32, want_hl8, want_mask, res, relu in combos:      # (every destination on comes first for each res)
    sub = '%s f32=%d hl8=%d mask=%d res=%d relu=%d' % (case, want_f32, want_hl8, want_mask, res, relu)
    f, lib = _ref_fwd(r, c, outlier, relu, res), _lib(r, c, outlier, relu, res)
    rs, rb = (t['res'], t['resb']) if res else (None, None)

    def single():
      rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
      o = _ffi.bn_fwd_hl8(x, r, c, rs, rb, gamma, beta, rm, rv, MOM, EPS, relu, want_f32, want_hl8, want_mask)
      return o[:4] + (tuple(o[4]), rm, rv)
    out = single()
    assert _same(single(), out)
    base = bases.get((res, relu))
    _forward_checks('bn_fwd_hl8', sub, out[:5], f, lib, t, r, c, res, relu, base)
    _hold('bn_fwd_hl8', sub, 'invstd', _rel(out[4][1], f['invstd']), lib['invstd'])
    _hold('bn_fwd_hl8', sub, 'running var', _rel(out[6], f['running_var']), lib['running_var'])
    _hold('bn_fwd_hl8', sub, 'running mean', _rel(out[5], f['running_mean']), lib['running_mean'])
    if base is None:
      assert want_f32 and want_hl8 and (want_mask or not relu)
      bases[(res, relu)] = base = out
    else:                                                      # a destination switched off changes none of the others
      assert _same(out[4:], base[4:]) and _same(out[2], base[2])
      assert want_mask is False or _same(out[3], base[3])
      assert want_hl8 is False or _same(out[1], base[1])
    # the split form: statistics -> finalisation -> bound + apply
    rm2, rv2 = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    invstd = _ffi.bn_finalize(st[1], st[2], r, EPS, MOM, rm2, rv2)
    sp = _ffi.bn_act_apply_hl8(x, r, c, rs, rb, st[1], invstd, gamma, beta, st[3], st[4], relu, want_f32, want_hl8,
                               want_mask=want_mask)
    assert _same(_ffi.bn_act_apply_hl8(x, r, c, rs, rb, st[1], invstd, gamma, beta, st[3], st[4], relu, want_f32,
                                       want_hl8, want_mask=want_mask), sp)
    _forward_checks('bn_act_apply_hl8', sub, sp + ((st[1], invstd, st[3], st[4]),), f, lib, t, r, c, res, relu,
                    None if want_f32 else (base[0],))
    # single-call and split forms agree (the tolerances of test_two_call_and_single_call_forms_agree)
    if want_f32:
      torch.testing.assert_close(sp[0], out[0], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(sp[2], out[2], rtol=1e-6, atol=0)
    if want_mask:
      assert torch.equal(sp[3], out[3])
    torch.testing.assert_close(invstd, out[4][1], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(rm2, out[5], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(rv2, out[6], rtol=1e-6, atol=1e-7)


def _backward_formula(saved, gamma, st, n):
  return ref.bound_bwd(saved[0], saved[1], gamma, saved[2], saved[3], st[0], st[1], st[2], float(n))


@pytest.mark.gpu
@pytest.mark.parametrize('r,c,outlier', _CASES)
def test_hl8_backward_entries_against_float64(r, c, outlier):
  """bn_partial<1, 0|1|2> with max |dz| (and the bound reset), bn_merge<1> with and without publish_bound,
  bn_bound_bwd with a host and a device count, bn_bwd_apply<0|1|2> with the fp32 / hl8 / d_residual destinations each
  on and off, through bn_act_bwd_reduce_ext + bn_act_bwd_apply_hl8 and through bn_bwd_hl8.  MASK 1 reads the fp32 y,
  MASK 2 the mask bytes of the same forward call, MASK 0 nothing (a forward without ReLU)."""
  geo = _GEO[(r, c)]
  _pin_chunks(r, c, geo[6])
  t, case = _case(r, c, outlier), _name(r, c, outlier)
  x, dy, gamma, beta = t['x'], t['dy'], t['gamma'], t['beta']
  for relu in (True, False):
    f, lib = _ref_fwd(r, c, outlier, relu, True), _lib(r, c, outlier, relu, True)
    y, _, _, mbytes, saved = _ffi.bn_fwd_hl8(x, r, c, t['res'], t['resb'], gamma, beta, None, None, MOM, EPS, relu, True,
                                             True, relu)
    mean, invstd, cmax, cmin = saved
    mask = (y > 0) if relu else torch.ones_like(dy, dtype=torch.bool)
    bw = ref.backward(dy, x, f['mean'], f['invstd'], gamma, mask if relu else None)
    dz32 = torch.where(mask, dy, torch.zeros_like(dy))
    forms = (('MASK 1', y, None), ('MASK 2', None, mbytes)) if relu else (('MASK 0', None, None),)
    got = {}
    for form, yk, mk in forms:
      sub = '%s %s' % (case, form)
      st = _ffi.bn_act_bwd_reduce_ext(dy, yk, mk, x, r, c, mean, invstd)
      assert _same(_ffi.bn_act_bwd_reduce_ext(dy, yk, mk, x, r, c, mean, invstd), st)
      _hold('bn_act_bwd_reduce_ext', sub, 'sum dz', _sum_rel(st[0], bw['s0'], bw['abs0']), lib['s0'])
      _hold('bn_act_bwd_reduce_ext', sub, 'sum dz xhat', _sum_rel(st[1], bw['s1'], bw['abs1']), lib['s1'])
      assert torch.equal(st[2], dz32.abs().max(0).values), '%s: max |dz|' % sub            # exact: an fp32 maximum
      formula = _backward_formula(saved, gamma, st, r)
      truth = float(bw['dx'].abs().max())
      dests = [(True, True, True)]
      if form != 'MASK 1':
        dests += [(a, b, d) for a in (True, False) for b in (True, False) for d in (True, False)
                  if (a or b or d) and not (a and b and d)]
      first = None
      for want_f32, want_hl8, want_dres in dests:
        ssub = '%s dx=%d hl8=%d dres=%d' % (sub, want_f32, want_hl8, want_dres)

        def apply(count):
          return _ffi.bn_act_bwd_apply_hl8(dy, yk, mk, x, r, c, mean, invstd, gamma, st[0], st[1], st[2], cmax, cmin,
                                           count, want_f32, want_hl8, want_dres)
        dx, dxh, dres = apply(r)
        assert _same(apply(r), (dx, dxh, dres))
        if first is None:
          first = (dx, dxh, dres)
          _hold('bn_act_bwd_apply_hl8', ssub, 'dx', _rel(dx, bw['dx']), lib['dx'])
          dev = apply(torch.full((1,), float(r), device=DEV))                # bn_bound_bwd / bn_bwd_apply: count_dev
          _hold('bn_act_bwd_apply_hl8', ssub, 'dx (device count)', _rel(dev[0], bw['dx']), lib['dx'])
          _check_hl8(dev[1], dev[0], 'bn_act_bwd_apply_hl8 (device count)', ssub)
          _check_bound(dev[1].bound, truth, formula, 'bn_act_bwd_apply_hl8 (device count)', ssub)
          assert _same(dev[2], dres)
        else:                                                  # a destination switched off changes none of the others
          assert want_f32 is False or _same(dx, first[0])
          assert want_hl8 is False or _same(dxh, first[1])
          assert want_dres is False or _same(dres, first[2])
        if want_hl8:
          _check_hl8(dxh, first[0], 'bn_act_bwd_apply_hl8', ssub)
          _check_bound(dxh.bound, truth, formula, 'bn_act_bwd_apply_hl8', ssub)
        if want_dres:
          _dres_exact(dres, dy, mask, 'bn_act_bwd_apply_hl8', ssub)
      got[form] = (st, first)
      if form != 'MASK 1':                                     # the single-call form (the wrapper has no fp32 y input)
        for want_dres in (True, False):
          ssub = '%s dres=%d' % (sub, want_dres)
          one = _ffi.bn_bwd_hl8(dy, mk, x, r, c, saved, gamma, want_dres)        # (dx Hl8, dres, d_gamma, d_beta)
          assert _same(_ffi.bn_bwd_hl8(dy, mk, x, r, c, saved, gamma, want_dres), one)
          assert _same(one[2], st[1]) and _same(one[3], st[0])                  # same kernels, same order
          _check_hl8(one[0], first[0], 'bn_bwd_hl8', ssub)
          _check_bound(one[0].bound, truth, formula, 'bn_bwd_hl8', ssub)         # publish_bound of bn_merge<1>
          assert _same(one[1], first[2] if want_dres else None)
    if relu:                                                   # MASK 1 and MASK 2 of the same y: bit-identical
      assert _same(got['MASK 1'], got['MASK 2'])


@pytest.mark.gpu
@pytest.mark.parametrize('r,c', FULL_DESTINATIONS)
def test_backward_calls_without_a_destination(r, c):
  """The two early returns of the host side: spml_bn_act_bwd_f32 and spml_bn_bwd_hl8_f32 asked for no dx, no hl8 copy
  and no d_residual stop after the reduction (no apply launch; the hl8 form without the bound reset and publish_bound)
  and still deliver d_gamma / d_beta, bit-identical to the sums of the reduce entries.  The hl8 wrapper always asks
  for the hl8 dx, so that call goes to the C ABI."""
  from ctypes import c_void_p
  t, case = _case(r, c), _name(r, c)
  x, dy, gamma, beta = t['x'], t['dy'], t['gamma'], t['beta']
  f, lib = _ref_fwd(r, c, False, True, True), _lib(r, c, False, True, True)
  y, _, _, mbytes, saved = _ffi.bn_fwd_hl8(x, r, c, t['res'], t['resb'], gamma, beta, None, None, MOM, EPS, True, True,
                                           False, True)
  mean, invstd, cmax, cmin = saved
  bw = ref.backward(dy, x, f['mean'], f['invstd'], gamma, y > 0)
  s0, s1 = _ffi.bn_act_bwd_reduce(dy, y, x, mean, invstd)
  none = _ffi.bn_act_bwd(dy, y, x, mean, invstd, gamma, False, False)          # (dx, dres, d_gamma, d_beta)
  assert none[0] is None and none[1] is None and _same(none[2:], (s1, s0))
  _hold('bn_act_bwd (no destination)', case, 'd_beta', _sum_rel(none[3], bw['s0'], bw['abs0']), lib['s0'])
  _hold('bn_act_bwd (no destination)', case, 'd_gamma', _sum_rel(none[2], bw['s1'], bw['abs1']), lib['s1'])
  st = _ffi.bn_act_bwd_reduce_ext(dy, None, mbytes, x, r, c, mean, invstd)
  dgb = torch.full((2, c), float('nan'), device=DEV)
  ws = _ffi._bn_workspace(r, c, dy.device)
  dp, null = _ffi._dp, c_void_p(0)
  _ffi.check(_ffi.lib().spml_bn_bwd_hl8_f32(
      dp(dy), null, dp(mbytes), dp(x), r, c, dp(mean), dp(invstd), dp(gamma), dp(cmax), dp(cmin), dp(dgb[0]),
      dp(dgb[1]), null, null, null, null, _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr()), 'spml_bn_bwd_hl8_f32')
  assert _same((dgb[1], dgb[0]), (st[0], st[1]))
  _hold('bn_bwd_hl8 (no destination)', case, 'd_beta', _sum_rel(dgb[1], bw['s0'], bw['abs0']), lib['s0'])
  _hold('bn_bwd_hl8 (no destination)', case, 'd_gamma', _sum_rel(dgb[0], bw['s1'], bw['abs1']), lib['s1'])


@pytest.mark.gpu
def test_finalize_ranks_pools_three_unequal_ranks():
  """bn_finalize_ranks with world = 3 and 50 / 31 / 64 rows of one tensor (the statistics of bn_stats_ext per rank),
  momentum and running statistics, against the float64 statistics of the whole tensor; then one rank's backward apply
  with the pooled device-side count (bn_bound_bwd / bn_bwd_apply<2> reading count_dev; the host count is 0 there)."""
  r, c, cuts = 145, 40, ((0, 50), (50, 81), (81, 145))
  t, case = _case(r, c), _name(r, c)
  x, dy, gamma, beta = t['x'], t['dy'], t['gamma'], t['beta']
  f, lib = _ref_fwd(r, c, False, True, False), _lib(r, c, False, True, False)
  parts = [x[a:b].clone() for a, b in cuts]
  gathered = torch.stack([_ffi.bn_stats_ext(p, p.shape[0], c)[:3] for p in parts]).contiguous()
  ext = torch.stack([_ffi.bn_stats_ext(p, p.shape[0], c)[3:] for p in parts])
  cmax, cmin = ext[:, 0].max(0).values.contiguous(), ext[:, 1].min(0).values.contiguous()

  def pool():
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    mean, invstd, total = _ffi.bn_finalize_ranks(gathered, EPS, MOM, rm, rv)
    return mean.clone(), invstd.clone(), total.clone(), rm, rv
  mean, invstd, total, rm, rv = pool()
  assert _same(pool(), (mean, invstd, total, rm, rv))
  assert float(total) == float(r)
  _hold('bn_finalize_ranks', case, 'mean', _rel(mean, f['mean']), lib['mean'])
  _hold('bn_finalize_ranks', case, 'invstd', _rel(invstd, f['invstd']), lib['invstd'])
  _hold('bn_finalize_ranks', case, 'running mean', _rel(rm, f['running_mean']), lib['running_mean'])
  _hold('bn_finalize_ranks', case, 'running var', _rel(rv, f['running_var']), lib['running_var'])
  # every rank's forward with the pooled statistics, its local sums, their total, and rank 0's apply
  outs = [_ffi.bn_act_apply_hl8(p, p.shape[0], c, None, None, mean, invstd, gamma, beta, cmax, cmin, True, True, True,
                                want_mask=True) for p in parts]
  y = torch.cat([o[0] for o in outs])
  _hold('bn_finalize_ranks', case, 'y', _rel(y, f['y']), lib['y'])
  bw = ref.backward(dy, x, f['mean'], f['invstd'], gamma, y > 0)
  sums = [_ffi.bn_act_bwd_reduce_ext(dy[a:b].clone(), None, o[3], p, p.shape[0], c, mean, invstd)
          for (a, b), o, p in zip(cuts, outs, parts)]
  st = torch.stack([sum(s[0] for s in sums), sum(s[1] for s in sums), torch.stack([s[2] for s in sums]).max(0).values])
  _hold('bn_finalize_ranks', case, 'sum dz', _sum_rel(st[0], bw['s0'], bw['abs0']), lib['s0'])
  _hold('bn_finalize_ranks', case, 'sum dz xhat', _sum_rel(st[1], bw['s1'], bw['abs1']), lib['s1'])
  a, b = cuts[0]
  dx, dxh, _ = _ffi.bn_act_bwd_apply_hl8(dy[a:b].clone(), None, outs[0][3], parts[0], b - a, c, mean, invstd, gamma,
                                         st[0], st[1], st[2], cmax, cmin, total, True, True, False)
  err = float((dx.double() - bw['dx'][a:b]).abs().max()) / float(bw['dx'].abs().max())
  _hold('bn_finalize_ranks', case, 'dx of rank 0 (device count)', err, lib['dx'])
  _check_hl8(dxh, dx, 'bn_finalize_ranks', case)
  _check_bound(dxh.bound, float(bw['dx'].abs().max()), _backward_formula((mean, invstd, cmax, cmin), gamma, st, r),
               'bn_finalize_ranks', case)


_POOLED = [(8, n) for n in (1, 64, 65, 1024, 1025, 4096)] + [(264, 1024), (264, 1025)]


@pytest.mark.gpu
@pytest.mark.parametrize('c,chunks', _POOLED)
def test_chunk_pooled_entries_against_float64(c, chunks):
  """The four `_chunks` entries fed the reference's chunk statistics (cast to fp32; 32-row chunks, a 5-row last one)
  instead of a convolution's: bn_merge<0|1> alone.  1 / 64 / 65 chunks: one lane slot, a full one, the second;
  1024: the last count of the register path; 1025 and 4096 (the layout's limit): the three streamed loops.
  Yardstick: the framework's op on the whole tensor (the pooled entry sees one more rounding per chunk value)."""
  rows = 32
  r = rows * (chunks - 1) + 5
  t, case = _case(r, c), '%s in %d chunks' % (_name(r, c), chunks)
  x, dy, gamma, beta = t['x'], t['dy'], t['gamma'], t['beta']
  f, lib = _ref_fwd(r, c, False, True, True), _lib(r, c, False, True, True)
  data = ref.chunk_stats_fwd(x, rows).float().contiguous()
  assert data.shape == (4, chunks, c)

  def stats():
    return _ffi.ChunkStats(data, chunks, rows, torch.zeros(1, device=DEV))     # the producer reset the bound slot
  st = _ffi.bn_stats_ext(x, r, c, chunk_stats=stats())
  assert _same(_ffi.bn_stats_ext(x, r, c, chunk_stats=stats()), st)
  _hold('bn_stats_ext(chunks)', case, 'mean', _rel(st[1], f['mean']), lib['mean'])
  _hold('bn_stats_ext(chunks)', case, 'M2', _sum_rel(st[2], f['m2'], f['m2']), lib['m2'])
  assert torch.equal(st[3], x.max(0).values) and torch.equal(st[4], x.min(0).values)

  def fwd():
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    o = _ffi.bn_fwd_hl8(x, r, c, t['res'], t['resb'], gamma, beta, rm, rv, MOM, EPS, True, True, True, True,
                        chunk_stats=stats())
    return o[:4] + (tuple(o[4]), rm, rv)
  out = fwd()
  assert _same(fwd(), out)
  _forward_checks('bn_fwd_hl8(chunks)', case, out[:5], f, lib, t, r, c, True, True, None)
  _hold('bn_fwd_hl8(chunks)', case, 'invstd', _rel(out[4][1], f['invstd']), lib['invstd'])
  _hold('bn_fwd_hl8(chunks)', case, 'running mean', _rel(out[5], f['running_mean']), lib['running_mean'])
  _hold('bn_fwd_hl8(chunks)', case, 'running var', _rel(out[6], f['running_var']), lib['running_var'])
  y, _, _, mbytes, saved = out[:5]
  mask = y > 0
  bw = ref.backward(dy, x, f['mean'], f['invstd'], gamma, mask)
  bdata = ref.chunk_stats_bwd(bw['dz'], x, f['mean'], rows).float().contiguous()
  assert bdata.shape == (3, chunks, c)

  def bstats():
    return _ffi.ChunkStats(bdata, chunks, rows, torch.zeros(1, device=DEV))
  sb = _ffi.bn_act_bwd_reduce_ext(dy, None, mbytes, x, r, c, saved[0], saved[1], chunk_stats=bstats())
  assert _same(_ffi.bn_act_bwd_reduce_ext(dy, None, mbytes, x, r, c, saved[0], saved[1], chunk_stats=bstats()), sb)
  _hold('bn_act_bwd_reduce_ext(chunks)', case, 'sum dz', _sum_rel(sb[0], bw['s0'], bw['abs0']), lib['s0'])
  _hold('bn_act_bwd_reduce_ext(chunks)', case, 'sum dz xhat', _sum_rel(sb[1], bw['s1'], bw['abs1']), lib['s1'])
  assert torch.equal(sb[2], bw['dz'].float().abs().max(0).values)
  one = _ffi.bn_bwd_hl8(dy, mbytes, x, r, c, saved, gamma, True, chunk_stats=bstats())     # (dx Hl8, dres, d_gamma, d_beta)
  assert _same(_ffi.bn_bwd_hl8(dy, mbytes, x, r, c, saved, gamma, True, chunk_stats=bstats()), one)
  assert _same(one[2], sb[1]) and _same(one[3], sb[0])
  # the fp32 dx of the same arithmetic: the apply kernel alone with the pooled sums
  dx, _, _ = _ffi.bn_act_bwd_apply_hl8(dy, None, mbytes, x, r, c, saved[0], saved[1], gamma, sb[0], sb[1], sb[2],
                                       saved[2], saved[3], r, True, False, False)
  _hold('bn_bwd_hl8(chunks)', case, 'dx', _rel(dx, bw['dx']), lib['dx'])
  _check_hl8(one[0], dx, 'bn_bwd_hl8(chunks)', case)
  _check_bound(one[0].bound, float(bw['dx'].abs().max()), _backward_formula(saved, gamma, sb, r), 'bn_bwd_hl8(chunks)',
               case)
  _dres_exact(one[1], dy, mask, 'bn_bwd_hl8(chunks)', case)


@pytest.mark.gpu
def test_chunk_pooled_statistics_with_six_channels():
  """spml_bn_stats_ext_chunks_f32 does not ask for C % 4 == 0: the last bn_merge<0> block has two live channels."""
  r, c, rows = 69, 6, 32
  x = _case(r, 8)['x'][:, :c].contiguous()
  xd = x.double()
  data = ref.chunk_stats_fwd(x, rows).float().contiguous()
  st = _ffi.bn_stats_ext(x, r, c, chunk_stats=_ffi.ChunkStats(data, 3, rows, torch.zeros(1, device=DEV)))
  var, mean = torch.var_mean(x, 0, unbiased=False)
  want_mean, want_m2 = xd.mean(0), ((xd - xd.mean(0)) ** 2).sum(0)
  _hold('bn_stats_ext(chunks)', '(69, 6) in 3 chunks', 'mean', _rel(st[1], want_mean), _rel(mean, want_mean))
  _hold('bn_stats_ext(chunks)', '(69, 6) in 3 chunks', 'M2', _sum_rel(st[2], want_m2, want_m2),
        _sum_rel(var * r, want_m2, want_m2))
  assert torch.equal(st[3], x.max(0).values) and torch.equal(st[4], x.min(0).values)


@pytest.mark.gpu
def test_one_row_at_the_c_abi():
  """R = 1 (ops.batch_norm_act refuses it; the C ABI does not): M2 = 0, invstd = 1 / sqrt(eps), y = beta (+ residual),
  the running variance takes the divisor 1, dx = 0."""
  r, c = 1, 8
  t = _case(r, c)
  x, dy, gamma, beta, res = t['x'], t['dy'], t['gamma'], t['beta'], t['res']
  f = ref.forward(x, gamma, beta, EPS, 0.25, False, res, torch.zeros(c, device=DEV), torch.ones(c, device=DEV))
  is_want = torch.full((c,), EPS, device=DEV).double().rsqrt()
  mean, m2 = _ffi.bn_stats(x)
  assert _same(mean, x[0]) and bool((m2 == 0).all())
  st = _ffi.bn_stats_ext(x, r, c)
  assert _same(st[1], x[0]) and bool((st[2] == 0).all()) and _same(st[3], x[0]) and _same(st[4], x[0])
  rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
  y, mean1, invstd1 = _ffi.bn_act_fwd(x, res, gamma, beta, rm, rv, 0.25, EPS, False)
  assert _same(mean1, x[0]) and _same(y, (beta + res[0]).view(1, c))
  assert _rel(invstd1, is_want) <= 2.0 ** -22 and _rel(rv, f['running_var']) <= 2.0 ** -22
  assert _rel(rm, f['running_mean']) <= 2.0 ** -22
  torch.testing.assert_close(rv, torch.full((c,), 0.75, device=DEV), rtol=1e-6, atol=0)
  rm2, rv2 = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
  y2, yh, bound, mbytes, saved = _ffi.bn_fwd_hl8(x, r, c, res, t['resb'], gamma, beta, rm2, rv2, 0.25, EPS, True, True,
                                                 True, True)
  assert _same(y2, torch.relu(y)) and _same((rm2, rv2), (rm, rv)) and _same(saved[1], invstd1)
  assert torch.equal(ref.mask_bits(mbytes, r, c), y2 > 0)
  _check_hl8(yh, y2, 'bn_fwd_hl8', '(1, 8)')
  assert float(bound) >= float(y2.abs().max())
  dx, dres, dg, db = _ffi.bn_act_bwd(dy, y2, x, mean1, invstd1, gamma, True, True)
  assert bool((dx == 0).all()) and bool((dg == 0).all())
  _dres_exact(dres, dy, y2 > 0, 'bn_act_bwd', '(1, 8)')
  assert _same(db, dres[0])
  one = _ffi.bn_bwd_hl8(dy, mbytes, x, r, c, saved, gamma, True)
  assert bool(torch.isfinite(ref.hl8_halves(one[0])).all()) and bool((ref.decode_hl8(one[0]) == 0).all())
  assert _same(one[1], dres) and math.isfinite(float(one[0].bound))


@pytest.mark.gpu
def test_constant_channels_stay_finite():
  """One value per channel at (300, 40): M2 exactly 0, invstd = 1 / sqrt(eps), y = beta (+ residual), and nothing
  non-finite in any output of the forward and backward entries, hl8 halves and bounds included."""
  r, c = 300, 40
  _pin_chunks(r, c, 3)
  t = _case(r, c, False, True)
  x, dy, gamma, beta, res = t['x'], t['dy'], t['gamma'], t['beta'], t['res']
  mean, m2 = _ffi.bn_stats(x)
  st = _ffi.bn_stats_ext(x, r, c)
  print('bn-parity | constant (300, 40) | largest M2 %.3e, mean off by %.3e' %
        (float(m2.max()), float((mean - x[0]).abs().max())))
  assert bool((m2 == 0).all()) and bool((st[2] == 0).all())
  assert _same(mean, x[0]) and _same(st[1], x[0]) and _same(st[3], x[0]) and _same(st[4], x[0])
  for relu in (True, False):
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    y, yh, bound, mbytes, saved = _ffi.bn_fwd_hl8(x, r, c, res, t['resb'], gamma, beta, rm, rv, MOM, EPS, relu, True,
                                                  True, relu)
    want = beta + res
    assert _same(y, torch.relu(want) if relu else want)
    assert _rel(saved[1], torch.full((c,), EPS, device=DEV).double().rsqrt()) <= 2.0 ** -22
    torch.testing.assert_close(rv, torch.full((c,), 1.0 - MOM, device=DEV), rtol=1e-6, atol=0)
    _check_hl8(yh, y, 'bn_fwd_hl8', 'constant (300, 40)')
    assert math.isfinite(float(bound)) and float(bound) >= float(y.abs().max())
    yf, _, _ = _ffi.bn_act_fwd(x, res, gamma, beta, None, None, MOM, EPS, relu)
    assert _same(yf, y)
    one = _ffi.bn_bwd_hl8(dy, mbytes, x, r, c, saved, gamma, True)
    stb = _ffi.bn_act_bwd_reduce_ext(dy, y if relu else None, None, x, r, c, saved[0], saved[1])
    dx, dxh, dres = _ffi.bn_act_bwd_apply_hl8(dy, y if relu else None, None, x, r, c, saved[0], saved[1], gamma, stb[0],
                                              stb[1], stb[2], saved[2], saved[3], r, True, True, True)
    for v in (one[1], one[2], one[3], one[0].bound, stb, dx, dres, dxh.bound, ref.hl8_halves(one[0]),
              ref.hl8_halves(dxh)):
      assert bool(torch.isfinite(v).all())
    assert bool((stb[1] == 0).all())                           # xhat = 0 everywhere
    mask = (y > 0) if relu else torch.ones_like(dy, dtype=torch.bool)
    bw = ref.backward(dy, x, x[0].double(), torch.full((c,), EPS, device=DEV).double().rsqrt(), gamma, mask if relu else None)
    _check_hl8(dxh, dx, 'bn_act_bwd_apply_hl8', 'constant (300, 40)')
    _check_hl8(one[0], dx, 'bn_bwd_hl8', 'constant (300, 40)')
    assert float(dxh.bound) >= float(bw['dx'].abs().max()) and float(one[0].bound) >= float(bw['dx'].abs().max())
