"""bn3's backward sums taken in the epilogue of the data gradient of the unit above
(`spml_conv_hl8_bwd_stats_addend_f32`, `mc_bottleneck._Handover`) against the route they replace
(`spml_conv_hl8_f32` with the addend -> `bn_partial<1,2>` + `bn_merge<1>`).

Kernel level: `out` is bit-identical to `conv_hl8(..., addend, addend_mask)`, max|dz| to the reduction pass; sum dz and
sum dz * xhat are compared with an fp64 reference computed on the CPU from the returned `out`.  As in
tests/test_conv_bn_bwd_stats_gpu.py the bound is not fixed in advance: the error of the existing route against the
same reference is measured over the same cases, and the epilogue route is allowed twice the worst of them (both are
fp32 sums of the same terms in different fixed orders).

Unit level: chains of `Bottleneck` units in deterministic mode with `SPML_BN3_HANDOVER` 0 / 1 / 2 against an fp64
autograd reference of the same modules (CPU); every gradient of the hand-over route may be twice as far from the
reference as the old route's is on the same inputs.  Mode 2 of the plan (bn3's backward before the join) is not built
(profiles/bn3_handover.md): the value 2 selects the same route as 1, which the bit-for-bit comparison of the two pins.  Measured figures: profiles/bn3_handover.md."""
import copy
import ctypes
import os

import pytest
import torch

from spml_amd import _ffi, mc_bottleneck

DEV = 'cuda:0'
gpu = pytest.mark.gpu

K = 64
WIDTHS = [256, 512]                      # N = 512: two column tiles, i.e. the stride of the [3][row tiles][N] planes
# rows: 646 (partial last tile), 156 (fewer rows than a 160-row tile), 15 (fewer than one 16-row block), 161 (one row
# past a 160-row tile: the last chunk is a single row)
GEOMS = [(2, 17, 19), (1, 12, 13), (1, 3, 5), (1, 161, 1)]
ENVS = [{}, dict(SPML_CONV_RB='4'), dict(SPML_CONV_RB='5')]       # 96-, 128- and 160-row tiles
FORMS = ['masked', 'unmasked']
SEEDS = [1, 2, 3]
CASES = [(n, g, e, f) for n in WIDTHS for g in GEOMS for e in ENVS for f in FORMS]


def _case_id(case):
  n, (ni, h, w), env, form = case
  return 'n%d-r%d%s-%s' % (n, ni * h * w, ''.join('-%s%s' % (a[10:], b) for a, b in env.items()), form)


def _operands(n, geom, seed, form, k=K):
  ni, h, w = geom
  rows = ni * h * w
  g = torch.Generator().manual_seed(1000 * seed + rows + n)
  cl = dict(memory_format=torch.channels_last)
  x = torch.randn(ni, k, h, w, generator=g).to(DEV).contiguous(**cl)
  wt = (torch.randn(n, k, 1, 1, generator=g) * k ** -0.5).to(DEV)
  a = (torch.randn(ni, n, h, w, generator=g) * 1.3 + 0.4).to(DEV).contiguous(**cl)          # the batch norm's saved input
  mask = torch.randint(0, 16, (rows * (n // 4),), generator=g, dtype=torch.uint8).to(DEV)
  mean = (0.4 + 0.1 * torch.randn(n, generator=g)).to(DEV)
  invstd = (0.5 + torch.rand(n, generator=g)).to(DEV)
  addend = torch.randn(ni, n, h, w, generator=g).to(DEV).contiguous(**cl)
  amask = torch.randint(0, 16, (rows * (n // 4),), generator=g, dtype=torch.uint8).to(DEV) if form == 'masked' else None
  return _ffi.hl8_from_f32(x), _ffi.hl8_weight(wt)[0], a, mask, mean, invstd, addend, amask


def _reference(out, a, mask, mean, invstd, rows, n):
  """fp64 on the CPU: (sum dz, sum dz xhat, sum |dz|, sum |dz xhat|) per channel."""
  o = out.permute(0, 2, 3, 1).reshape(rows, n).double().cpu()
  av = a.permute(0, 2, 3, 1).reshape(rows, n).double().cpu()
  bits = (mask.cpu().view(rows, n // 4, 1) >> torch.arange(4, dtype=torch.uint8).view(1, 1, 4)) & 1
  dz = o * bits.reshape(rows, n).double()
  t1 = dz * (av - mean.double().cpu()) * invstd.double().cpu()
  return dz.sum(0), t1.sum(0), dz.abs().sum(0), t1.abs().sum(0)


def _rel(got, want, scale):
  return ((got.double().cpu() - want).abs() / scale.clamp_min(1e-300)).max().item()


class _Env(object):
  def __init__(self, env):
    self.env = env

  def __enter__(self):
    self.old = {key: os.environ.get(key) for key in self.env}
    os.environ.update(self.env)

  def __exit__(self, *exc):
    for key, v in self.old.items():
      if v is None:
        os.environ.pop(key, None)
      else:
        os.environ[key] = v


@pytest.fixture(scope='module')
def measured():
  """Every case x seed once: both routes and the shared fp64 reference."""
  res = {}
  for case in CASES:
    n, geom, env, form = case
    ni, h, w = geom
    rows = ni * h * w
    with _Env(env):
      for seed in SEEDS:
        xh, wf, a, mask, mean, invstd, addend, amask = _operands(n, geom, seed, form)
        plain = _ffi.conv_hl8(xh, wf, ni, h, w, 1, 1, addend=addend, addend_mask=amask)
        out, cs = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, 1, 1, a, mask, mean, addend=addend, addend_mask=amask)
        assert cs is not None and cs.data.shape == (3, cs.chunks, n)
        out2, cs2 = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, 1, 1, a, mask, mean, addend=addend, addend_mask=amask)
        st_old = _ffi.bn_act_bwd_reduce_ext(plain, None, mask, a, rows, n, mean, invstd)
        st_new = _ffi.bn_act_bwd_reduce_ext(out, None, mask, a, rows, n, mean, invstd, chunk_stats=cs)
        ref = _reference(out, a, mask, mean, invstd, rows, n)
        res[(_case_id(case), seed)] = dict(
            same_out=torch.equal(out, plain), same_max=torch.equal(st_new[2], st_old[2]),
            repeat=torch.equal(out2, out) and torch.equal(cs2.data, cs.data), chunks=cs.chunks, chunk_rows=cs.chunk_rows,
            bound_slot=float(cs.bound),
            old=(_rel(st_old[0], ref[0], ref[2]), _rel(st_old[1], ref[1], ref[3])),
            new=(_rel(st_new[0], ref[0], ref[2]), _rel(st_new[1], ref[1], ref[3])))
  worst_old = tuple(max(r['old'][i] for r in res.values()) for i in range(2))
  worst_new = tuple(max(r['new'][i] for r in res.values()) for i in range(2))
  print('\nbn3 backward statistics, worst error / sum |term| over %d cases x %d seeds: existing route %.3e / %.3e, '
        'epilogue route %.3e / %.3e, allowed %.3e / %.3e' %
        (len(CASES), len(SEEDS), worst_old[0], worst_old[1], worst_new[0], worst_new[1], 2 * worst_old[0], 2 * worst_old[1]))
  return res, worst_old


@gpu
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_epilogue_statistics_with_addend(case, measured):
  res, worst_old = measured
  n, geom, env, form = case
  rows = geom[0] * geom[1] * geom[2]
  want_rows = {None: 96, '4': 128, '5': 160}[env.get('SPML_CONV_RB')]
  for seed in SEEDS:
    r = res[(_case_id(case), seed)]
    print(_case_id(case), seed, r)
    assert r['chunk_rows'] == want_rows
    assert (r['chunks'] - 1) * r['chunk_rows'] < rows <= r['chunks'] * r['chunk_rows']
    assert r['same_out'], 'out differs from conv_hl8 with the addend'
    assert r['same_max'], 'max |dz| differs from bn_act_bwd_reduce_ext'
    assert r['repeat'], 'two calls on the same inputs differ'
    assert r['bound_slot'] == 0.0
    assert r['new'][0] <= 2 * worst_old[0], (r['new'][0], worst_old[0])
    assert r['new'][1] <= 2 * worst_old[1], (r['new'][1], worst_old[1])


@gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n_out', [128, 64])
def test_narrow_outputs_are_refused_and_take_the_plain_route(n_out, form):
  geom = (2, 17, 19)
  ni, h, w = geom
  xh, wf, a, mask, mean, _, addend, amask = _operands(n_out, geom, 5, form)
  chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
  rc = _ffi.lib().spml_conv_hl8_bwd_stats_layout(ni, h, w, K, n_out, 1, ctypes.byref(chunks), ctypes.byref(rows))
  assert rc != 0
  st = torch.empty((3, 8, n_out), device=DEV)
  out = torch.empty((ni, n_out, h, w), device=DEV).contiguous(memory_format=torch.channels_last)
  assert _ffi.lib().spml_conv_hl8_bwd_stats_addend_f32(
      _ffi.ptr(xh.data), _ffi._dp(xh.bound), _ffi.ptr(wf.data), _ffi._dp(wf.bound), _ffi._dp(out), _ffi._dp(a),
      _ffi._dp(mask), _ffi._dp(mean), _ffi._dp(st), None, ni, h, w, K, n_out, 1, 1, _ffi._dp(addend), _ffi._dp(amask),
      _ffi.stream_ptr()) == rc
  got, cs = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, 1, 1, a, mask, mean, addend=addend, addend_mask=amask)
  assert cs is None
  assert torch.equal(got, _ffi.conv_hl8(xh, wf, ni, h, w, 1, 1, addend=addend, addend_mask=amask))


# ---------------------------------------------------------------------------------------------------------------
# unit chains
# ---------------------------------------------------------------------------------------------------------------
MODES = ['0', '1', '2']
# (inplanes, planes, downsample) per unit: three plain units; the first unit with a downsample branch (its bn3
# backward also writes the gradient of that branch from the handed sums); a downsample unit in the middle (its last
# data gradient is the second launch, with the unmasked addend)
# Widths: 512 -> 128 -> 512 is the narrowest unit the matrix-core path takes (the weight gradient tiles multiples of
# 128 channels); 256 -> 64 -> 256 runs on the framework convolutions and has its own test below.
CHAINS = {'plain': [(512, 128, False)] * 3,
          'ds_first': [(256, 128, True), (512, 128, False), (512, 128, False)],
          'ds_middle': [(512, 128, False), (512, 128, True), (512, 128, False)]}
GEOM = (2, 17, 19)


def _make_chain(spec, seed):
  from spml_amd.models.backbones.resnet import Bottleneck, _bn
  torch.manual_seed(seed)
  units = []
  for inplanes, planes, downsample in spec:
    ds = None
    if downsample:
      ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, bias=False), _bn(planes * 4))
    units.append(Bottleneck(inplanes, planes, 1, dilation=2, downsample=ds))
  net = torch.nn.Sequential(*units)
  for m in net.modules():
    if isinstance(m, torch.nn.Conv2d):
      fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
      m.weight.data.normal_(0, (2.0 / fan) ** 0.5)
    elif isinstance(m, torch.nn.BatchNorm2d):
      m.weight.data.uniform_(0.5, 1.5)
      m.bias.data.uniform_(-0.2, 0.2)
  return net.train()


def _inputs(spec, seed=7):
  n, h, w = GEOM
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, spec[0][0], h, w, generator=g).clamp_min(0)
  up = torch.randn(n, spec[-1][1] * 4, h, w, generator=g) * 1e-3
  return x, up


def _forward(net, xi, second_consumer):
  """The chain unit by unit; second_consumer: the middle activation also feeds a reduction of its own."""
  mid = net[1](net[0](xi))
  y = net[2](mid)
  return y + mid.mean() if second_consumer else y


def _run_gpu(net, x, up, second_consumer=False, twice=False, matrix_core=True):
  """-> list (one entry per backward) of {name: gradient}, the input gradient under 'x'."""
  net = copy.deepcopy(net).to(DEV).to(memory_format=torch.channels_last)
  cl = dict(memory_format=torch.channels_last)
  xi = x.to(DEV).contiguous(**cl).requires_grad_(True)
  for unit in net:
    assert unit.downsample is not None or unit.conv1.in_channels == unit.conv3.out_channels
  assert mc_bottleneck.available(net[0], xi) == matrix_core
  loss = (_forward(net, xi, second_consumer) * up.to(DEV).contiguous(**cl)).sum()
  outs = []
  for i in range(2 if twice else 1):
    xi.grad = None
    net.zero_grad(set_to_none=True)
    loss.backward(retain_graph=twice and i == 0)
    g = {k: p.grad.clone() for k, p in net.named_parameters()}
    g['x'] = xi.grad.clone()
    outs.append(g)
  return outs


def _run_ref64(net, x, up, second_consumer=False):
  net = copy.deepcopy(net).double()
  xi = x.double().requires_grad_(True)
  (_forward(net, xi, second_consumer) * up.double()).sum().backward()
  g = {k: p.grad for k, p in net.named_parameters()}
  g['x'] = xi.grad
  return g


def _errors(got, ref):
  """max |got - ref| / max |ref| per gradient."""
  return {k: (got[k].double().cpu() - ref[k]).abs().max().item() / max(ref[k].abs().max().item(), 1e-300) for k in ref}


def _same(a, b):
  return all(torch.equal(a[k], b[k]) for k in a)


@pytest.fixture()
def deterministic(monkeypatch):
  monkeypatch.setenv('SPML_NO_MC_CONV', '0')
  monkeypatch.setenv('SPML_DETERMINISTIC', '1')
  monkeypatch.delenv('SPML_CONV_BN_BWD_STATS', raising=False)
  was = _ffi.set_deterministic(True)
  yield monkeypatch
  _ffi.set_deterministic(was)


def _spy(monkeypatch):
  """Records (has addend, statistics returned) of every conv_hl8_bwd_stats call and counts the raw entry point."""
  calls, raw = [], []
  real = _ffi.conv_hl8_bwd_stats

  def wrapper(*a, **k):
    out = real(*a, **k)
    calls.append((k.get('addend') is not None, out[1] is not None))
    return out
  monkeypatch.setattr(_ffi, 'conv_hl8_bwd_stats', wrapper)
  lib = _ffi.lib()
  real_entry = lib.spml_conv_hl8_bwd_stats_addend_f32

  class Lib(object):
    def __getattr__(self, name):
      if name == 'spml_conv_hl8_bwd_stats_addend_f32':
        return lambda *a: (raw.append(1), real_entry(*a))[1]
      return getattr(lib, name)
  proxy = Lib()
  monkeypatch.setattr(_ffi, 'lib', lambda: proxy)
  return calls, raw


@gpu
@pytest.mark.parametrize('chain', sorted(CHAINS))
def test_unit_chain_gradients_against_fp64(chain, deterministic):
  spec = CHAINS[chain]
  net = _make_chain(spec, seed=11)
  x, up = _inputs(spec)
  ref = _run_ref64(net, x, up)
  calls, raw = _spy(deterministic)
  runs, used = {}, {}
  for mode in MODES:
    deterministic.setenv('SPML_BN3_HANDOVER', mode)
    before, n_raw = mc_bottleneck._Handover.taken, len(raw)
    runs[mode] = [_run_gpu(net, x, up)[0] for _ in range(2)]
    used[mode] = (mc_bottleneck._Handover.taken - before, len(raw) - n_raw)
    assert _same(*runs[mode]), 'mode %s does not reproduce its own bits' % mode
  # two hand-overs per backward (units 2 -> 1 and 1 -> 0), none with the switch off
  assert used['0'] == (0, 0) and used['1'] == (4, 4) and used['2'] == (4, 4), used
  assert _same(runs['1'][0], runs['2'][0]), 'modes 1 and 2 differ'
  e0, e1 = _errors(runs['0'][0], ref), _errors(runs['1'][0], ref)
  for k in sorted(ref):
    print('%-28s mode 0 %.3e  mode 1 %.3e' % (k, e0[k], e1[k]))
  for k in ref:
    assert e1[k] <= 2 * e0[k], (k, e1[k], e0[k])
  # Where a ReLU of the fp32 forward lands on the other side of zero than the fp64 one's, both errors above are that
  # flip's (the forward does not depend on the mode).  So also: the two routes against each other, within the bounds
  # tests/test_conv_bn_bwd_stats_gpu.py applies to the bn1 / bn2 routes (their sums differ at the 1e-7 level)
  for k in ref:
    a, b = runs['1'][0][k], runs['0'][0][k]
    assert (a - b).abs().max().item() <= (2e-4 if k == 'x' else 5e-4) * max(b.abs().max().item(), 1e-30), k
  # the top unit's bn3 has no unit above it: its own gradients do not depend on the switch
  for k in ref:
    if k.startswith('2.bn3'):
      assert torch.equal(runs['0'][0][k], runs['1'][0][k]), k


@gpu
def test_second_consumer_keeps_the_old_route_for_that_activation(deterministic):
  spec = CHAINS['plain']
  net = _make_chain(spec, seed=12)
  x, up = _inputs(spec, seed=8)
  ref = _run_ref64(net, x, up, second_consumer=True)
  deterministic.setenv('SPML_BN3_HANDOVER', '0')
  g0 = _run_gpu(net, x, up, second_consumer=True)[0]
  e0 = _errors(g0, ref)
  for mode in MODES[1:]:
    deterministic.setenv('SPML_BN3_HANDOVER', mode)
    before = mc_bottleneck._Handover.taken
    g1 = _run_gpu(net, x, up, second_consumer=True)[0]
    # unit 1's d_out is the sum of two gradients, not the tensor unit 2 left its sums (or results) for: only the
    # hand-over unit 1 -> unit 0 is used
    assert mc_bottleneck._Handover.taken - before == 1
    e1 = _errors(g1, ref)
    for k in ref:
      assert e1[k] <= 2 * e0[k], (mode, k, e1[k], e0[k])
    for k in ref:                                # nothing of units 1 and 2 changed
      if k[0] in '12':
        assert torch.equal(g0[k], g1[k]), (mode, k)


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_backward_twice_over_a_retained_graph(mode, deterministic):
  spec = CHAINS['ds_first']
  net = _make_chain(spec, seed=13)
  x, up = _inputs(spec, seed=9)
  deterministic.setenv('SPML_BN3_HANDOVER', mode)
  first, second = _run_gpu(net, x, up, twice=True)
  assert _same(first, second)


@gpu
def test_switched_off_statistics_never_reach_the_new_entry_point(deterministic):
  spec = CHAINS['ds_middle']
  net = _make_chain(spec, seed=14)
  x, up = _inputs(spec)
  calls, raw = _spy(deterministic)
  deterministic.setenv('SPML_BN3_HANDOVER', '2')
  deterministic.setenv('SPML_CONV_BN_BWD_STATS', '0')
  before = mc_bottleneck._Handover.taken
  g_off = _run_gpu(net, x, up)[0]
  assert not raw and mc_bottleneck._Handover.taken == before
  assert all(not got for _, got in calls)
  deterministic.setenv('SPML_BN3_HANDOVER', '0')
  deterministic.delenv('SPML_CONV_BN_BWD_STATS')
  assert _same(g_off, _run_gpu(net, x, up)[0])         # (128-wide bn1 / bn2 never take the epilogue route)


@gpu
def test_units_off_the_matrix_core_path_have_no_handover(deterministic):
  """256 -> 64 -> 256: the weight gradient does not tile 64 channels, the units run on the framework convolutions and
  the switch reaches nothing."""
  spec = [(256, 64, False)] * 3
  net = _make_chain(spec, seed=15)
  x, up = _inputs(spec)
  before = mc_bottleneck._Handover.taken
  runs = {}
  for mode in MODES:
    deterministic.setenv('SPML_BN3_HANDOVER', mode)
    runs[mode] = _run_gpu(net, x, up, matrix_core=False)[0]
  assert mc_bottleneck._Handover.taken == before
  assert all(torch.isfinite(g).all() for r in runs.values() for g in r.values())


# ---------------------------------------------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------------------------------------------
def _host_operands(rows, k, n):
  a = _ffi.Hl8(torch.empty(rows * k * 4, dtype=torch.uint8), torch.ones(1), rows, k)
  b = _ffi.Hl8(torch.empty(n * k * 4, dtype=torch.uint8), torch.ones(1), n, k)
  return a, b


@pytest.mark.parametrize('bad', ['addend', 'addend_mask', 'mask_without_addend', 'bn_x'])
def test_wrapper_raises_on_mismatched_operand_shapes(bad):
  ni, h, w, k, n = 1, 12, 13, 64, 256
  rows = ni * h * w
  a, b = _host_operands(rows, k, n)
  args = dict(bn_x=torch.empty(rows * n), relu_mask=torch.empty(rows * n // 4, dtype=torch.uint8), bn_mean=torch.empty(n),
              addend=torch.empty(rows * n), addend_mask=torch.empty(rows * n // 4, dtype=torch.uint8))
  if bad == 'addend':
    args['addend'] = torch.empty(rows * n - n)
  elif bad == 'addend_mask':
    args['addend_mask'] = torch.empty(rows * n // 4 + 1, dtype=torch.uint8)
  elif bad == 'mask_without_addend':
    args['addend'] = None
  else:
    args['bn_x'] = torch.empty(rows * n + 4)
  with pytest.raises(_ffi.SpmlHipError, match='operand shapes'):
    _ffi.conv_hl8_bwd_stats(a, b, ni, h, w, 1, 1, args['bn_x'], args['relu_mask'], args['bn_mean'],
                            addend=args['addend'], addend_mask=args['addend_mask'])


def test_handover_guard_is_host_logic():
  """`take` hands the sums out once, and only for the tensor `put` saw, unmodified."""
  h = mc_bottleneck._Handover()
  dx, other = torch.zeros(2, 8, 3, 3), torch.zeros(2, 8, 3, 3)
  before = mc_bottleneck._Handover.taken
  assert h.take(dx) is None                                       # nothing was put
  h.put(dx, 'sums')
  assert h.take(other) is None and h.take(dx) is None             # another tensor; and the holder is emptied on use
  h.put(dx, 'sums')
  dx.add_(1)
  assert h.take(dx) is None                                       # modified in place since
  h.put(dx, 'sums')
  assert h.take(dx.view(2, 8, 9)) is None                         # same storage, another shape
  assert mc_bottleneck._Handover.taken == before
  h.put(dx, 'sums')
  assert h.take(dx) == 'sums' and mc_bottleneck._Handover.taken == before + 1
