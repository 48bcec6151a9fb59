"""Backward batch-norm statistics taken in the epilogue of the data-gradient convolution
(`spml_conv_hl8_bwd_stats_f32` -> `spml_bn_bwd_hl8_chunks_f32` / `spml_bn_act_bwd_reduce_ext_chunks_f32`)
against the route they replace (`spml_conv_hl8_f32` -> `bn_partial<1,2>` + `bn_merge<1>`).

Kernel level: `out` and max|dz| are bit-identical to the plain route; sum dz and sum dz * xhat are compared with an
fp64 reference computed on the CPU from the returned `out`, the saved input, the mask and the mean.  The bound is
not fixed in advance: the error of the existing route against the same reference is measured over the same shapes
and three seeds, relative to sum |term| per channel, and the epilogue route is allowed twice the worst of them
(both are fp32 sums of the same terms in different fixed orders).  Measured figures: profiles/bn_bwd_stats.md."""
import copy
import ctypes

import pytest
import torch

from spml_amd import _ffi, mc_bottleneck

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

# (taps, dilation, K, N): 1x1 256 -> 256; 3x3 dilation 2 256 -> 256; 1x1 128 -> 512 (two column tiles)
CONVS = [(1, 1, 256, 256), (9, 2, 256, 256), (1, 1, 128, 512)]
# rows n*h*w = 646 (partial last tile), 156 (fewer rows than one 160-row tile), 320 (exact 160-row tiles)
GEOMS = [(2, 17, 19), (1, 12, 13), (1, 16, 20)]
SEEDS = [1, 2, 3]
# the launch picks 96-row tiles for shapes this small; the 128- and 160-row tiles (what the training step runs) and the
# chunked accumulation (3x3 of res5) are selected through the library's tuning switches
EXTRA = [dict(SPML_CONV_RB='4'), dict(SPML_CONV_RB='5'), dict(SPML_CONV_CHUNK_MIN_K='2304')]
CASES = [(c, g, {}) for c in CONVS for g in GEOMS] + \
        [(c, GEOMS[0], e) for c in CONVS[:2] for e in EXTRA[:2]] + [(CONVS[1], g, EXTRA[2]) for g in GEOMS[:2]] + \
        [(CONVS[2], g, EXTRA[1]) for g in GEOMS[1:]]
# geometry edges of the epilogue's row range check: one row past a tile (97 = 96 + 1 on the default 96-row tiles,
# 161 = 160 + 1 under SPML_CONV_RB=5: the last chunk is a single row) and fewer rows than one 16-row block (15)
EDGE_GEOMS = [(1, 97, 1), (1, 3, 5)]
CASES += [(c, g, {}) for c in CONVS for g in EDGE_GEOMS] + [(CONVS[0], (1, 161, 1), EXTRA[1]), (CONVS[1], (1, 3, 5), EXTRA[1])]


def _case_id(case):
  (taps, dil, k, n), (ni, h, w), env = case
  return '%dtap-k%d-n%d-r%d%s' % (taps, k, n, ni * h * w, ''.join('-%s%s' % (a[10:], b) for a, b in env.items()))


def _operands(conv, geom, seed):
  taps, dil, k, n = conv
  ni, h, w = geom
  rows = ni * h * w
  g = torch.Generator().manual_seed(1000 * seed + rows + taps)
  cl = dict(memory_format=torch.channels_last)
  x = torch.randn(ni, k, h, w, generator=g).to(DEV).contiguous(**cl)
  wt = (torch.randn(n, k, 3 if taps == 9 else 1, 3 if taps == 9 else 1, generator=g) * (taps * k) ** -0.5).to(DEV)
  a = (torch.randn(ni, n, h, w, generator=g) * 1.3 + 0.4).to(DEV).contiguous(**cl)          # the batch norm's saved input
  mask = torch.randint(0, 16, (rows * (n // 4),), generator=g, dtype=torch.uint8).to(DEV)
  mean = (0.4 + 0.1 * torch.randn(n, generator=g)).to(DEV)
  invstd = (0.5 + torch.rand(n, generator=g)).to(DEV)
  return _ffi.hl8_from_f32(x), _ffi.hl8_weight(wt)[0], a, mask, mean, invstd


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


@pytest.fixture(scope='module')
def measured():
  """Every case x seed once: both routes and the shared fp64 reference."""
  import os
  res = {}
  for case in CASES:
    conv, geom, env = case
    taps, dil, k, n = conv
    ni, h, w = geom
    rows = ni * h * w
    old_env = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    try:
      for seed in SEEDS:
        xh, wf, a, mask, mean, invstd = _operands(conv, geom, seed)
        plain = _ffi.conv_hl8(xh, wf, ni, h, w, taps, dil)
        out, cs = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, taps, dil, a, mask, mean)
        assert cs is not None and cs.data.shape == (3, cs.chunks, n)
        out2, cs2 = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, taps, dil, a, mask, mean)
        st_old = _ffi.bn_act_bwd_reduce_ext(plain, None, mask, a, rows, n, mean, invstd)
        st_new = _ffi.bn_act_bwd_reduce_ext(out, None, mask, a, rows, n, mean, invstd, chunk_stats=cs)
        ref = _reference(out, a, mask, mean, invstd, rows, n)
        res[(_case_id(case), seed)] = dict(
            same_out=torch.equal(out, plain), same_max=torch.equal(st_new[2], st_old[2]),
            repeat=torch.equal(out2, out) and torch.equal(cs2.data, cs.data), chunks=cs.chunks, chunk_rows=cs.chunk_rows,
            bound_slot=float(cs.bound),
            old=(_rel(st_old[0], ref[0], ref[2]), _rel(st_old[1], ref[1], ref[3])),
            new=(_rel(st_new[0], ref[0], ref[2]), _rel(st_new[1], ref[1], ref[3])))
    finally:
      for key, v in old_env.items():
        if v is None:
          os.environ.pop(key, None)
        else:
          os.environ[key] = v
  worst_old = tuple(max(r['old'][i] for r in res.values()) for i in range(2))
  worst_new = tuple(max(r['new'][i] for r in res.values()) for i in range(2))
  print('\nbackward statistics, worst error / sum |term| over %d cases x %d seeds: existing route %.3e / %.3e, '
        'epilogue route %.3e / %.3e, allowed %.3e / %.3e' %
        (len(CASES), len(SEEDS), worst_old[0], worst_old[1], worst_new[0], worst_new[1], 2 * worst_old[0], 2 * worst_old[1]))
  return res, worst_old


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_epilogue_statistics(case, measured):
  res, worst_old = measured
  rows = case[1][0] * case[1][1] * case[1][2]
  for seed in SEEDS:
    r = res[(_case_id(case), seed)]
    print(_case_id(case), seed, r)
    assert (r['chunks'] - 1) * r['chunk_rows'] < rows <= r['chunks'] * r['chunk_rows']
    assert r['same_out'], 'out differs from conv_hl8'
    assert r['same_max'], 'max |dz| differs from bn_act_bwd_reduce_ext'
    assert r['repeat'], 'two calls on the same inputs differ'
    assert r['bound_slot'] == 0.0
    assert r['new'][0] <= 2 * worst_old[0], (r['new'][0], worst_old[0])
    assert r['new'][1] <= 2 * worst_old[1], (r['new'][1], worst_old[1])


@pytest.mark.parametrize('n_out', [128, 64])
def test_narrow_outputs_are_refused_and_take_the_plain_route(n_out):
  conv, geom = (1, 1, 256, n_out), (2, 17, 19)
  ni, h, w = geom
  xh, wf, a, mask, mean, _ = _operands(conv, geom, 5)
  chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
  rc = _ffi.lib().spml_conv_hl8_bwd_stats_layout(ni, h, w, 256, n_out, 1, ctypes.byref(chunks), ctypes.byref(rows))
  assert rc == _ffi.lib().spml_conv_hl8_stats_layout(ni, h, w, 256, n_out, 1, ctypes.byref(chunks), ctypes.byref(rows))
  assert rc != 0
  st = torch.empty((3, 8, n_out), device=DEV)
  out = torch.empty((ni, n_out, h, w), device=DEV).contiguous(memory_format=torch.channels_last)
  assert _ffi.lib().spml_conv_hl8_bwd_stats_f32(
      _ffi.ptr(xh.data), _ffi._dp(xh.bound), _ffi.ptr(wf.data), _ffi._dp(wf.bound), _ffi._dp(out), _ffi._dp(a),
      _ffi._dp(mask), _ffi._dp(mean), _ffi._dp(st), None, ni, h, w, 256, n_out, 1, 1, _ffi.stream_ptr()) == rc
  got, cs = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, 1, 1, a, mask, mean)
  assert cs is None
  assert torch.equal(got, _ffi.conv_hl8(xh, wf, ni, h, w, 1, 1))


def test_single_rank_and_sync_forms_from_the_planes(measured):
  """`bn_bwd_hl8` (single rank) and the SyncBatchNorm form (reduction, then the apply pass that would follow the
  all-reduce; one process, one emulated rank) from the planes against the same calls on the tensor: sums within the
  measured bound, the same max |dz|, and the gradients / bounds they lead to."""
  _, worst_old = measured
  conv, geom = CONVS[1], GEOMS[0]
  taps, dil, k, n = conv
  ni, h, w = geom
  rows = ni * h * w
  xh, wf, a, mask, mean, invstd = _operands(conv, geom, 4)
  gamma = torch.linspace(0.5, 1.5, n, device=DEV)
  av = a.permute(0, 2, 3, 1).reshape(rows, n)
  saved = (mean, invstd, av.max(0).values.contiguous(), av.min(0).values.contiguous())
  dy, cs = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, taps, dil, a, mask, mean)
  ref = _reference(dy, a, mask, mean, invstd, rows, n)
  # SyncBatchNorm form
  st_t = _ffi.bn_act_bwd_reduce_ext(dy, None, mask, a, rows, n, mean, invstd)
  st_p = _ffi.bn_act_bwd_reduce_ext(dy, None, mask, a, rows, n, mean, invstd, chunk_stats=cs)
  assert torch.equal(st_p[2], st_t[2])
  assert _rel(st_p[0], ref[0], ref[2]) <= 2 * worst_old[0]
  assert _rel(st_p[1], ref[1], ref[3]) <= 2 * worst_old[1]
  outs = [_ffi.bn_act_bwd_apply_hl8(dy, None, mask, a, rows, n, mean, invstd, gamma, s[0], s[1], s[2], saved[2], saved[3],
                                    rows, want_dx_f32=True) for s in (st_t, st_p)]
  scale = outs[0][0].abs().max().item()
  assert (outs[1][0] - outs[0][0]).abs().max().item() <= 1e-6 * scale
  torch.testing.assert_close(outs[1][1].bound, outs[0][1].bound, rtol=1e-6, atol=0)
  # single rank: the bound slot the convolution reset is the one bn_merge max-reduces into
  dy2, cs2 = _ffi.conv_hl8_bwd_stats(xh, wf, ni, h, w, taps, dil, a, mask, mean)
  dx_t, _, dg_t, db_t = _ffi.bn_bwd_hl8(dy, mask, a, rows, n, saved, gamma)
  dx_p, _, dg_p, db_p = _ffi.bn_bwd_hl8(dy2, mask, a, rows, n, saved, gamma, chunk_stats=cs2)
  assert dx_p.bound.data_ptr() == cs2.bound.data_ptr()
  torch.testing.assert_close(dx_p.bound, dx_t.bound, rtol=1e-6, atol=0)
  torch.testing.assert_close(dx_p.bound, outs[0][1].bound, rtol=1e-5, atol=0)
  assert _rel(db_p, ref[0], ref[2]) <= 2 * worst_old[0]
  assert _rel(dg_p, ref[1], ref[3]) <= 2 * worst_old[1]


def _make_unit(inplanes, planes, dilation, downsample, seed):
  from spml_amd.models.backbones.resnet import Bottleneck, _bn
  torch.manual_seed(seed)
  ds = None
  if downsample:
    ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, bias=False), _bn(planes * 4))
  blk = Bottleneck(inplanes, planes, 1, dilation=dilation, downsample=ds)
  for m in blk.modules():
    if isinstance(m, torch.nn.Conv2d):
      fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
      m.weight.data.normal_(0, (2.0 / fan) ** 0.5)
    elif isinstance(m, torch.nn.BatchNorm2d):
      m.weight.data.uniform_(0.5, 1.5)
      m.bias.data.uniform_(-0.2, 0.2)
  return blk.to(DEV).to(memory_format=torch.channels_last).train()


def _run_unit(blk, x, up):
  blk = copy.deepcopy(blk)
  xi = x.clone().requires_grad_(True)
  assert mc_bottleneck.available(blk, xi)
  y = blk(xi)
  (y * up).sum().backward()
  return xi.grad, {n: p.grad.clone() for n, p in blk.named_parameters()}


@pytest.mark.parametrize('inplanes,planes,dil,ds,n,h,w', [(1024, 256, 2, False, 2, 17, 19), (512, 256, 1, True, 2, 12, 9)])
def test_unit_backward_with_and_without_the_epilogue_route(inplanes, planes, dil, ds, n, h, w, monkeypatch):
  """`_Unit` forward + backward with SPML_CONV_BN_BWD_STATS on and off: dx and every weight / gamma / beta gradient
  agree within the bounds tests/test_mc_bottleneck_gpu.py applies against the framework ops, and in deterministic
  mode each setting reproduces its own bits."""
  monkeypatch.setenv('SPML_NO_MC_CONV', '0')
  monkeypatch.setenv('SPML_DETERMINISTIC', '1')
  was = _ffi.set_deterministic(True)
  try:
    blk = _make_unit(inplanes, planes, dil, ds, seed=inplanes + dil)
    g = torch.Generator().manual_seed(7)
    cl = dict(memory_format=torch.channels_last)
    x = torch.randn(n, inplanes, h, w, generator=g).clamp_min(0).to(DEV).contiguous(**cl)
    up = (torch.randn(n, planes * 4, h, w, generator=g) * 1e-3).to(DEV).contiguous(**cl)
    calls = []
    real = _ffi.bn_bwd_hl8
    monkeypatch.setattr(_ffi, 'bn_bwd_hl8', lambda *a, **k: (calls.append(k.get('chunk_stats') is not None), real(*a, **k))[1])
    runs = {}
    for switch in ('1', '0'):
      monkeypatch.setenv('SPML_CONV_BN_BWD_STATS', switch)
      del calls[:]
      runs[switch] = [_run_unit(blk, x, up) for _ in range(2)]
      # bn3 (and the downsample batch norm) never take the planes; bn2 and bn1 take them when the switch is on
      assert calls[:len(calls) // 2] == ([False, switch == '1', switch == '1'] + ([False] if ds else [])), calls
      (dx_a, g_a), (dx_b, g_b) = runs[switch]
      assert torch.equal(dx_a, dx_b)
      for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), (switch, k)
  finally:
    _ffi.set_deterministic(was)

  def close(a, b, tol, what):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= tol * max(scale, 1e-30), (what, err, scale)

  (dx1, g1), (dx0, g0) = runs['1'][0], runs['0'][0]
  close(dx1, dx0, 2e-4, 'input gradient')
  for k in g0:
    close(g1[k], g0[k], 5e-4, k)
