"""Launch trace of the matrix-core bottleneck unit and of conv + bn + relu (spml_amd/mc_bottleneck.py) on the CPU:
the `_ffi` wrappers they call are replaced by fakes that return zero tensors of the right shapes and write down
what they were called with.  What is pinned: the exact sequence of library calls of a forward + backward pass, the
number of tensors the autograd node keeps for the backward, and which gradients come back.  The expected sequences
were recorded before the saved state was given names and the stages were folded into one body each; they are
written out here, not generated."""
import pytest
import torch

from spml_amd import _ffi, mc_bottleneck
from spml_amd.models.backbones.resnet import Bottleneck, _bn

N, H, W = 1, 3, 3


def _tag(name, *flags):
  return '%s(%s)' % (name, ','.join(str(f) for f in flags if f not in (None, False, '')))


@pytest.fixture
def trace(monkeypatch):
  calls = []
  monkeypatch.setenv('SPML_WGRAD_STREAM', '0')             # no side stream: nothing touches torch.cuda
  monkeypatch.delenv('SPML_BN3_HANDOVER', raising=False)
  monkeypatch.delenv('SPML_NO_MC_CONV', raising=False)

  def hl8(rows, channels):
    return _ffi.Hl8(torch.zeros(rows * channels * 4, dtype=torch.uint8), torch.zeros(1), rows, channels)

  def nhwc(n, c, h, w):
    return torch.zeros((n, c, h, w)).contiguous(memory_format=torch.channels_last)

  def chunk_stats(kinds, n):
    return _ffi.ChunkStats(torch.zeros(kinds, 1, n), 1, N * H * W, torch.zeros(1))

  def hl8_from_f32(x, rows=None, channels=None, bound=None):
    calls.append(_tag('hl8_from_f32'))
    if rows is None:
      rows, channels = x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]
    return hl8(rows, channels)

  def hl8_weight_set(weights):
    calls.append(_tag('hl8_weight_set', len(weights)))
    out = []
    for wt in weights:
      co, ci, t = wt.shape[0], wt.shape[1], wt.shape[2] * wt.shape[3]
      out.append((hl8(co, t * ci), hl8(ci, t * co)))
    return out

  def conv_hl8(a, b, n_img, h, w, taps, dilation=1, addend=None, addend_mask=None):
    calls.append(_tag('conv_hl8', taps, addend is not None and 'addend', addend_mask is not None and 'mask'))
    assert a.rows == n_img * h * w and b.channels == taps * a.channels
    return nhwc(n_img, b.rows, h, w)

  def conv_hl8_stats(a, b, n_img, h, w, taps, dilation=1):
    calls.append(_tag('conv_hl8_stats', taps))
    assert a.rows == n_img * h * w and b.channels == taps * a.channels
    return nhwc(n_img, b.rows, h, w), chunk_stats(4, b.rows)

  def conv_hl8_bwd_stats(a, b, n_img, h, w, taps, dilation, bn_x, relu_mask, bn_mean, addend=None, addend_mask=None):
    calls.append(_tag('conv_hl8_bwd_stats', taps, addend is not None and 'addend', addend_mask is not None and 'mask'))
    assert a.rows == n_img * h * w and b.channels == taps * a.channels
    assert bn_x.numel() == a.rows * b.rows and relu_mask.numel() == a.rows * (b.rows // 4) and bn_mean.numel() == b.rows
    return nhwc(n_img, b.rows, h, w), chunk_stats(3, b.rows)

  def conv_wgrad_hl8(dy, x, n_img, h, w, taps, dilation=1):
    calls.append(_tag('conv_wgrad_hl8', taps))
    assert dy.rows == n_img * h * w == x.rows
    side = 3 if taps == 9 else 1
    return torch.zeros((dy.channels, x.channels, side, side)).contiguous(memory_format=torch.channels_last)

  def bn_fwd_hl8(x, rows, channels, residual, residual_bound, gamma, beta, running_mean, running_var, momentum, eps,
                 relu, want_f32, want_hl8, want_mask, chunk_stats=None):
    calls.append(_tag('bn_fwd_hl8', chunk_stats is not None and 'chunks', residual is not None and 'res',
                      relu and 'relu', want_f32 and 'f32', want_hl8 and 'hl8'))
    assert x.numel() == rows * channels and gamma.numel() == channels
    st = torch.zeros(4, channels)
    bound = torch.zeros(1)
    mask = torch.zeros(rows * (channels // 4), dtype=torch.uint8) if want_mask else None
    return (torch.zeros_like(x) if want_f32 else None, hl8(rows, channels) if want_hl8 else None, bound, mask,
            (st[0], st[1], st[2], st[3]))

  def bn_bwd_hl8(dy, relu_mask, x, rows, channels, saved, gamma, want_dres=False, chunk_stats=None):
    calls.append(_tag('bn_bwd_hl8', chunk_stats is not None and 'chunks', want_dres and 'dres'))
    assert dy.numel() == rows * channels == x.numel() and len(saved) == 4 and gamma.numel() == channels
    assert relu_mask is None or relu_mask.numel() == rows * (channels // 4)
    dgb = torch.zeros(2, channels)
    return hl8(rows, channels), (torch.zeros_like(dy) if want_dres else None), dgb[0], dgb[1]

  for fake in (hl8_from_f32, hl8_weight_set, conv_hl8, conv_hl8_stats, conv_hl8_bwd_stats, conv_wgrad_hl8, bn_fwd_hl8,
               bn_bwd_hl8):
    monkeypatch.setattr(_ffi, fake.__name__, fake)
  return calls


def _unit(inplanes, planes, downsample):
  ds = None
  if downsample:
    ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, bias=False), _bn(planes * 4))
  return Bottleneck(inplanes, planes, 1, dilation=2, downsample=ds).train()


def _input(channels, requires_grad=True):
  x = torch.randn(N, channels, H, W).contiguous(memory_format=torch.channels_last)
  return x.requires_grad_(requires_grad)


def _check_grads(modules, x, want_x):
  for m in modules:
    for name, p in m.named_parameters():
      assert p.grad is not None and p.grad.shape == p.shape, name
  assert (x.grad is not None) == want_x
  if want_x:
    assert x.grad.shape == x.shape


FWD_HEAD = ['hl8_from_f32()', 'hl8_weight_set(3)', 'conv_hl8_stats(1)', 'bn_fwd_hl8(chunks,relu,hl8)',
            'conv_hl8_stats(9)', 'bn_fwd_hl8(chunks,relu,hl8)', 'conv_hl8_stats(1)']
FWD_PLAIN = FWD_HEAD + ['bn_fwd_hl8(chunks,res,relu,f32,hl8)']
BWD_BODY = ['conv_wgrad_hl8(1)', 'conv_hl8_bwd_stats(1)', 'bn_bwd_hl8(chunks)', 'conv_wgrad_hl8(9)',
            'conv_hl8_bwd_stats(9)', 'bn_bwd_hl8(chunks)', 'conv_wgrad_hl8(1)']
BWD_PLAIN = ['bn_bwd_hl8()'] + BWD_BODY + ['conv_hl8(1,addend,mask)']


def test_plain_unit(trace):
  blk, x = _unit(256, 64, False), _input(256)
  y = mc_bottleneck.bottleneck_forward(blk, x)
  assert trace == FWD_PLAIN
  assert len(y.grad_fn.saved_tensors) == 33
  assert y.shape == x.shape and y._spml_hl8.channels == 256
  del trace[:]
  y.sum().backward()
  assert trace == BWD_PLAIN
  _check_grads([blk], x, True)


def test_unit_with_downsample(trace):
  blk, x = _unit(128, 64, True), _input(128)
  y = mc_bottleneck.bottleneck_forward(blk, x)
  assert trace == ['hl8_from_f32()', 'hl8_weight_set(4)'] + FWD_HEAD[2:] + [
      'conv_hl8_stats(1)', 'bn_fwd_hl8(chunks,f32)', 'bn_fwd_hl8(chunks,res,relu,f32,hl8)']
  assert len(y.grad_fn.saved_tensors) == 41
  assert y.shape == (N, 256, H, W)
  del trace[:]
  y.sum().backward()
  assert trace == ['bn_bwd_hl8(dres)'] + BWD_BODY + ['bn_bwd_hl8()', 'conv_wgrad_hl8(1)', 'conv_hl8(1)',
                                                     'conv_hl8(1,addend)']
  _check_grads([blk], x, True)


@pytest.mark.parametrize('downsample', [False, True])
def test_unit_whose_input_needs_no_gradient(trace, downsample):
  cin = 128 if downsample else 256
  blk, x = _unit(cin, 64, downsample), _input(cin, requires_grad=False)
  y = mc_bottleneck.bottleneck_forward(blk, x)
  assert len(y.grad_fn.saved_tensors) == (41 if downsample else 33)
  del trace[:]
  y.sum().backward()
  if downsample:
    assert trace == ['bn_bwd_hl8(dres)'] + BWD_BODY + ['bn_bwd_hl8()', 'conv_wgrad_hl8(1)']
  else:
    assert trace == ['bn_bwd_hl8()'] + BWD_BODY
  _check_grads([blk], x, False)


def test_two_chained_units_hand_bn3_sums_over(trace):
  lower, upper, x = _unit(256, 64, False), _unit(256, 64, False), _input(256)
  mid = mc_bottleneck.bottleneck_forward(lower, x)
  y = mc_bottleneck.bottleneck_forward(upper, mid)
  # (the upper unit takes the hl8 copy the lower one left on its output: no conversion pass)
  assert trace == FWD_PLAIN + FWD_PLAIN[1:]
  assert len(mid.grad_fn.saved_tensors) == 33
  assert len(y.grad_fn.saved_tensors) == 33 + 3
  before = mc_bottleneck._Handover.taken
  del trace[:]
  y.sum().backward()
  assert trace == ['bn_bwd_hl8()'] + BWD_BODY + ['conv_hl8_bwd_stats(1,addend,mask)'] + \
      ['bn_bwd_hl8(chunks)'] + BWD_BODY + ['conv_hl8(1,addend,mask)']
  assert mc_bottleneck._Handover.taken == before + 1
  _check_grads([lower, upper], x, True)


def test_handover_switched_off(trace, monkeypatch):
  monkeypatch.setenv('SPML_BN3_HANDOVER', '0')
  lower, upper, x = _unit(256, 64, False), _unit(256, 64, False), _input(256)
  y = mc_bottleneck.bottleneck_forward(upper, mc_bottleneck.bottleneck_forward(lower, x))
  assert len(y.grad_fn.saved_tensors) == 33
  before = mc_bottleneck._Handover.taken
  del trace[:]
  y.sum().backward()
  assert trace == BWD_PLAIN + BWD_PLAIN
  assert mc_bottleneck._Handover.taken == before


def test_unit_without_a_gradient_for_its_output(trace):
  """No gradient arrives for the fp32 output: the early return has one entry per forward argument (16 operands,
  the two handover objects, the three handed-in tensors) and launches nothing."""
  grads = mc_bottleneck._Unit.backward(None, None, None, None)
  assert len(grads) == 21 and all(g is None for g in grads)
  assert trace == []


@pytest.mark.parametrize('taps', [1, 9])
@pytest.mark.parametrize('need_x', [True, False])
def test_conv_bn_act(trace, taps, need_x):
  k = 3 if taps == 9 else 1
  conv = torch.nn.Conv2d(128, 64, k, padding=2 * (k // 2), dilation=2, bias=False)
  bn = _bn(64).train()
  x = _input(128, requires_grad=need_x)
  y = mc_bottleneck.conv_bn_act(conv, bn, x)
  assert trace == ['hl8_from_f32()', 'hl8_weight_set(1)', 'conv_hl8_stats(%d)' % taps, 'bn_fwd_hl8(chunks,relu,f32)']
  assert len(y.grad_fn.saved_tensors) == 11
  assert y.shape == (N, 64, H, W)
  del trace[:]
  y.sum().backward()
  assert trace == ['bn_bwd_hl8()', 'conv_wgrad_hl8(%d)' % taps] + (['conv_hl8(%d)' % taps] if need_x else [])
  _check_grads([conv, bn], x, need_x)
