"""Launch trace of the ASPP head's `_DilatedSum` (spml_amd/models/heads/spp.py) on the CPU, in the manner of
tests/test_mc_unit_trace.py: the `_ffi` wrappers it calls are replaced by fakes that return zero tensors of the right
shapes and write down what they were called with (the `*_supported` predicates stay the library's own); the
framework's `conv2d` is recorded and passed on.  What is pinned: the sequence of calls of a forward + backward pass on
every route, the number of tensors the autograd node keeps, whether it keeps the input's hl8 copy, and which gradients
come back.  The expected sequences were recorded before the routes had names; they are written out here, not
generated."""
import pytest
import torch
import torch.nn.functional as F

from spml_amd import _ffi
from spml_amd.models.heads.spp import _DilatedSum

N, H, W = 1, 5, 4
DILATIONS = (6, 12, 18, 24)


@pytest.fixture
def trace(monkeypatch):
  calls = []
  for switch in ('SPML_ASPP_FWD_MC', 'SPML_ASPP_FWD_GEMM', 'SPML_ASPP_WGRAD_MC'):
    monkeypatch.delenv(switch, raising=False)

  def hl8(rows, channels):
    return _ffi.Hl8(torch.zeros(rows * channels * 4, dtype=torch.uint8), torch.zeros(1), rows, channels)

  def hl8_from_f32(x, rows=None, channels=None, bound=None):
    calls.append('hl8_from_f32')
    assert x.is_contiguous(memory_format=torch.channels_last)
    return hl8(x.shape[0] * x.shape[2] * x.shape[3], x.shape[1])

  def forward(name):
    def fake(x, weights, biases, dilations, n_img, h, w):
      calls.append('%s(%d)' % (name, len(weights)))
      assert x.rows == n_img * h * w and x.channels == weights[0].shape[1] and len(biases) == len(dilations) == len(weights)
      return torch.zeros((n_img, weights[0].shape[0], h, w)).contiguous(memory_format=torch.channels_last)
    return fake

  def conv_wgrad_pyramid_hl8(dy, x, n_img, h, w, dilations):
    calls.append('conv_wgrad_pyramid_hl8(%d)' % len(dilations))
    assert dy.rows == n_img * h * w == x.rows
    return list(torch.zeros((len(dilations), dy.channels, 3, 3, x.channels)).permute(0, 1, 4, 2, 3))

  def conv_wgrad_hl8(dy, x, n_img, h, w, taps, dilation=1):
    calls.append('conv_wgrad_hl8(%d,d=%d)' % (taps, dilation))
    assert dy.rows == n_img * h * w == x.rows
    return torch.zeros((dy.channels, x.channels, 3, 3)).contiguous(memory_format=torch.channels_last)

  def conv_hl8_pyramid_dgrad(dy, weights, dilations, n_img, h, w):
    calls.append('conv_hl8_pyramid_dgrad(%d)' % len(weights))
    assert dy.rows == n_img * h * w and dy.channels == weights[0].shape[0]
    return torch.zeros((n_img, weights[0].shape[1], h, w)).contiguous(memory_format=torch.channels_last)

  real_conv2d = F.conv2d

  def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    calls.append('conv2d(d=%d)' % dilation)
    return real_conv2d(x, weight, bias, stride, padding, dilation, groups)

  monkeypatch.setattr(_ffi, 'hl8_from_f32', hl8_from_f32)
  monkeypatch.setattr(_ffi, 'conv_hl8_pyramid_forward_gemm', forward('conv_hl8_pyramid_forward_gemm'))
  monkeypatch.setattr(_ffi, 'conv_hl8_pyramid_forward', forward('conv_hl8_pyramid_forward'))
  monkeypatch.setattr(_ffi, 'conv_wgrad_pyramid_hl8', conv_wgrad_pyramid_hl8)
  monkeypatch.setattr(_ffi, 'conv_wgrad_hl8', conv_wgrad_hl8)
  monkeypatch.setattr(_ffi, 'conv_hl8_pyramid_dgrad', conv_hl8_pyramid_dgrad)
  monkeypatch.setattr(F, 'conv2d', conv2d)
  return calls


def _head(cin, cout, bias=(True, True, True, True)):
  g = torch.Generator().manual_seed(cin + cout)
  ws = [(torch.randn(cout, cin, 3, 3, generator=g) * 0.01).requires_grad_(True) for _ in bias]
  bs = [torch.randn(cout, generator=g).requires_grad_(True) if b else None for b in bias]
  return ws, bs


def _run(trace, cin, cout, need_x=True, bias=(True, True, True, True), dilations=DILATIONS):
  """-> (forward calls, backward calls, saved tensors, hl8 copy kept, x.grad, [dw], [db])."""
  ws, bs = _head(cin, cout, bias)
  x = torch.randn(N, cin, H, W).contiguous(memory_format=torch.channels_last).requires_grad_(need_x)
  params = []
  for wt, b in zip(ws, bs):
    params += [wt, b]
  y = _DilatedSum.apply(x, dilations, *params)
  assert y.shape == (N, cout, H, W)
  fwd = list(trace)
  del trace[:]
  saved, kept = len(y.grad_fn.saved_tensors), y.grad_fn.xh is not None
  y.sum().backward()
  for wt in ws:
    assert wt.grad is not None and wt.grad.shape == wt.shape
  for b in bs:
    assert b is None or (b.grad is not None and b.grad.shape == b.shape)
  assert (x.grad is not None) == need_x
  return fwd, list(trace), saved, kept


FWD_LIBRARY = ['conv2d(d=6)', 'conv2d(d=12)', 'conv2d(d=18)', 'conv2d(d=24)']
WGRAD_PER_BRANCH = ['conv_wgrad_hl8(9,d=6)', 'conv_wgrad_hl8(9,d=12)', 'conv_wgrad_hl8(9,d=18)', 'conv_wgrad_hl8(9,d=24)']
DGRAD = ['conv_hl8_pyramid_dgrad(4)']


def test_narrow_head_default(trace):
  fwd, bwd, saved, kept = _run(trace, 256, 64)
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward_gemm(4)']
  assert bwd == ['hl8_from_f32', 'conv_wgrad_pyramid_hl8(4)'] + DGRAD
  assert (saved, kept) == (5, True)


def test_narrow_head_without_the_gemm_forward(trace, monkeypatch):
  monkeypatch.setenv('SPML_ASPP_FWD_GEMM', '0')
  fwd, bwd, saved, kept = _run(trace, 256, 64)
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward(4)']
  assert bwd == ['hl8_from_f32', 'conv_wgrad_pyramid_hl8(4)'] + DGRAD
  assert (saved, kept) == (5, True)


def test_narrow_head_with_the_library_forward(trace, monkeypatch):
  monkeypatch.setenv('SPML_ASPP_FWD_MC', '0')
  fwd, bwd, saved, kept = _run(trace, 256, 64)
  assert fwd == ['hl8_from_f32'] + FWD_LIBRARY            # (the hl8 copy: for the weight gradients)
  assert bwd == ['hl8_from_f32', 'conv_wgrad_pyramid_hl8(4)'] + DGRAD
  assert (saved, kept) == (5, True)


def test_narrow_head_with_the_library_weight_gradients(trace, monkeypatch):
  monkeypatch.setenv('SPML_ASPP_WGRAD_MC', '0')
  fwd, bwd, saved, kept = _run(trace, 256, 64)
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward_gemm(4)']
  assert bwd == ['hl8_from_f32'] + DGRAD                   # (the four convolution_backward calls are the framework's)
  assert (saved, kept) == (5, False)


def test_narrow_head_with_both_on_the_library(trace, monkeypatch):
  monkeypatch.setenv('SPML_ASPP_FWD_MC', '0')
  monkeypatch.setenv('SPML_ASPP_WGRAD_MC', '0')
  fwd, bwd, saved, kept = _run(trace, 256, 64)
  assert fwd == FWD_LIBRARY
  assert bwd == ['hl8_from_f32'] + DGRAD
  assert (saved, kept) == (5, False)


def test_dilation_beyond_the_one_launch_kernels(trace):
  fwd, bwd, saved, kept = _run(trace, 256, 64, dilations=(6, 12, 18, 300))
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward(4)']
  assert bwd == ['hl8_from_f32'] + DGRAD
  assert (saved, kept) == (5, False)


def test_wide_head(trace, monkeypatch):
  monkeypatch.setenv('SPML_ASPP_FWD_MC', '0')              # (a wide head does not ask)
  fwd, bwd, saved, kept = _run(trace, 256, 256)
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward(4)']
  assert bwd == ['hl8_from_f32'] + WGRAD_PER_BRANCH + DGRAD
  assert (saved, kept) == (5, True)


def test_input_that_needs_no_gradient(trace):
  fwd, bwd, saved, kept = _run(trace, 256, 64, need_x=False)
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward_gemm(4)']
  assert bwd == ['hl8_from_f32', 'conv_wgrad_pyramid_hl8(4)']
  assert (saved, kept) == (5, True)
  fwd, bwd, saved, kept = _run(trace, 256, 256, need_x=False)
  assert bwd == ['hl8_from_f32'] + WGRAD_PER_BRANCH


def test_branch_without_bias(trace):
  fwd, bwd, saved, kept = _run(trace, 256, 64, bias=(True, False, True, True))
  assert fwd == ['hl8_from_f32', 'conv_hl8_pyramid_forward_gemm(4)']
  assert bwd == ['hl8_from_f32', 'conv_wgrad_pyramid_hl8(4)'] + DGRAD
  assert (saved, kept) == (5, True)


def test_frozen_weights_launch_no_weight_gradient(trace):
  ws, bs = _head(256, 64)
  for t in ws + bs:
    t.requires_grad_(False)
  x = torch.randn(N, 256, H, W).contiguous(memory_format=torch.channels_last).requires_grad_(True)
  params = []
  for wt, b in zip(ws, bs):
    params += [wt, b]
  y = _DilatedSum.apply(x, DILATIONS, *params)
  del trace[:]
  out = _DilatedSum.backward(y.grad_fn, torch.ones_like(y))      # (the node is the context)
  assert trace == ['hl8_from_f32'] + DGRAD
  # the node hands back None for the dilations and for every parameter
  assert len(out) == 10 and out[0].shape == x.shape and all(g is None for g in out[1:])
