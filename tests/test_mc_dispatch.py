"""Host-side dispatch of the matrix-core bottleneck units (no GPU): which units qualify, and that
everything else stays on the framework ops."""
import pytest
import torch

from spml_amd import _ffi, mc_bottleneck
from spml_amd.models.backbones.resnet import Bottleneck, ResnetBackbone
from spml_amd.models.heads.spp import ASPP, _dilated_sum_available


def test_supported_shapes_follow_the_kernel_tiling():
  assert _ffi.conv_hl8_supported(1024, 256, 1) and _ffi.conv_hl8_supported(256, 256, 9)
  assert _ffi.conv_hl8_supported(1024, 128, 1) and _ffi.conv_hl8_supported(2048, 64, 9)   # narrow tiles
  assert not _ffi.conv_hl8_supported(1024, 96, 1)           # 64-column granularity
  assert not _ffi.conv_hl8_supported(1000, 256, 1)          # 16-channel k steps
  assert not _ffi.conv_hl8_supported(256, 256, 25)
  assert _ffi.conv_wgrad_hl8_supported(1024, 256, 1) and _ffi.conv_wgrad_hl8_supported(128, 256, 9)
  assert not _ffi.conv_wgrad_hl8_supported(64, 256, 9)       # 128-channel granularity


def test_cpu_nchw_eval_and_strided_units_stay_on_the_framework():
  blk = Bottleneck(1024, 256, 1, dilation=2).train()
  x = torch.randn(1, 1024, 5, 5)
  assert not mc_bottleneck.available(blk, x)                # CPU tensor
  y = blk(x)                                                # ... and the framework path still works
  assert y.shape == x.shape
  meta = torch.empty(1, 1024, 5, 5, device='meta')
  assert not mc_bottleneck.available(blk, meta)


def test_only_res4_and_res5_units_qualify_by_shape():
  """Channel counts of the DeepLab-v2 backbone: res4 / res5 units tile (256-multiples), the stride-1 units
  of res3 run the 128-wide tiles, res2 does not tile, the stride-2 unit never does."""
  net = ResnetBackbone([3, 4, 23, 3], [1, 2, 1, 1], [1, 1, 2, 4])

  def shape_ok(b):
    convs = [b.conv1, b.conv2, b.conv3] + ([b.downsample[0]] if b.downsample is not None else [])
    return b.stride == 1 and all(
        _ffi.conv_hl8_supported(c.in_channels, c.out_channels, c.kernel_size[0] * c.kernel_size[1]) and
        _ffi.conv_hl8_supported(c.out_channels, c.in_channels, c.kernel_size[0] * c.kernel_size[1]) and
        _ffi.conv_wgrad_hl8_supported(c.in_channels, c.out_channels, c.kernel_size[0] * c.kernel_size[1])
        for c in convs)
  assert not any(shape_ok(b) for b in list(net.res2))                    # 64-channel convolutions
  assert [shape_ok(b) for b in net.res3] == [False, True, True, True]   # 128-wide tiles; unit 0 has stride 2
  assert all(shape_ok(b) for b in list(net.res4) + list(net.res5))


def test_aspp_fused_data_gradient_needs_gpu_channels_last_and_bare_branches():
  head = ASPP(256, 64, bn=False, relu=False)
  x = torch.randn(1, 256, 9, 9, requires_grad=True)
  assert not _dilated_sum_available(x, [b[0] for b in (head.aspp_1, head.aspp_2, head.aspp_3, head.aspp_4)])
  out = head(x)                                             # framework path on CPU
  out.sum().backward()
  assert x.grad is not None and out.shape == (1, 64, 9, 9)
  with_bn = ASPP(256, 64, bn=True, relu=True)
  assert with_bn(torch.randn(2, 256, 9, 9)).shape == (2, 64, 9, 9)


# ---------------------------------------------------------------------------
# the three predicates of spml_amd/mc_bottleneck.py, as a table.  They only read attributes of the input, so a stand-in
# for a channels-last fp32 GPU tensor reaches every branch without a GPU.
class _GpuInput(object):
  is_cuda, dtype = True, torch.float32

  def __init__(self, requires_grad=True, channels_last=True):
    self.requires_grad, self.channels_last = requires_grad, channels_last

  def dim(self):
    return 4

  def is_contiguous(self, memory_format=torch.contiguous_format):
    return self.channels_last == (memory_format is torch.channels_last)


def _unit(inplanes, planes, downsample=False, stride=1):
  from spml_amd.models.backbones.resnet import _bn
  ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, bias=False), _bn(planes * 4)) if downsample else None
  return Bottleneck(inplanes, planes, stride, dilation=2, downsample=ds)


def _frozen(blk):
  for p in blk.parameters():
    p.requires_grad_(False)
  return blk


def _with(blk, **replace):
  for name, module in replace.items():
    setattr(blk, name, module)
  return blk


_C, _B = torch.nn.Conv2d, torch.nn.BatchNorm2d
TRAIN, EVAL, NEITHER = 'train', 'eval', 'neither'
# name -> (unit, input, environment, which path takes it).  'train': `available` in training mode (autograd on or
# off), nothing else; 'eval': additionally `eval_available` in eval mode without autograd.  `available` is False in eval
# mode and `eval_available` is False in training mode or with autograd on, for every row.
UNIT_TABLE = {
    'res4': (lambda: _unit(1024, 256), {}, {}, EVAL),
    'res4 with downsample': (lambda: _unit(512, 256, True), {}, {}, EVAL),
    'res3': (lambda: _unit(512, 128), {}, {}, EVAL),
    'res2': (lambda: _unit(256, 64), {}, {}, NEITHER),
    'switched off': (lambda: _unit(1024, 256), {}, {'SPML_NO_MC_CONV': '1'}, NEITHER),
    'NCHW input': (lambda: _unit(1024, 256), {'channels_last': False}, {}, NEITHER),
    'stride 2': (lambda: _unit(1024, 256, stride=2), {}, {}, NEITHER),
    'res3, narrow units off': (lambda: _unit(512, 128), {}, {'SPML_MC_NARROW_UNITS': '0'}, NEITHER),
    'res4, narrow units off': (lambda: _unit(1024, 256), {}, {'SPML_MC_NARROW_UNITS': '0'}, EVAL),
    'frozen res2': (lambda: _frozen(_unit(256, 64)), {'requires_grad': False}, {}, NEITHER),
    'frozen res2, opted in': (lambda: _frozen(_unit(256, 64)), {'requires_grad': False},
                              {'SPML_MC_FROZEN_UNITS': '1'}, TRAIN),
    'frozen res4': (lambda: _frozen(_unit(1024, 256)), {'requires_grad': False}, {}, EVAL),
    'dilation != padding': (lambda: _with(_unit(1024, 256), conv2=_C(256, 256, 3, padding=1, dilation=2, bias=False)),
                            {}, {}, NEITHER),
    'anisotropic dilation': (lambda: _with(_unit(1024, 256),
                                           conv2=_C(256, 256, 3, padding=(2, 3), dilation=(2, 3), bias=False)),
                             {}, {}, NEITHER),
    'biased convolution': (lambda: _with(_unit(1024, 256), conv1=_C(1024, 256, 1, bias=True)), {}, {}, NEITHER),
    'grouped convolution': (lambda: _with(_unit(1024, 256), conv3=_C(256, 1024, 1, groups=2, bias=False)), {}, {},
                            NEITHER),
    '5x5 convolution': (lambda: _with(_unit(1024, 256), conv2=_C(256, 256, 5, padding=4, dilation=2, bias=False)), {},
                        {}, NEITHER),
    'momentum=None': (lambda: _with(_unit(1024, 256), bn2=_B(256, momentum=None)), {}, {}, NEITHER),
    'no affine': (lambda: _with(_unit(1024, 256), bn3=_B(1024, affine=False)), {}, {}, NEITHER),
    'no running statistics': (lambda: _with(_unit(1024, 256), bn1=_B(256, track_running_stats=False)), {}, {}, NEITHER),
    'padded 1x1 (the unit does not look)': (lambda: _with(_unit(1024, 256), conv1=_C(1024, 256, 1, padding=1, bias=False)),
                                            {}, {}, EVAL),
    '1000 input channels': (lambda: _unit(1000, 256), {}, {}, NEITHER),
}


@pytest.mark.parametrize('name', sorted(UNIT_TABLE))
def test_unit_predicates(name, monkeypatch):
  make, x_kw, env, path = UNIT_TABLE[name]
  for switch in ('SPML_NO_MC_CONV', 'SPML_MC_NARROW_UNITS', 'SPML_MC_FROZEN_UNITS'):
    monkeypatch.delenv(switch, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  blk, x = make(), _GpuInput(**x_kw)
  for training in (True, False):
    blk.train(training)
    for grad in (True, False):
      with torch.set_grad_enabled(grad):
        got = (mc_bottleneck.available(blk, x), mc_bottleneck.eval_available(blk, x))
      want = (training and path != NEITHER, not training and not grad and path == EVAL)
      assert got == want, (training, grad)
      assert blk.training == training


CONV_TABLE = {
    'pyramid head 3x3': (lambda: (_C(4096, 512, 3, padding=12, dilation=12, bias=False), _B(512)), {}, {}, True),
    '1x1': (lambda: (_C(512, 256, 1, bias=False), _B(256)), {}, {}, True),
    'input without gradient': (lambda: (_C(512, 256, 1, bias=False), _B(256)), {'requires_grad': False}, {}, True),
    'switched off': (lambda: (_C(512, 256, 1, bias=False), _B(256)), {}, {'SPML_NO_MC_CONV': '1'}, False),
    'narrow units off (units only)': (lambda: (_C(512, 128, 1, bias=False), _B(128)), {}, {'SPML_MC_NARROW_UNITS': '0'},
                                      True),
    'NCHW input': (lambda: (_C(512, 256, 1, bias=False), _B(256)), {'channels_last': False}, {}, False),
    'dilation != padding': (lambda: (_C(512, 256, 3, padding=1, dilation=2, bias=False), _B(256)), {}, {}, False),
    'anisotropic dilation': (lambda: (_C(512, 256, 3, padding=(2, 3), dilation=(2, 3), bias=False), _B(256)), {}, {},
                             False),
    'padded 1x1': (lambda: (_C(512, 256, 1, padding=1, bias=False), _B(256)), {}, {}, False),
    'biased convolution': (lambda: (_C(512, 256, 1, bias=True), _B(256)), {}, {}, False),
    'stride 2': (lambda: (_C(512, 256, 1, stride=2, bias=False), _B(256)), {}, {}, False),
    'momentum=None (not asked for here)': (lambda: (_C(512, 256, 1, bias=False), _B(256, momentum=None)), {}, {}, True),
    'no affine': (lambda: (_C(512, 256, 1, bias=False), _B(256, affine=False)), {}, {}, False),
    '64 input channels, 3x3': (lambda: (_C(64, 256, 3, padding=1, bias=False), _B(256)), {}, {}, False),
}


@pytest.mark.parametrize('name', sorted(CONV_TABLE))
def test_conv_bn_act_predicate(name, monkeypatch):
  make, x_kw, env, want = CONV_TABLE[name]
  monkeypatch.delenv('SPML_NO_MC_CONV', raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  (conv, bn), x = make(), _GpuInput(**x_kw)
  for training in (True, False):
    bn.train(training)
    for grad in (True, False):
      with torch.set_grad_enabled(grad):
        assert mc_bottleneck.conv_bn_act_available(conv, bn, x) == (want and training and grad), (training, grad)


def test_eval_available_does_not_write_the_training_flag():
  class ReadOnly(Bottleneck):
    training = property(lambda self: False, lambda self, value: pytest.fail('eval_available wrote block.training'))

  blk = _unit(1024, 256).eval()
  blk.__class__ = ReadOnly
  with torch.no_grad():
    assert mc_bottleneck.eval_available(blk, _GpuInput())
    assert not mc_bottleneck.eval_available(blk, _GpuInput(channels_last=False))


# ---------------------------------------------------------------------------
# the route of the image-similarity term (spml_amd/models/predictions/segsort.py): (on the GPU, the images' pixels one
# contiguous run, the batched kernels cover the loss, environment) -> (shared prototypes, batched, side streams,
# record_stream calls) and the path name
IMG_SIM_TABLE = [
    ((True, True, True, {}), (True, True, 0, False), 'batched'),
    ((True, True, False, {}), (True, False, 4, True), 'looped/shared-protos/streams=4'),
    ((True, False, True, {}), (False, False, 4, True), 'looped/per-image-protos/streams=4'),
    ((False, True, True, {}), (True, False, 0, False), 'looped/shared-protos/streams=0'),
    ((False, False, True, {}), (False, False, 0, False), 'looped/per-image-protos/streams=0'),
    ((True, True, True, {'SPML_IMG_SIM_BATCHED': '0'}), (True, False, 4, True), 'looped/shared-protos/streams=4'),
    ((True, True, True, {'SPML_IMG_SIM_BATCHED': '1'}), (True, True, 0, False), 'batched'),
    ((True, True, True, {'SPML_IMG_SIM_BATCHED_PROTOS': '0'}), (False, False, 4, True),
     'looped/per-image-protos/streams=4'),
    ((False, True, True, {'SPML_IMG_SIM_BATCHED_PROTOS': '0'}), (False, False, 0, False),
     'looped/per-image-protos/streams=0'),
    ((True, True, True, {'SPML_IMG_SIM_STREAMS': '4'}), (True, False, 4, True), 'looped/shared-protos/streams=4'),
    ((True, True, True, {'SPML_IMG_SIM_STREAMS': '1'}), (True, False, 0, False), 'looped/shared-protos/streams=0'),
    ((True, True, True, {'SPML_IMG_SIM_STREAMS': '0'}), (True, False, 0, False), 'looped/shared-protos/streams=0'),
    ((True, True, True, {'SPML_IMG_SIM_STREAMS': '8'}), (True, False, 8, True), 'looped/shared-protos/streams=8'),
    ((False, True, True, {'SPML_IMG_SIM_STREAMS': '8'}), (True, False, 0, False), 'looped/shared-protos/streams=0'),
    ((True, True, True, {'SPML_IMG_SIM_RECORD_STREAM': '0'}), (True, True, 0, False), 'batched'),
    ((True, True, True, {'SPML_IMG_SIM_BATCHED': '0', 'SPML_IMG_SIM_RECORD_STREAM': '0'}), (True, False, 4, False),
     'looped/shared-protos/streams=4'),
    ((True, True, True, {'SPML_IMG_SIM_STREAMS': '8', 'SPML_IMG_SIM_RECORD_STREAM': '0'}), (True, False, 8, False),
     'looped/shared-protos/streams=8'),
    ((True, True, True, {'SPML_IMG_SIM_BATCHED_PROTOS': '0', 'SPML_IMG_SIM_BATCHED': '0', 'SPML_IMG_SIM_STREAMS': '0',
                         'SPML_IMG_SIM_RECORD_STREAM': '0'}), (False, False, 0, False),
     'looped/per-image-protos/streams=0'),
]


@pytest.mark.parametrize('row', range(len(IMG_SIM_TABLE)))
def test_img_sim_route(row, monkeypatch):
  from spml_amd.models.predictions import segsort as head
  (on_gpu, contiguous, covered, env), want, name = IMG_SIM_TABLE[row]
  for switch in ('SPML_IMG_SIM_BATCHED_PROTOS', 'SPML_IMG_SIM_BATCHED', 'SPML_IMG_SIM_STREAMS',
                 'SPML_IMG_SIM_RECORD_STREAM'):
    monkeypatch.delenv(switch, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  route = head._img_sim_route(on_gpu, contiguous, covered)
  assert tuple(route) == want
  assert (route.shared_protos, route.batched, route.streams, route.record_stream) == want
  assert head.img_sim_path_name(route) == name
  assert head._img_sim_route(on_gpu, contiguous, covered, env=env) == route      # (the environment handed in)


def _aspp_flags_before_the_routes_had_names(cin, cout, branches, dilations):
  """The expressions `_DilatedSum.forward` evaluated in line before `_aspp_route`, word for word -> (wide, fwd_mc,
  narrow_wgrad, keeps the hl8 copy, gemm forward)."""
  import os
  wide = _ffi.conv_hl8_supported(cin, cout, 9) and _ffi.conv_wgrad_hl8_supported(cin, cout, 9)
  fwd_mc = wide or (_ffi.conv_hl8_supported(cin, cout, 9) and os.environ.get('SPML_ASPP_FWD_MC') != '0')
  narrow_wgrad = (not wide and _ffi.conv_wgrad_pyramid_hl8_supported(cin, cout, branches) and
                  all(1 <= d <= 255 for d in dilations) and os.environ.get('SPML_ASPP_WGRAD_MC') != '0')
  gemm = bool(fwd_mc and not wide and os.environ.get('SPML_ASPP_FWD_GEMM') != '0' and
              _ffi.conv_hl8_pyramid_forward_gemm_supported(cin, cout, branches) and
              all(1 <= d <= 255 for d in dilations))
  return wide, fwd_mc, narrow_wgrad, wide or narrow_wgrad, gemm


_D4 = (6, 12, 18, 24)
# (cin, cout, dilations, environment) -> (forward, weight gradients, keeps the hl8 copy), path name
ASPP_TABLE = [
    ((256, 64, _D4, {}), ('gemm-gather', 'pyramid', True), 'fwd=gemm-gather wgrad=pyramid'),
    ((2048, 64, _D4, {}), ('gemm-gather', 'pyramid', True), 'fwd=gemm-gather wgrad=pyramid'),
    ((256, 256, _D4, {}), ('taps36', 'per-branch', True), 'fwd=taps36 wgrad=per-branch'),
    ((256, 64, (6, 12, 18, 300), {}), ('taps36', 'library', False), 'fwd=taps36 wgrad=library'),
    ((256, 256, (6, 12, 18, 300), {}), ('taps36', 'per-branch', True), 'fwd=taps36 wgrad=per-branch'),
    ((256, 64, _D4, {'SPML_ASPP_FWD_GEMM': '0'}), ('taps36', 'pyramid', True), 'fwd=taps36 wgrad=pyramid'),
    ((256, 64, _D4, {'SPML_ASPP_FWD_MC': '0'}), ('library', 'pyramid', True), 'fwd=library wgrad=pyramid'),
    ((256, 64, _D4, {'SPML_ASPP_WGRAD_MC': '0'}), ('gemm-gather', 'library', False), 'fwd=gemm-gather wgrad=library'),
    ((2048, 64, _D4, {'SPML_ASPP_FWD_MC': '0', 'SPML_ASPP_WGRAD_MC': '0'}), ('library', 'library', False),
     'fwd=library wgrad=library'),
    ((256, 256, _D4, {'SPML_ASPP_FWD_MC': '0', 'SPML_ASPP_FWD_GEMM': '0', 'SPML_ASPP_WGRAD_MC': '0'}),
     ('taps36', 'per-branch', True), 'fwd=taps36 wgrad=per-branch'),
    ((256, 32, _D4, {}), ('library', 'library', False), 'fwd=library wgrad=library'),      # no 32-column tiles
]


@pytest.mark.parametrize('row', range(len(ASPP_TABLE)))
def test_aspp_route(row, monkeypatch):
  from spml_amd.models.heads import spp
  (cin, cout, dilations, env), want, name = ASPP_TABLE[row]
  for switch in ('SPML_ASPP_FWD_MC', 'SPML_ASPP_FWD_GEMM', 'SPML_ASPP_WGRAD_MC'):
    monkeypatch.delenv(switch, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  route = spp._aspp_route(cin, cout, 4, dilations)
  assert (route.forward, route.wgrad, route.keep_xh) == want
  assert spp.aspp_path_name(route) == name
  wide, fwd_mc, narrow_wgrad, keeps, gemm = _aspp_flags_before_the_routes_had_names(cin, cout, 4, dilations)
  assert route.forward == ('gemm-gather' if gemm else 'taps36' if fwd_mc else 'library')
  assert route.wgrad == ('per-branch' if wide else 'pyramid' if narrow_wgrad else 'library')
  assert route.keep_xh == keeps
