"""Stride-1 bottleneck unit of the ResNet backbone (spml/models/backbones/resnet.py:11-63) on the
matrix-core convolutions of `csrc/conv.hip`.

The unit's three (four with a downsample branch) convolutions run as split-f16 implicit GEMMs at
fp32-class accuracy, and the batch norms between them hand the activations over in the split
("hl8") form directly:

    x (fp32 + hl8) -conv1-> a1 -bn1,relu-> y1 (hl8 only) -conv2-> a2 -bn2,relu-> y2 (hl8 only)
      -conv3-> a3 -bn3 (+ identity), relu-> out (fp32 + hl8)

Backward mirrors it: every batch-norm backward writes the gradient of its convolution as hl8
(scaled by a bound derived from the per-channel extremes of the reduction pass), the data
gradients come from the same GEMM kernel on transposed weights, the gradient of the residual
branch is accumulated in the epilogue of conv1's data gradient.  One autograd node per unit.
SyncBatchNorm: per-rank statistics are combined between the statistics pass and the apply pass
(all_gather / all_reduce of [C]-sized vectors), as in `ops._BatchNormAct`.
"""
import collections
import inspect
import os
import types
import weakref
from itertools import islice

import torch
import torch.distributed as dist

from spml_amd import _ffi
from spml_amd._cache import BoundedCache


def _group_of(bn):
  if isinstance(bn, torch.nn.SyncBatchNorm) and dist.is_available() and dist.is_initialized():
    return bn.process_group if bn.process_group is not None else dist.group.WORLD
  return None


def _conv_tiles(conv, need_backward):
  """Stride-1, ungrouped, unbiased 1x1 / 9-tap convolution whose channel counts the forward kernel tiles -- and,
  need_backward, the data- and weight-gradient kernels.  (The padding tests differ and stay with the callers.)"""
  cin, cout, taps = conv.in_channels, conv.out_channels, conv.kernel_size[0] * conv.kernel_size[1]
  return (conv.stride == (1, 1) and conv.groups == 1 and conv.bias is None and taps in (1, 9) and
          _ffi.conv_hl8_supported(cin, cout, taps) and (not need_backward or (
              _ffi.conv_hl8_supported(cout, cin, taps) and _ffi.conv_wgrad_hl8_supported(cin, cout, taps))))


def available(block, x, allow_forward_only=True, training=True):
  """Channels-last fp32 GPU input, stride 1, channel counts the kernels tile; the block in training mode (or,
  training=False, in eval mode: `eval_available`)."""
  if os.environ.get('SPML_NO_MC_CONV') == '1' or not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
    return False
  if block.training != training or block.stride != 1 or not x.is_contiguous(memory_format=torch.channels_last):
    return False
  convs = [block.conv1, block.conv2, block.conv3] + ([block.downsample[0]] if block.downsample is not None else [])
  # units with 128-multiple channel counts only (res3) run the 128-wide tiles; SPML_MC_NARROW_UNITS=0 keeps
  # them on the framework convolutions
  if os.environ.get('SPML_MC_NARROW_UNITS') == '0' and any(
      (c.in_channels & 255) or (c.out_channels & 255) for c in convs):
    return False
  bns = [block.bn1, block.bn2, block.bn3] + ([block.downsample[1]] if block.downsample is not None else [])
  # a frozen unit behind a frozen input (res2 of the training recipes: in no optimizer group, batch norms still in
  # training mode) only ever runs forward: its channel counts need no data- / weight-gradient tiles.  Opt-in
  # (SPML_MC_FROZEN_UNITS=1): at 64 channels the 64-column tiles are no faster than the library -- 122.0 / 120.5 ms
  # per step with res2 on this path against 120.0 / 120.2 without, alternating runs on one box
  forward_only = allow_forward_only and not (torch.is_grad_enabled() and (x.requires_grad or any(
      p.requires_grad for m in convs + bns for p in m.parameters())))
  if forward_only and any(c.out_channels & 127 for c in convs) and os.environ.get('SPML_MC_FROZEN_UNITS') != '1':
    return False
  return (all((c.kernel_size == (1, 1) or (c.padding == c.dilation and c.dilation[0] == c.dilation[1])) and
              _conv_tiles(c, not forward_only) for c in convs) and
          all(b.affine and b.track_running_stats and b.momentum is not None for b in bns))


def eval_available(block, x):
  """Inference (eval mode, no autograd): same shape conditions as the training path."""
  return not torch.is_grad_enabled() and available(block, x, allow_forward_only=False, training=False)


def _touch(bn):
  """The fused kernels update the running statistics through raw pointers, which does not bump the
  tensors' version counters; the eval-mode fold below keys its cache on them."""
  if bn.running_mean is not None:
    torch.autograd.graph.increment_version((bn.running_mean, bn.running_var))


_folded = weakref.WeakKeyDictionary()       # conv module -> (version key, folded weights, bias); dies with the module


def _fold(conv, bn):
  """Batch norm in eval mode folded into the convolution: weight * (gamma * invstd)[co] in both hl8
  layouts + bias = beta - mean * gamma * invstd; cached per module (weakly: not carried by deepcopy / torch.save of
  the model) until a parameter or statistic changes (version counters; in-library updates go through `_touch`)."""
  ver = tuple(t._version for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)) + \
      (conv.weight.data_ptr(), bn.running_mean.data_ptr(), bn.eps)
  hit = _folded.get(conv)
  if hit is not None and hit[0] == ver:
    return hit[1], hit[2]
  scale = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
  w = conv.weight.detach() * scale.view(-1, 1, 1, 1)
  bias = (bn.bias.detach() - bn.running_mean * scale).contiguous()
  wf, _ = _ffi.hl8_weight(w)
  _folded[conv] = (ver, wf, bias)
  return wf, bias


def bottleneck_forward_eval(block, x):
  """Inference forward of one Bottleneck: three (four) matrix-core convolutions with the folded batch
  norm, ReLU and the residual add in their epilogues; one conversion pass between them."""
  n, cin, h, w = x.shape
  xh = getattr(x, '_spml_hl8', None) or _ffi.hl8_from_f32(x)
  dil = block.conv2.dilation[0]
  if block.downsample is not None:
    wd, bd = _fold(block.downsample[0], block.downsample[1])
    identity, _ = _ffi.conv_hl8_affine(xh, wd, bd, n, h, w, 1, relu=False, want_hl8=False)
  else:
    identity = x
  w1, b1 = _fold(block.conv1, block.bn1)
  w2, b2 = _fold(block.conv2, block.bn2)
  w3, b3 = _fold(block.conv3, block.bn3)
  _, y1 = _ffi.conv_hl8_affine(xh, w1, b1, n, h, w, 1)
  _, y2 = _ffi.conv_hl8_affine(y1, w2, b2, n, h, w, 9, dil)
  out, oh = _ffi.conv_hl8_affine(y2, w3, b3, n, h, w, 1, addend=identity)
  out._spml_hl8 = oh
  return out


def bump_counters(counters):
  """`num_batches_tracked += 1` for every batch norm of a unit in one launch."""
  if counters:
    torch._foreach_add_(counters, 1)


class _Bn(object):
  """Forward half of one batch norm inside the unit + what its backward needs."""

  def __init__(self, bn, a, rows, channels, residual=None, residual_bound=None, relu=True, want_f32=False,
               want_hl8=True, chunk_stats=None, counters=None, gathered=None):
    # gathered: (the ranks' [world, 3, C] statistics, this rank's [5, C]) if the caller has already exchanged them
    # (`sync_pair`: two independent batch norms share ONE all_gather)
    # counters (a list): the caller bumps `num_batches_tracked` of all its batch norms with ONE launch
    # (`bump_counters`) instead of one tiny kernel per layer (141 per training step)
    group = _group_of(bn)
    world = dist.get_world_size(group) if group is not None else 1
    self.count, self.group, self.world, self.relu = rows * world, group, world, relu
    # SyncBatchNorm: (count, mean, M2) of the ranks are gathered, pooled and finalised in one launch;
    # the channel extremes stay local (they only have to bound this rank's tensor)
    if world > 1 and gathered is None:
      st = _ffi.bn_stats_ext(a, rows, channels, chunk_stats=chunk_stats)
      allst = torch.empty((world * 3, channels), dtype=st.dtype, device=st.device)
      dist.all_gather_into_tensor(allst, st[:3], group=group)       # one contiguous [world, 3, C] block
      gathered = allst.view(world, 3, channels), st
    if bn.num_batches_tracked is not None:
      if counters is not None:
        counters.append(bn.num_batches_tracked)
      else:
        bn.num_batches_tracked.add_(1)
    if world == 1:                       # everything inside the library: three launches
      self.y, self.yh, self.bound, self.mask, self.saved = _ffi.bn_fwd_hl8(
          a, rows, channels, residual, residual_bound, bn.weight, bn.bias, bn.running_mean, bn.running_var,
          bn.momentum, bn.eps, relu, want_f32, want_hl8, relu, chunk_stats=chunk_stats)
      _touch(bn)
      return
    allst, st = gathered
    # (the pooled row count stays on the device: the ranks' counts may differ, batchnorm.py:124-145)
    mean, invstd, self.count = _ffi.bn_finalize_ranks(allst, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
    _touch(bn)
    cmax, cmin = st[3], st[4]
    self.y, self.yh, self.bound, self.mask = _ffi.bn_act_apply_hl8(
        a, rows, channels, residual, residual_bound, mean, invstd, bn.weight, bn.bias, cmax, cmin, relu,
        want_f32, want_hl8, want_mask=relu)
    self.saved = (mean, invstd, cmax, cmin)


class _BnRecord(collections.namedtuple(
    '_BnRecord', 'a gamma mean invstd cmax cmin mask count group world rows channels')):
  """What the backward of one batch norm reads: its input a (fp32 [rows, channels]), gamma, the four saved statistics,
  the ReLU mask bytes (None: no ReLU), and the row count (a device float where the ranks' counts were pooled) / process
  group / world size of the statistics."""
  __slots__ = ()
  saved = property(lambda self: (self.mean, self.invstd, self.cmax, self.cmin))


def _bn_backward(dy, bn, want_dres=False, want_dx_f32=False, chunk_stats=None):
  """-> (dx fp32 | None, dx hl8, d_residual | None, d_gamma, d_beta) of the batch norm of record `bn`
  chunk_stats: the chunk sums the data gradient that produced dy left (`_ffi.conv_hl8_bwd_stats`): the reduction
  pass over dy and a is replaced by their merge."""
  if bn.world == 1:
    dxh, dres, d_gamma, d_beta = _ffi.bn_bwd_hl8(dy, bn.mask, bn.a, bn.rows, bn.channels, bn.saved, bn.gamma,
                                                 want_dres=want_dres, chunk_stats=chunk_stats)
    return None, dxh, dres, d_gamma, d_beta
  st = _ffi.bn_act_bwd_reduce_ext(dy, None, bn.mask, bn.a, bn.rows, bn.channels, bn.mean, bn.invstd,
                                  chunk_stats=chunk_stats)                           # (sum dz, sum dz*xhat, max|dz|)
  local = st[:2].clone()                           # local sums: DDP averages parameter gradients
  d_beta, d_gamma = local[0], local[1]
  dist.all_reduce(st[:2], group=bn.group)
  dx, dxh, dres = _ffi.bn_act_bwd_apply_hl8(dy, None, bn.mask, bn.a, bn.rows, bn.channels, bn.mean, bn.invstd,
                                            bn.gamma, st[0], st[1], st[2], bn.cmax, bn.cmin, bn.count,
                                            want_dx_f32=want_dx_f32, want_dx_hl8=True, want_dres=want_dres)
  return dx, dxh, dres, d_gamma, d_beta


def sync_pair(bn_a, a_a, chunk_a, bn_b, a_b, chunk_b, rows, channels):
  """Two synchronised batch norms over independent tensors of the same width (a unit's third convolution and its
  downsample convolution): the local statistics of both travel in ONE all_gather of [3, 2 C] per rank instead of two
  of [3, C].  -> (gathered_a, gathered_b) [world, 3, C] each, or (None, None) on the unsynchronised path."""
  group = _group_of(bn_a)
  if group is None or _group_of(bn_b) is not group or dist.get_world_size(group) == 1:
    return None, None
  world = dist.get_world_size(group)
  st_a = _ffi.bn_stats_ext(a_a, rows, channels, chunk_stats=chunk_a)
  st_b = _ffi.bn_stats_ext(a_b, rows, channels, chunk_stats=chunk_b)
  loc = torch.cat([st_a[:3], st_b[:3]], dim=1)                       # [3, 2 C]
  allst = torch.empty((world * 3, 2 * channels), dtype=loc.dtype, device=loc.device)
  dist.all_gather_into_tensor(allst, loc, group=group)
  allst = allst.view(world, 3, 2 * channels)
  return (allst[:, :, :channels].contiguous(), st_a), (allst[:, :, channels:].contiguous(), st_b)


def _bn_backward_pair(d_out, bn3, bnd):
  """Backward of a unit's third batch norm (+ identity, ReLU) and of its downsample batch norm (records bn3, bnd),
  synchronised: both see dz = d_out * mask3 (the downsample branch IS the residual), so both (sum dz, sum dz x-hat)
  pairs are reduced before ONE all_reduce of [2, 2 C], and the gradient of the residual branch is never materialised.
  -> what `_bn_backward` returns, for bn3 and for bnd (no fp32 dx, no d_residual)"""
  mask, rows, c = bn3.mask, bn3.rows, bn3.channels
  st3 = _ffi.bn_act_bwd_reduce_ext(d_out, None, mask, bn3.a, rows, c, bn3.mean, bn3.invstd)
  std = _ffi.bn_act_bwd_reduce_ext(d_out, None, mask, bnd.a, rows, c, bnd.mean, bnd.invstd)
  both = torch.cat([st3[:2], std[:2]], dim=1)                  # [2, 2 C]
  local = both.clone()                                        # local sums: DDP averages parameter gradients
  dist.all_reduce(both, group=bn3.group)
  _, da3, _ = _ffi.bn_act_bwd_apply_hl8(d_out, None, mask, bn3.a, rows, c, bn3.mean, bn3.invstd, bn3.gamma,
                                        both[0, :c].contiguous(), both[1, :c].contiguous(), st3[2], bn3.cmax,
                                        bn3.cmin, bn3.count)
  _, dad, _ = _ffi.bn_act_bwd_apply_hl8(d_out, None, mask, bnd.a, rows, c, bnd.mean, bnd.invstd, bnd.gamma,
                                        both[0, c:].contiguous(), both[1, c:].contiguous(), std[2], bnd.cmax,
                                        bnd.cmin, bn3.count)
  return (None, da3, None, local[1, :c], local[0, :c]), (None, dad, None, local[1, c:], local[0, c:])


_side_streams = BoundedCache(16)      # one HIP stream per device, created once (a device resource, not call state)


def _side_stream(device):
  """Second stream for the weight gradients: they are off the backward's critical path, and the
  HBM-bound batch-norm passes of the next convolution overlap with them on the same CUs."""
  if os.environ.get('SPML_WGRAD_STREAM') == '0':
    return None
  return _side_streams.get_or_make(device.index, lambda: torch.cuda.Stream(device=device))


def _wgrad(side, dy, x, n, h, w, taps, dil=1):
  """conv_wgrad_hl8 on the side stream (after everything queued so far on the current one)."""
  if side is None:
    return _ffi.conv_wgrad_hl8(dy, x, n, h, w, taps, dil)
  main = torch.cuda.current_stream()
  side.wait_stream(main)
  with torch.cuda.stream(side):
    dw = _ffi.conv_wgrad_hl8(dy, x, n, h, w, taps, dil)
  # both halves of dy are freed by the caller before the side stream is joined: the 512-byte
  # bound block is read by the LAST kernel of the side stream (conv_wgrad_reduce) and would
  # otherwise be handed to the next batch-norm backward's `bound` on the main stream
  dy.data.record_stream(side)
  dy.bound.record_stream(side)
  dw.record_stream(main)
  return dw


def handover_mode():
  """SPML_BN3_HANDOVER: 0 = every unit's bn3 backward reduces (d_out, a3, mask3) in a pass of its own; 1 (default) =
  the unit above leaves those sums in the epilogue of its last data gradient, whose output IS that d_out.  (Mode 2 of
  the plan -- the unit above also runs that bn3 backward before it joins its weight gradients -- did not separate from
  the run-to-run noise and is not built: profiles/bn3_handover.md.)"""
  return 0 if os.environ.get('SPML_BN3_HANDOVER') == '0' else 1


class _Handover(object):
  """What travels from a unit (the producer of an activation) to the unit that consumes it, and back in the backward
  pass.  Forward: references to the producer's bn3 operands (a3, mask3, the batch mean; the producer saves the same
  tensor objects, so no memory is added).  Backward: the consumer's last data gradient -- the producer's d_out -- with
  the chunk sums of the producer's bn3 backward its epilogue left.  The sums are only good for that very tensor:
  `take` hands them out once, and only if the gradient autograd delivers is the tensor `put` saw, unmodified (a second
  consumer of the activation makes autograd deliver a sum, i.e. another tensor)."""
  taken = 0                              # (class-wide: how many times handed sums were used)

  def __init__(self):
    self.bn3 = None                      # (a3, mask3, mean) of the producer
    self.dx = self.stats = self.version = None

  def put(self, dx, stats):
    self.dx, self.stats, self.version = dx, stats, dx._version

  def take(self, d_out):
    dx, stats, version = self.dx, self.stats, self.version
    self.dx = self.stats = self.version = None
    if dx is None or d_out._version != version or d_out.data_ptr() != dx.data_ptr() or d_out.shape != dx.shape or \
        d_out.stride() != dx.stride() or d_out.dtype != dx.dtype:
      return None
    _Handover.taken += 1
    return stats


def _save_named(ctx, **entries):
  """`ctx.save_for_backward` under names; `_saved_named` is the mirror.  An entry is a tensor, None, a tuple of
  tensors, an Hl8 (saved as its two tensors, (rows, channels) kept in the layout) or a _BnRecord (its seven tensors --
  six where there is no mask --, the rest of it kept in the layout).  Only tensors are saved, in the order given."""
  layout, tensors = [], []
  for name, v in entries.items():
    kind = type(v)
    if kind is _ffi.Hl8:
      make, parts, rest = kind, (v.data, v.bound), (v.rows, v.channels)
    elif kind is _BnRecord:
      k = 6 if v.mask is None else 7       # (its tensors lead the record; a None mask stays in the layout)
      make, parts, rest = kind, v[:k], v[k:]
    elif kind is tuple:
      make, parts, rest = (lambda *p: p), v, ()
    else:
      make, parts, rest = (lambda p=None: p), (() if v is None else (v,)), ()
    layout.append((name, make, len(parts), rest))
    tensors += parts
  ctx.saved_layout = layout
  ctx.save_for_backward(*tensors)


def _saved_named(ctx):
  it = iter(ctx.saved_tensors)
  return types.SimpleNamespace(**{name: make(*islice(it, k), *rest) for name, make, k, rest in ctx.saved_layout})


def _forward_stage(xh, wf, geom, taps, dil, bn, gamma, conv_out=None, **bn_args):
  """conv(xh, wf) -> batch norm `bn` (+ residual, ReLU: bn_args as for `_Bn`) -> (_Bn, its _BnRecord).  Where the
  tiling allows it (256-column tiles) the convolution's epilogue leaves the chunk statistics and the batch norm does
  not read the tensor for them.  conv_out: (a, chunk statistics) of a convolution the caller has already launched."""
  n, h, w = geom
  a, st = conv_out or _ffi.conv_hl8_stats(xh, wf, n, h, w, taps, dil)
  nb = _Bn(bn, a, n * h * w, wf.rows, chunk_stats=st, **bn_args)
  return nb, _BnRecord(a, gamma, *nb.saved, nb.mask, nb.count, nb.group, nb.world, n * h * w, wf.rows)


def _backward_stage(side, dy, bn, xh, geom, taps, dil, dgrad, done=None, **bn_args):
  """Backward of one conv -> bn stage: batch-norm backward of record `bn` (bn_args as for `_bn_backward`; done: its
  result where the caller has run it) -> weight gradient against the stage's input xh on the side stream -> the data
  gradient `dgrad(da)` (None: none) -> (what dgrad returned, d_residual | None, dw, d_gamma, d_beta); da is dropped."""
  _, da, dres, dg, db = done or _bn_backward(dy, bn, **bn_args)
  dw = _wgrad(side, da, xh, *geom, taps, dil)
  return (dgrad(da) if dgrad is not None else None), dres, dw, dg, db


class _Unit(torch.autograd.Function):

  @staticmethod
  def forward(ctx, block, x, xh_data, xh_bound, w1, g1, b1, w2, g2, b2, w3, g3, b3, wd, gd, bd, hand_out=None,
              hand_in=None, below_a3=None, below_mask3=None, below_mean3=None):
    # hand_out: this unit's _Handover (filled here); hand_in + below_* (its three tensors, the bn3 operands of the unit
    # that produced x), if any
    n, cin, h, w = x.shape
    geom, dil = (n, h, w), block.conv2.dilation[0]
    xh = _ffi.Hl8(xh_data, xh_bound, n * h * w, cin) if xh_data is not None else _ffi.hl8_from_f32(x)
    (w1f, w1t), (w2f, w2t), (w3f, w3t), *wds = _ffi.hl8_weight_set([w1, w2, w3] + ([wd] if wd is not None else []))
    counters = []
    n1, bn1 = _forward_stage(xh, w1f, geom, 1, 1, block.bn1, g1, counters=counters)
    n2, bn2 = _forward_stage(n1.yh, w2f, geom, 9, dil, block.bn2, g2, counters=counters)
    out3 = _ffi.conv_hl8_stats(n2.yh, w3f, n, h, w, 1)
    nd = wdt = bnd = ex3 = None            # (ex3: exchanged statistics of bn3, if it shares the exchange)
    if wd is not None:
      (wdf, wdt), = wds
      outd = _ffi.conv_hl8_stats(xh, wdf, n, h, w, 1)
      # the statistics of the third convolution and of the downsample convolution are independent: one exchange
      ex3, exd = sync_pair(block.bn3, *out3, block.downsample[1], *outd, n * h * w, w3f.rows)
      nd, bnd = _forward_stage(xh, wdf, geom, 1, 1, block.downsample[1], gd, conv_out=outd, relu=False, want_f32=True,
                               want_hl8=False, counters=counters, gathered=exd)
    residual, res_bound = (x, xh.bound) if nd is None else (nd.y, nd.bound)
    n3, bn3 = _forward_stage(n2.yh, w3f, geom, 1, 1, block.bn3, g3, conv_out=out3, residual=residual,
                             residual_bound=res_bound, want_f32=True, counters=counters, gathered=ex3)
    bump_counters(counters)
    ctx.block, ctx.geom, ctx.has_downsample = block, (n, h, w, dil), wd is not None
    ctx.hand_in = ctx.hand_out = below_bn3 = None
    if hand_in is not None and below_a3 is not None and n3.world == 1 and tuple(below_a3.shape) == tuple(x.shape):
      ctx.hand_in, below_bn3 = hand_in, (below_a3, below_mask3, below_mean3)
    if hand_out is not None and n3.world == 1 and n3.mask is not None:
      ctx.hand_out, hand_out.bn3 = hand_out, (bn3.a, bn3.mask, bn3.mean)
    _save_named(ctx, xh=xh, y1h=n1.yh, y2h=n2.yh, w1t=w1t, w2t=w2t, w3t=w3t, wdt=wdt, bn1=bn1, bn2=bn2, bn3=bn3,
                bnd=bnd, below_bn3=below_bn3)
    ctx.mark_non_differentiable(n3.yh.data, n3.yh.bound)
    ctx.set_materialize_grads(False)       # no zero-filled 0.3-0.5 GB "gradients" for the hl8 side outputs
    return n3.y, n3.yh.data, n3.yh.bound

  @staticmethod
  def backward(ctx, d_out, _unused_data, _unused_bound):
    g = dict.fromkeys(_UNIT_GRADS)         # one gradient per forward argument, filled by name
    if d_out is None:
      return tuple(g.values())
    s = _saved_named(ctx)
    # the chunk sums of bn3's backward, if the unit above left them with this very d_out (checked before any copy);
    # the forward references have served
    handed = ctx.hand_out.take(d_out) if ctx.hand_out is not None else None
    if ctx.hand_out is not None:
      ctx.hand_out.bn3 = None
    n, h, w, dil = ctx.geom
    geom, has_ds = (n, h, w), ctx.has_downsample
    if not d_out.is_contiguous(memory_format=torch.channels_last):
      d_out = d_out.contiguous(memory_format=torch.channels_last)
    need_x = ctx.needs_input_grad[_UNIT_GRADS.index('x')]
    side = _side_stream(d_out.device)
    # bn3 (+ identity, relu)
    # the residual branch's gradient d_out * mask3 is only materialised for the downsample branch; the
    # plain identity takes it in the epilogue of conv1's data gradient (masked addend)
    done3 = doned = None
    if has_ds and s.bn3.world > 1 and s.bnd.group is s.bn3.group:     # synchronised: both reductions, ONE all_reduce
      done3, doned = _bn_backward_pair(d_out, s.bn3, s.bnd)
    # dy2 / dy1 are the dy of bn2 / bn1: where the tiling allows it (256-column tiles) the data gradient's epilogue
    # leaves the chunk sums of that batch norm's backward and the reduction pass over (dy, a, mask) is not run
    stats = _ffi.conv_hl8_bwd_stats
    dgrad = lambda wt, taps, dil, bn: lambda da: stats(da, wt, n, h, w, taps, dil, bn.a, bn.mask, bn.mean)
    (dy2, c2), dres, g['w3'], g['g3'], g['b3'] = _backward_stage(
        side, d_out, s.bn3, s.y2h, geom, 1, 1, dgrad(s.w3t, 1, 1, s.bn2), done=done3, want_dres=has_ds,
        chunk_stats=handed)
    del done3                              # (da3, as the stages release their da on return)
    (dy1, c1), _, g['w2'], g['g2'], g['b2'] = _backward_stage(
        side, dy2, s.bn2, s.y1h, geom, 9, dil, dgrad(s.w2t, 9, dil, s.bn1), chunk_stats=c2)
    del dy2
    # the last data gradient (conv1's + the masked d_out of the identity branch; with a downsample branch the second
    # launch, which adds the first one's result unmasked) is the d_out of the unit below: its epilogue leaves the chunk
    # sums of that unit's bn3 backward (dz = dx * mask3 of that unit), which then skips its reduction pass over
    # (d_out, a3, mask3)
    if s.below_bn3 is not None and need_x and handover_mode():
      last = lambda dy, wt, **kw: _ffi.conv_hl8_bwd_stats(dy, wt, n, h, w, 1, 1, *s.below_bn3, **kw)
    else:
      last = lambda dy, wt, **kw: (_ffi.conv_hl8(dy, wt, n, h, w, 1, **kw), None)
    if has_ds:        # conv1's data gradient waits for the downsample branch's weight gradient: stage 1 hands da1 out
      da1, _, g['w1'], g['g1'], g['b1'] = _backward_stage(side, dy1, s.bn1, s.xh, geom, 1, 1, lambda da: da,
                                                          chunk_stats=c1)
      dgrad_x = lambda dad: last(dad, s.wdt, addend=_ffi.conv_hl8(da1, s.w1t, n, h, w, 1))
      dxc, _, g['wd'], g['gd'], g['bd'] = _backward_stage(side, dres, s.bnd, s.xh, geom, 1, 1,
                                                          dgrad_x if need_x else None, done=doned)
    else:
      dgrad_x = lambda da1: last(da1, s.w1t, addend=d_out, addend_mask=s.bn3.mask)
      dxc, _, g['w1'], g['g1'], g['b1'] = _backward_stage(side, dy1, s.bn1, s.xh, geom, 1, 1,
                                                          dgrad_x if need_x else None, chunk_stats=c1)
    g['x'], cx = dxc or (None, None)
    if cx is not None:
      ctx.hand_in.put(g['x'], cx)
    if side is not None:
      torch.cuda.current_stream().wait_stream(side)      # the weight gradients are consumed on this stream
    return tuple(g.values())



class _ConvBnAct(torch.autograd.Function):
  """relu(bn(conv(x))) for ONE stride-1 convolution (1x1 or dilated 3x3) followed by a training-mode batch
  norm, on the same kernels as the units: the 3x3 convolution 4096 -> 512 that closes the pyramid-pooling head
  (spml/models/heads/spp.py:46-86) is 30 % of the DensePose step on the fp32 library (22 + 22 + 20 ms)."""

  @staticmethod
  def forward(ctx, conv, bn, x, weight, gamma, beta):
    n, _, h, w = x.shape
    taps, dil = weight.shape[2] * weight.shape[3], conv.dilation[0]
    xh = getattr(x, '_spml_hl8', None) or _ffi.hl8_from_f32(x)
    (wf, wt), = _ffi.hl8_weight_set([weight])
    nb, rec = _forward_stage(xh, wf, (n, h, w), taps, dil, bn, gamma, relu=True, want_f32=True, want_hl8=False)
    ctx.geom = (n, h, w, taps, dil)
    _save_named(ctx, xh=xh, wt=wt, bn=rec)
    return nb.y

  @staticmethod
  def backward(ctx, dy):
    g = dict.fromkeys(_CONV_BN_ACT_GRADS)
    n, h, w, taps, dil = ctx.geom
    s = _saved_named(ctx)
    if not dy.is_contiguous(memory_format=torch.channels_last):
      dy = dy.contiguous(memory_format=torch.channels_last)
    side = _side_stream(dy.device)
    dgrad = lambda da: _ffi.conv_hl8(da, s.wt, n, h, w, taps, dil)
    g['x'], _, g['weight'], g['gamma'], g['beta'] = _backward_stage(
        side, dy, s.bn, s.xh, (n, h, w), taps, dil,
        dgrad if ctx.needs_input_grad[_CONV_BN_ACT_GRADS.index('x')] else None)
    if side is not None:
      torch.cuda.current_stream().wait_stream(side)
    return tuple(g.values())


# one gradient per argument of forward (all but ctx), in this order
_UNIT_GRADS, _CONV_BN_ACT_GRADS = (tuple(inspect.signature(f.forward).parameters)[1:] for f in (_Unit, _ConvBnAct))


def conv_bn_act_available(conv, bn, x):
  """One stride-1 convolution + training-mode batch norm + ReLU on the matrix-core path: channels-last fp32
  GPU input, channel counts the forward, data-gradient and weight-gradient kernels tile."""
  if os.environ.get('SPML_NO_MC_CONV') == '1' or not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
    return False
  if not (bn.training and torch.is_grad_enabled() and x.is_contiguous(memory_format=torch.channels_last)):
    return False
  k = conv.kernel_size
  return (k in ((1, 1), (3, 3)) and conv.dilation[0] == conv.dilation[1] and
          conv.padding == tuple(d * (k[0] // 2) for d in conv.dilation) and bn.affine and bn.track_running_stats and
          _conv_tiles(conv, True))


def conv_bn_act(conv, bn, x):
  return _ConvBnAct.apply(conv, bn, x, conv.weight, bn.weight, bn.bias)


def bottleneck_forward(block, x):
  """Forward of one Bottleneck through the matrix-core path; the output tensor carries its hl8
  copy (attribute `_spml_hl8`) for the next unit."""
  xh = getattr(x, '_spml_hl8', None)
  ds = block.downsample
  hand = torch.is_grad_enabled() and handover_mode()
  hand_in, hand_out = (getattr(x, '_spml_handover', None), _Handover()) if hand else (None, None)
  out, oh, ob = _Unit.apply(
      block, x, None if xh is None else xh.data, None if xh is None else xh.bound,
      block.conv1.weight, block.bn1.weight, block.bn1.bias, block.conv2.weight, block.bn2.weight, block.bn2.bias,
      block.conv3.weight, block.bn3.weight, block.bn3.bias,
      None if ds is None else ds[0].weight, None if ds is None else ds[1].weight, None if ds is None else ds[1].bias,
      hand_out, hand_in, *(hand_in.bn3 if hand_in is not None and hand_in.bn3 is not None else (None,) * 3))
  out._spml_hl8 = _ffi.Hl8(oh, ob, out.shape[0] * out.shape[2] * out.shape[3], out.shape[1])
  if hand_out is not None and hand_out.bn3 is not None:
    out._spml_handover = hand_out          # (on the tensor object, like the hl8 copy: any op on `out` drops both)
  return out
