"""Stage-2 softmax classifier on frozen pixel embeddings.

Counterpart of `spml/models/predictions/softmax_classifier.py` (trained by
`pyscripts/train/train_classifier.py`): unit-normalised embedding -> 3x3 conv (2C, no
bias) -> BN -> ReLU -> dropout 0.65 -> 1x1 conv to `num_classes`; cross-entropy and pixel
accuracy at label resolution; labels >= num_classes count as ignored.

Inference (`pyscripts/inference/inference_softmax.py:126-137`): `accumulate_logits` adds one sliding-window crop's
logits into the full-resolution canvas through the HIP head (csrc/softmax_head.hip + the folded-BN matrix-core
convolution)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from spml_amd.nn.batchnorm import BatchNorm2d

import spml_amd.models.utils as model_utils
from spml_amd import _ffi, ops

_DROPOUT = 0.65


def _head(in_dim, num_classes):
  hidden = 2 * in_dim
  return nn.Sequential(
      nn.Conv2d(in_dim, hidden, 3, stride=1, padding=1, bias=False),
      BatchNorm2d(hidden),
      nn.ReLU(inplace=True),
      nn.Dropout(p=_DROPOUT),
      nn.Conv2d(hidden, num_classes, 1, stride=1, bias=True))


def fold_conv_bn(weight, bn):
  """Eval-mode batch norm folded into the bias-free convolution in front of it:
  `relu(conv(x, w') + b')` with w' = w * (gamma * invstd)[co], b' = beta - mean * gamma * invstd."""
  scale = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
  return weight.detach() * scale.view(-1, 1, 1, 1), (bn.bias.detach() - bn.running_mean * scale).contiguous()


HIP_HEAD_PATH = 'hip_head_f32mfma'
FRAMEWORK_HEAD_PATH = 'framework'


class SoftmaxClassifier(nn.Module):

  def __init__(self, config):
    super().__init__()
    self._inference_cache = None          # folded operands of the HIP head (prepare_inference)
    self.num_classes = config.dataset.num_classes
    self.ignore_index = config.dataset.semantic_ignore_index
    self.semantic_classifier = _head(config.network.embedding_dim, self.num_classes)
    self.semantic_loss = nn.CrossEntropyLoss(ignore_index=self.ignore_index)

  def _logits(self, embedding):
    unit = embedding / embedding.norm(dim=1, keepdim=True)
    return self.semantic_classifier(unit)

  def _supervise(self, logits, labels):
    """Cross-entropy + accuracy over the valid pixels, logits upsampled to the labels."""
    logits = ops.upsample_bilinear(logits, size=labels.shape[-2:])       # (deterministic mode: fixed-order backward)
    labels = torch.where(labels >= self.num_classes,
                         torch.full_like(labels, self.ignore_index), labels)
    labels = labels.squeeze(1).long()
    prediction = logits.argmax(dim=1)
    keep = labels != self.ignore_index
    accuracy = (prediction == labels)[keep].float().mean()
    if logits.is_cuda and _ffi.deterministic():
      # the framework's 2-D NLL forward adds the pixels' terms up with atomics: the reported loss (not its gradient)
      # flickers in the last bit run to run; deterministic mode: per-pixel terms, then a plain (fixed-order) sum
      per_pixel = F.cross_entropy(logits, labels, ignore_index=self.ignore_index, reduction='none')
      loss = per_pixel.sum() / keep.sum()
    else:
      loss = self.semantic_loss(logits, labels)
    return logits, prediction, loss, accuracy

  def forward(self, datas, targets=None):
    """softmax_classifier.py:36-93: `datas['embedding']` [N,C,H,W]; optional
    `targets['semantic_label']` [N,H',W']."""
    logits = self._logits(datas['embedding'])
    labels = (targets or {}).get('semantic_label', None)
    if labels is None:
      prediction, loss, accuracy = logits.argmax(dim=1), None, None
    else:
      logits, prediction, loss, accuracy = self._supervise(logits, labels)
    return {'semantic_prediction': prediction, 'semantic_logit': logits,
            'sem_ann_loss': loss, 'accuracy': accuracy}

  # ---- inference: one crop's logits added into the full-resolution canvas ----
  def _inference_tensors(self):
    head = self.semantic_classifier
    return (head[0].weight, head[1].weight, head[1].bias, head[1].running_mean, head[1].running_var,
            head[4].weight, head[4].bias)

  def _inference_key(self):
    """What the folded operands were computed from: storage, batch-norm epsilon and an integer checksum of the bit
    patterns of every parameter and statistic (position-weighted, exact in int64, so `.data.copy_()` -- which moves
    no version counter -- changes it too).  One device reduction and ONE host read."""
    ts = self._inference_tensors()
    bits = torch.cat([t.detach().reshape(-1).float().contiguous().view(torch.int32) for t in ts]).to(torch.int64)
    ramp = torch.arange(bits.numel(), dtype=torch.int64, device=bits.device) % 65521 + 1
    return (tuple(t.data_ptr() for t in ts), float(self.semantic_classifier[1].eps), int((bits * ramp).sum().item()))

  def invalidate_inference_cache(self):
    """Forget the folded operands (call after changing parameters in a way `prepare_inference` is not given the
    chance to see, e.g. between the crops of one image)."""
    self._inference_cache = None

  def train(self, mode=True):
    self._inference_cache = None
    return super().train(mode)

  def _load_from_state_dict(self, *args, **kwargs):
    self._inference_cache = None
    return super()._load_from_state_dict(*args, **kwargs)

  @staticmethod
  def _padded_hidden(c):
    """Hidden channels of the HIP head: 2C rounded up to the 64 output channels a tile of the matrix-core convolution
    covers.  The added channels have zero weights and a zero bias (ReLU(0) = 0) and zero columns in the 1x1 head: they
    add exact zeros, so C = 16 or 48 (2C % 64 = 32) run on the kernels too."""
    return (2 * c + 63) // 64 * 64

  def head_path_name(self, embedding):
    """Which path `accumulate_logits` takes for this embedding: the HIP head, or -- where the shape is outside what
    the kernels cover (C % 16, num_classes > 64, C > 512) -- the framework ops."""
    c = embedding.shape[-3]
    hidden = self._padded_hidden(c)
    ok = (c % 16 == 0 and c <= 512 and _ffi.conv_hl8_supported(c, hidden, 9) and
          _ffi.class_head_supported(hidden, self.num_classes))
    return HIP_HEAD_PATH if ok else FRAMEWORK_HEAD_PATH

  def prepare_inference(self):
    """Folds the batch norm into the 3x3 convolution and converts the operands of the HIP head, unless the cached
    ones still belong to the current parameters (`_inference_key`: costs a host synchronisation, so the
    full-resolution pass calls this once per image, not per crop).  Eval mode only."""
    if self.training:
      raise RuntimeError('SoftmaxClassifier.prepare_inference: the module is in train mode (call .eval() first)')
    key = self._inference_key()
    if self._inference_cache is None or self._inference_cache['key'] != key:
      head = self.semantic_classifier
      w, bias = fold_conv_bn(head[0].weight.float(), head[1])
      cls_weight = head[4].weight.detach().float().reshape(self.num_classes, -1)
      pad = self._padded_hidden(w.shape[1]) - w.shape[0]
      if pad:                                                   # (zero hidden channels: `_padded_hidden`)
        w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0)
        bias = torch.cat([bias.float(), bias.new_zeros((pad,), dtype=torch.float32)], 0)
        cls_weight = torch.cat([cls_weight, cls_weight.new_zeros((self.num_classes, pad))], 1)
      wf, _ = _ffi.hl8_weight(w)
      self._inference_cache = {
          'key': key, 'weight': wf, 'bias': bias.float().contiguous(), 'cls_weight': cls_weight.contiguous(),
          'cls_bias': head[4].bias.detach().float().contiguous()}
    return self._inference_cache

  def accumulate_logits(self, embedding, canvas, sh, sw):
    """`canvas[..., sh:sh+h, sw:sw+w] += logits(embedding)` in place, for ONE crop: `embedding` [1, C, h, w] (or
    [C, h, w]), `canvas` fp32 [1, num_classes, Hp, Wp] (or without the 1) -- inference_softmax.py:128-137 with
    softmax_classifier.py:52-55.  Eval mode only (raises in train mode).  Three launches: x / |x| to the split-f16
    operand, the 3x3 convolution with the folded batch norm + ReLU on the matrix cores, the 1x1 head accumulated into
    the canvas window.  Where the shape is unsupported (`head_path_name`) it falls back to
    `canvas[..., sh:sh+h, sw:sw+w] += self._logits(embedding)` on the framework: the same result.  Returns the name
    of the path taken.  The folded operands are cached on the module; `prepare_inference` (called here only when
    there is no cache) re-validates them."""
    if self.training:
      raise RuntimeError('SoftmaxClassifier.accumulate_logits: the module is in train mode (call .eval() first)')
    emb = embedding if embedding.dim() == 4 else embedding.unsqueeze(0)
    if emb.shape[0] != 1:
      raise ValueError('accumulate_logits takes one crop [1, C, h, w]')
    h, w = emb.shape[-2:]
    cv = canvas if canvas.dim() == 3 else canvas[0]
    if cv.dim() != 3 or cv.shape[0] != self.num_classes or (canvas.dim() == 4 and canvas.shape[0] != 1):
      raise ValueError('accumulate_logits: canvas must be [1, num_classes, Hp, Wp]')
    path = self.head_path_name(emb)
    with torch.no_grad():
      if path == FRAMEWORK_HEAD_PATH:
        cv[:, sh:sh + h, sw:sw + w] += self._logits(emb)[0]
        return path
      cache = self._inference_cache or self.prepare_inference()
      unit = _ffi.unit_hl8_from_nchw(emb.float().contiguous())
      hidden, _ = _ffi.conv_hl8_affine(unit, cache['weight'], cache['bias'], 1, h, w, 9, relu=True, want_hl8=False)
      _ffi.class_head_accumulate(hidden, cache['cls_weight'], cache['cls_bias'], cv, sh, sw, h, w)
    return path

  def get_params_lr(self):
    """Weights at 10x, biases at 20x without weight decay (softmax_classifier.py:95-111)."""
    pick = lambda suffix: list(model_utils.get_params(self, ['semantic_classifier'], [suffix]))
    return [{'params': pick('weight'), 'lr': 10},
            {'params': pick('bias'), 'lr': 20, 'weight_decay': 0}]


def softmax_classifier(config):
  return SoftmaxClassifier(config)
