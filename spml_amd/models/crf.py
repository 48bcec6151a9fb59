"""Dense CRF post-processing with the reference's interface (`spml/models/crf.py:14-41` of twke18/SPML).

The reference hands the image and the probability map to pydensecrf, which approximates the two fully connected
filters with a permutohedral lattice on the CPU.  This class runs the mean-field iteration itself, over all pixel pairs,
as HIP kernels (`csrc/dense_crf.hip`): same constructor, same call, no CPU fallback."""
import numpy as np
import torch

from spml_amd import _ffi


class DenseCRF(object):

  def __init__(self, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    self.iter_max = iter_max
    self.pos_w = pos_w
    self.pos_xy_std = pos_xy_std
    self.bi_w = bi_w
    self.bi_xy_std = bi_xy_std
    self.bi_rgb_std = bi_rgb_std

  def path_name(self, h, w, ncls):
    """The route a `[ncls, h, w]` call takes (host only)."""
    return _ffi.dense_crf_path_name(h, w, ncls, self.pos_xy_std)

  def prepare(self, image, ncls):
    """image: uint8 `[h, w, 3]` device tensor -> the prepared workspace of `infer` (reusable with other weights)."""
    if not torch.is_tensor(image) or not image.is_cuda:
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (the dense CRF has no CPU fallback)')
    ws = _ffi.dense_crf_workspace(image.shape[0], image.shape[1], ncls, image.device)
    _ffi.dense_crf_prepare(image, self.pos_xy_std, self.bi_xy_std, self.bi_rgb_std, ws)
    return ws

  def infer(self, ws, probmap, want_labels=True, iter_max=None, pos_w=None, bi_w=None):
    """probmap fp32 `[C, h, w]` device tensor and a prepared workspace -> (Q `[C, h, w]`, arg-max `[h, w]` or None)."""
    return _ffi.dense_crf_infer(probmap, self.iter_max if iter_max is None else iter_max,
                                self.pos_w if pos_w is None else pos_w, self.bi_w if bi_w is None else bi_w, ws,
                                want_labels)

  def refine(self, image, probmap):
    """Device tensors in, device tensors out: (Q `[C, h, w]` fp32, arg-max `[h, w]` int64)."""
    if not (torch.is_tensor(image) and torch.is_tensor(probmap) and image.is_cuda and probmap.is_cuda):
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (the dense CRF has no CPU fallback)')
    if probmap.dim() != 3 or image.dim() != 3 or tuple(image.shape) != (probmap.shape[1], probmap.shape[2], 3):
      raise ValueError('DenseCRF expects an image [h, w, 3] and a probability map [C, h, w] of the same size')
    if image.dtype != torch.uint8:
      raise ValueError('DenseCRF expects a uint8 image')
    with torch.no_grad():
      ws = self.prepare(image.contiguous(), probmap.shape[0])
      return self.infer(ws, probmap.float().contiguous())

  def infer_upsampled(self, ws, lowres, image_hw, want_labels=True, want_labels_before=True, want_prob_up=False,
                      iter_max=None, pos_w=None, bi_w=None):
    """`infer` on the bilinear up-sampling of `lowres` fp32 `[C, oh, ow]` to `image_hw` (`F.interpolate`,
    align_corners=False), formed inside the first kernel -> (Q `[C, h, w]`, its arg-max `[h, w]` or None, the
    arg-max of the up-sampled map -- the label before the CRF -- or None, the up-sampled map `[C, h, w]` or None)."""
    if not torch.is_tensor(lowres) or not lowres.is_cuda:
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (the dense CRF has no CPU fallback)')
    return _ffi.dense_crf_infer_upsampled(lowres, image_hw, self.iter_max if iter_max is None else iter_max,
                                          self.pos_w if pos_w is None else pos_w, self.bi_w if bi_w is None else bi_w,
                                          ws, want_labels, want_labels_before, want_prob_up)

  def refine_upsampled(self, image, lowres):
    """`refine` of the random-walk programs (pseudo_softmaxrw_crf.py:172-187): the image `[h, w, 3]` uint8 and a map
    `[C, oh, ow]` of any lower (or equal) resolution, device tensors -> (Q `[C, h, w]` fp32, its arg-max `[h, w]` int64,
    the arg-max of the up-sampled map `[h, w]` int64)."""
    if not (torch.is_tensor(image) and torch.is_tensor(lowres) and image.is_cuda and lowres.is_cuda):
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (the dense CRF has no CPU fallback)')
    if lowres.dim() != 3 or image.dim() != 3 or image.shape[2] != 3:
      raise ValueError('DenseCRF expects an image [h, w, 3] and a low-resolution map [C, oh, ow]')
    if image.dtype != torch.uint8:
      raise ValueError('DenseCRF expects a uint8 image')
    with torch.no_grad():
      ws = self.prepare(image.contiguous(), lowres.shape[0])
      return self.infer_upsampled(ws, lowres.float().contiguous(), tuple(image.shape[:2]))[:3]

  def infer_votes(self, ws, clu, topk, ncls, image_hw, want_labels=True, want_labels_before=True, want_prob=False,
                  iter_max=None, pos_w=None, bi_w=None):
    """`infer` on the vote map of the kNN label inference (inference_crf.py:240-245): `clu` int64 `[h * w]` dense segment
    ids, `topk` int64 `[m, k]` retrieved labels per segment; the map `one_hot(topk[clu]).sum(1) / k` is gathered from a
    per-segment table inside the first kernel -> (Q `[C, h, w]`, its arg-max `[h, w]` or None, the arg-max of
    the votes -- the label before the CRF -- or None, the vote map `[C, h, w]` or None)."""
    if not (torch.is_tensor(clu) and torch.is_tensor(topk) and clu.is_cuda and topk.is_cuda):
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (the dense CRF has no CPU fallback)')
    return _ffi.dense_crf_infer_votes(clu, topk, ncls, image_hw, self.iter_max if iter_max is None else iter_max,
                                      self.pos_w if pos_w is None else pos_w, self.bi_w if bi_w is None else bi_w, ws,
                                      want_labels, want_labels_before, want_prob)

  def refine_votes(self, image, clu, topk, ncls):
    """`refine` of the kNN program (inference_crf.py:237-257): the image `[h, w, 3]` uint8, one dense segment id per pixel
    (`[h * w]` or `[h, w]` int64; a strided view, such as the crop of a padded map, is copied) and the retrieved labels
    `[m, k]` int64, device tensors -> (Q `[C, h, w]` fp32, its arg-max `[h, w]` int64, the arg-max of the votes `[h, w]`
    int64)."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (image, clu, topk)):
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (the dense CRF has no CPU fallback)')
    if image.dim() != 3 or image.shape[2] != 3 or topk.dim() != 2 or clu.numel() != image.shape[0] * image.shape[1]:
      raise ValueError('DenseCRF expects an image [h, w, 3], one segment id per pixel and labels [m, k]')
    if image.dtype != torch.uint8:
      raise ValueError('DenseCRF expects a uint8 image')
    with torch.no_grad():
      ws = self.prepare(image.contiguous(), ncls)
      return self.infer_votes(ws, clu.long().contiguous(), topk.long().contiguous(), ncls, tuple(image.shape[:2]))[:3]

  def __call__(self, image, probmap):
    """numpy arrays (HWC uint8, CHW float32) -> numpy CHW float32 through the GPU, as the reference; device tensors ->
    a device tensor.  Without a GPU, or for CPU tensors, `SpmlHipError`."""
    if torch.is_tensor(image) or torch.is_tensor(probmap):
      return self.refine(image, probmap)[0]
    if not torch.cuda.is_available():
      raise _ffi.SpmlHipError('the dense CRF needs an MI355X (the HIP path has no CPU fallback)')
    device = torch.device('cuda', torch.cuda.current_device())
    image_d = torch.from_numpy(np.ascontiguousarray(image)).to(device)
    prob_d = torch.from_numpy(np.ascontiguousarray(probmap, dtype=np.float32)).to(device)
    return self.refine(image_d, prob_d)[0].cpu().numpy()
