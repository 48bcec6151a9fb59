"""Full-resolution inference pieces of the memory-bank pass
(`pyscripts/inference/prototype.py:107-211`, the same loop is in `inference.py:162-220`):
sliding-window embedding with overlap averaging, k-means over the whole image at full
resolution (the real consumer of the 513x513xC k-means kernel), prototypes + majority
labels, memory-bank files.  SURVEY.md 8(f) rows N1/N2.

The per-crop normalise + accumulate is one HIP kernel (`spml_window_accumulate_f32`),
clustering and prototypes are the same kernels the training path uses."""
import math

import numpy as np
import torch

import spml_amd.utils.general.common as common_utils
import spml_amd.utils.segsort.common as segsort_common
import spml_amd.utils.segsort.others as segsort_others
from spml_amd import _ffi, ops


def sliding_window_ends(pad_size, crop_size, stride):
  """End coordinates of the crops along one axis (prototype.py:134-142)."""
  n = math.ceil(1.0 * (pad_size - crop_size) / stride) + 1
  return np.linspace(crop_size, pad_size, n, dtype=np.int32)


def _is_channels_last(embedding_model):
  first = next(embedding_model.parameters(), None)
  return first is not None and first.is_cuda and first.dim() == 4 and \
      first.is_contiguous(memory_format=torch.channels_last) and not first.is_contiguous()


def _require_gpu(*tensors, what=None):
  """The device check of every entry point: each of `tensors` is on the GPU, or the one error of the HIP path.  `what`
  names the offender in front of its device ('a view on', 'got'); without it the message is the dense CRF's, which
  names neither."""
  for tensor in tensors:
    if not (torch.is_tensor(tensor) and tensor.is_cuda):
      why = 'the dense CRF has no CPU fallback)' if what is None else '%s %s); there is no CPU fallback' % (what, tensor.device)
      raise _ffi.SpmlHipError('the HIP path needs GPU tensors (' + why)


def _eighth_size(name, image_hw):
  """-> `(h // 8, w // 8)`, the size the random walk runs at; `name` is the caller's, for the error of an image that has
  none."""
  out_hw = (image_hw[0] // 8, image_hw[1] // 8)
  if out_hw[0] < 1 or out_hw[1] < 1:
    raise ValueError(name + ': the image is smaller than 8 x 8')
  return out_hw


def _check_views(who, views, also=None):
  """What every multi-view routine asks of `views`: at least one, each one image `[1,3,Hp,Wp]`, each on the GPU.  `who`
  names the caller in the errors; `also(i)` is the caller's own check of view `i`, run before that view's device check."""
  if not views:
    raise ValueError('%s needs at least one view' % who)
  for i, (image, _, _) in enumerate(views):
    if image.dim() != 4 or image.shape[0] != 1:
      raise ValueError('%s expects views of one image [1,3,Hp,Wp]' % who)
    if also is not None:
      also(i)
    _require_gpu(image, what='a view on')


def _group_by_padded_size(views):
  """Consecutive views of one padded size (a flip pair, or several scales that all pad up to the crop size) -> list of
  lists of views, in call order."""
  groups = []
  for view in views:
    if groups and groups[-1][0][0].shape == view[0].shape:
      groups[-1].append(view)
    else:
      groups.append([view])
  return groups


def _padding_ignored_labels(pad_hw, valid_hw, ignore_index, device):
  """Fake labels `[1,Hp,Wp]` that make the clustering ignore the zero padding outside the top-left `valid_hw` region
  (prototype.py:117-131)."""
  fake = torch.full((1,) + tuple(pad_hw), ignore_index, dtype=torch.long, device=device)
  fake[:, :valid_hw[0], :valid_hw[1]] = 0
  return fake


def _window_embeddings(embedding_model, images, crop_size, stride):
  """The sliding-window loop of prototype.py:134-181 (= inference_softmax.py:105-128) over `images`, padded images
  `[1,3,Hp,Wp]` of ONE size: yields `(k, sh, sw, embedding [1,C,crop_h,crop_w])` for every crop -- image after image,
  each in the reference's window order.  The crops go through the network in groups of 8 that may span images (eval mode:
  every sample is independent, the reference's one-crop-at-a-time loop gives the same embeddings), in the memory format
  of the model."""
  pad_h, pad_w = images[0].shape[-2:]
  crop_h, crop_w = crop_size
  ends_h = sliding_window_ends(pad_h, crop_h, stride[0])
  ends_w = sliding_window_ends(pad_w, crop_w, stride[1])
  windows = [(k, int(eh) - crop_h, int(ew) - crop_w) for k in range(len(images)) for eh in ends_h for ew in ends_w]
  nhwc = _is_channels_last(embedding_model)
  group = 8
  for g0 in range(0, len(windows), group):
    part = windows[g0:g0 + group]
    crops = torch.cat([images[k][:, :, sh:sh + crop_h, sw:sw + crop_w] for k, sh, sw in part], 0)
    if nhwc:
      crops = crops.contiguous(memory_format=torch.channels_last)
    embs = embedding_model.generate_embeddings({'image': crops}, resize_as_input=True)['embedding']
    for i, (k, sh, sw) in enumerate(part):
      yield k, sh, sw, embs[i:i + 1]


def embed_full_resolution(embedding_model, image, crop_size, stride):
  """Sliding-window embedding `[1,C,Hp,Wp]` of a padded image `[1,3,Hp,Wp]`
  (prototype.py:134-181): crops are embedded with `generate_embeddings(...,
  resize_as_input=True)`, normalised over the channels and overlap-averaged."""
  if image.dim() != 4 or image.shape[0] != 1:
    raise ValueError('embed_full_resolution expects one image [1,3,H,W]')
  pad_h, pad_w = image.shape[-2:]
  acc = None
  counts = torch.zeros((pad_h, pad_w), dtype=torch.float32, device=image.device)
  with torch.no_grad():
    for _, sh, sw, emb in _window_embeddings(embedding_model, [image], crop_size, stride):
      emb = emb[0].float().contiguous()
      if acc is None:
        acc = torch.zeros((emb.shape[0], pad_h, pad_w), dtype=torch.float32, device=image.device)
      _ffi.window_accumulate(emb, acc, counts, sh, sw)
    acc /= counts
  return acc.unsqueeze(0)


def full_resolution_prototypes(embedding_model, image, semantic_label, crop_size, stride,
                               semantic_ignore_index=255):
  """One image of the memory-bank pass (prototype.py:107-211): padded `image`
  `[1,3,Hp,Wp]`, `semantic_label` `[h,w]` of the un-padded (top-left) region ->
  (prototypes [M,C], majority label per prototype [M], cluster index map [h,w])."""
  h, w = semantic_label.shape[-2:]
  fake = _padding_ignored_labels(image.shape[-2:], (h, w), semantic_ignore_index, image.device)
  embeddings = embed_full_resolution(embedding_model, image, crop_size, stride)
  with torch.no_grad():
    out = embedding_model.generate_clusters(embeddings, fake, fake)
    prototypes = segsort_common.calculate_prototypes_from_labels(
        out['cluster_embedding'], out['cluster_index'])
    _, prototype_labels = segsort_common.find_majority_label_index(
        semantic_label.to(image.device), out['cluster_index'])
  return prototypes, prototype_labels, out['cluster_index'].view(h, w)


def label_views(label, view_sizes):
  """The label half of `create_image_pyramid` (spml/utils/general/others.py): the label map `[h,w]` resized by nearest
  neighbour to each `(rh, rw)` of `view_sizes` -- the second entries of `flip_scale_views`' views, so that the image and
  the label of a view always have one size.  -> list of int64 `[rh, rw]` maps on the label's device.  A host-side
  stand-in for the loader (cv2's INTER_NEAREST there, torch's `nearest` here): not parity-pinned; for views that
  `flip_scale_views` mirrored the caller mirrors the label too (the memory-bank pass makes none).  The label views of a
  decoded file come from `device_views(..., semantic_label=...)`."""
  label = torch.as_tensor(label)
  if label.dim() != 2:
    raise ValueError('label_views expects one label map [h,w]')
  out = []
  for rh, rw in view_sizes:
    if (int(rh), int(rw)) == tuple(label.shape):
      out.append(label.long())
    else:
      # (through float, as general/common.py:11-26 resizes labels: exact for values below 2^24)
      resized = torch.nn.functional.interpolate(label[None, None].float(), size=(int(rh), int(rw)), mode='nearest')
      out.append(resized[0, 0].long())
  return out


def multiscale_prototypes(embedding_model, views, label_views, crop_size, stride, semantic_ignore_index=255,
                          num_classes=256):
  """One image of the multi-scale memory-bank pass (`pyscripts/inference/prototype_msc.py:92-206`; with one view,
  `prototype.py:92-211`).  `views`: list of `(image [1,3,Hp,Wp], (rh, rw), is_flip)` (`flip_scale_views` with scales
  0.5, 1, 1.5 and no flip there); `label_views`: the semantic label `[rh, rw]` of every view (`label_views`; a mirrored
  view takes a mirrored label).

  Per view: fake labels that make the clustering ignore the zero padding (:109-120), `embed_full_resolution` (:126-173),
  `generate_clusters` (:176-183), `calculate_prototypes_from_labels` (:186-188) and -- in the place of
  `find_majority_label_index` (:189-192) -- `segment_majority_labels` with the segment count taken from the prototype
  rows and `num_classes` classes (256: label maps hold the ignore label 255; such prototypes stay in the bank files, the
  retrieval side drops them: `drop_ignored_memory`): one HIP count + arg-max, no host read.  The views' prototypes and
  labels are concatenated in view order (:204-206).  Returns a dict: `prototype` `[sum M, C]`, `prototype_label`
  `[sum M]` int64, `segment_counts` (list of M per view), `cluster_index` (list of `[rh * rw]` dense segment ids) and
  `majority_path` (`'hip_majority'`, or `'framework_majority'` where a view is outside the kernel's limits)."""
  if views and len(label_views) != len(views):        # (an empty list is reported first, by _check_views)
    raise ValueError('multiscale_prototypes needs one label map per view (%d for %d views)' % (len(label_views), len(views)))

  def label_fits(i):
    (rh, rw), label = views[i][1], label_views[i]
    if tuple(label.shape[-2:]) != (rh, rw) or label.numel() != rh * rw:
      raise ValueError('multiscale_prototypes: a %d x %d view with a label map of shape %r' % (rh, rw, tuple(label.shape)))
  _check_views('multiscale_prototypes', views, label_fits)
  device = views[0][0].device
  prototypes, labels, counts, cluster_index = [], [], [], []
  majority_path = segsort_common.HIP_MAJORITY_PATH
  with torch.no_grad():
    for (image, (rh, rw), _), label in zip(views, label_views):
      fake = _padding_ignored_labels(image.shape[-2:], (rh, rw), semantic_ignore_index, device)
      embeddings = embed_full_resolution(embedding_model, image, crop_size, stride)
      out = embedding_model.generate_clusters(embeddings, fake, fake)
      protos = segsort_common.calculate_prototypes_from_labels(out['cluster_embedding'], out['cluster_index'])
      major, path = segsort_common.segment_majority_labels(label.to(device), out['cluster_index'], protos.shape[0],
                                                           num_classes)
      if path != segsort_common.HIP_MAJORITY_PATH:
        majority_path = path
      prototypes.append(protos)
      labels.append(major)
      counts.append(int(protos.shape[0]))
      cluster_index.append(out['cluster_index'])
  return {'prototype': torch.cat(prototypes, 0), 'prototype_label': torch.cat(labels, 0), 'segment_counts': counts,
          'cluster_index': cluster_index, 'majority_path': majority_path}


def drop_ignored_memory(prototypes, prototype_labels, semantic_ignore_index=255):
  """The memory bank without the prototypes of the ignore class (inference.py:99-111)."""
  keep = torch.nonzero(prototype_labels != semantic_ignore_index).view(-1)
  return prototypes.index_select(0, keep), prototype_labels.index_select(0, keep)


def _clustered_full_resolution(embedding_model, image, valid_hw, crop_size, stride, semantic_ignore_index):
  """The embedding and clustering steps `predict_full_resolution` and `predict_knn_full_resolution_crf` share
  (`inference.py:145-220` = `inference_crf.py:145-229`): the sliding-window embedding of the padded `image` and the
  k-means over it with the padding outside the top-left `valid_hw` region ignored -> the dict the prediction model reads
  (`embedding` plus what `generate_clusters` returns)."""
  fake = _padding_ignored_labels(image.shape[-2:], valid_hw, semantic_ignore_index, image.device)
  embeddings = {'embedding': embed_full_resolution(embedding_model, image, crop_size, stride)}
  with torch.no_grad():
    embeddings.update(embedding_model.generate_clusters(embeddings['embedding'], fake, fake))
  return embeddings


def predict_full_resolution(embedding_model, prediction_model, image, valid_hw, crop_size, stride,
                            memory_prototypes, memory_prototype_labels, semantic_ignore_index=255):
  """One image of the kNN label inference (`pyscripts/inference/inference.py:145-237`), the composition
  of the two rows above: sliding-window embedding of the padded `image` `[1,3,Hp,Wp]` (:162-210),
  k-means at full resolution with the padding outside the top-left `valid_hw` region ignored
  (:145-156, :212-220: the 513x513xC kernel's consumer), then `prediction_model(..., with_loss=False,
  with_prediction=True)` against the memory bank (:223-227: prototypes of the segments, top-20
  retrieval, majority vote, scatter to the pixels).  Returns a dict with `semantic_prediction` `[h,w]`
  (what :231-237 turns into the label image), `semantic_score` (the retrieved labels, `[h*w,20]`)
  and `cluster_index` `[h*w]`."""
  h, w = valid_hw
  embeddings = _clustered_full_resolution(embedding_model, image, valid_hw, crop_size, stride, semantic_ignore_index)
  with torch.no_grad():
    outputs = prediction_model(
        embeddings,
        {'semantic_memory_prototype': memory_prototypes,
         'semantic_memory_prototype_label': memory_prototype_labels},
        with_loss=False, with_prediction=True)
  return {'semantic_prediction': outputs['semantic_prediction'].view(h, w),
          'semantic_score': outputs['semantic_score'], 'cluster_index': embeddings['cluster_index']}


def window_counts(pad_size, crop_size, stride):
  """How many sliding windows cover each position of one axis -> float32 `[pad_size]`.  The windows of an image are the
  Cartesian product of the two axes' windows, so the reference's `counts[y][x]` (inference_softmax_msc.py:120-134) is
  `window_counts(pad_h, ...)[y] * window_counts(pad_w, ...)[x]` exactly (small integers)."""
  counts = np.zeros((int(pad_size),), dtype=np.float32)
  for end in sliding_window_ends(pad_size, crop_size, stride):
    counts[int(end) - crop_size:int(end)] += 1
  return counts


def _accumulate_window_logits(embedding_model, prediction_model, images, canvases, crop_size, stride):
  """The sliding-window loop of inference_softmax.py:105-137 (= inference_softmax_msc.py:107-134 without the counts) over
  `images`, padded images `[1,3,Hp,Wp]` of ONE size: the crops of all of them -- image after image, each in the
  reference's window order -- go through the backbone in groups of 8, and each crop's logits are added into the canvas
  `[1,ncls,Hp,Wp]` of its own image, so the fp32 sum order of a pixel is the reference's.  Returns the name of the path
  `SoftmaxClassifier.accumulate_logits` took."""
  path = None
  for k, sh, sw, emb in _window_embeddings(embedding_model, images, crop_size, stride):
    path = prediction_model.accumulate_logits(emb, canvases[k], sh, sw)
  return path


def predict_softmax_full_resolution(embedding_model, prediction_model, image, valid_hw, crop_size, stride):
  """One image of the softmax label inference (`pyscripts/inference/inference_softmax.py:105-148`): sliding
  windows over the padded `image` `[1,3,Hp,Wp]` (:105-123), per crop the embedding at input resolution and the
  classifier head (:126-128), the crops' logits SUMMED into the canvas (:130-137: no counts, unlike the embedding
  route), arg-max (:142) cropped to the top-left `valid_hw` region (:148).  The crops of a group go through the
  backbone together; each crop's logits are added in the reference's window order, so the fp32 sum order of a pixel is
  the reference's.  Returns `semantic_logit` `[1,ncls,Hp,Wp]`, `semantic_prediction` `[h,w]` (int64) and `head_path`,
  the name of the path `SoftmaxClassifier.accumulate_logits` took."""
  if image.dim() != 4 or image.shape[0] != 1:
    raise ValueError('predict_softmax_full_resolution expects one image [1,3,H,W]')
  h, w = valid_hw
  pad_h, pad_w = image.shape[-2:]
  canvas = torch.zeros((1, prediction_model.num_classes, pad_h, pad_w), dtype=torch.float32, device=image.device)
  prediction_model.prepare_inference()          # once per image: validates the folded operands (one host read)
  with torch.no_grad():
    path = _accumulate_window_logits(embedding_model, prediction_model, [image], [canvas], crop_size, stride)
    prediction = _ffi.argmax_channels(canvas[0], h, w)
  return {'semantic_logit': canvas, 'semantic_prediction': prediction, 'head_path': path}


HIP_VIEW_PROBS_PATH = 'hip_view_probs'
FRAMEWORK_VIEW_PROBS_PATH = 'framework_view_probs'
MAX_VIEW_PROBS_CLASSES = 64            # spml_view_probs_accumulate_f32 keeps every class of a pixel in registers


def framework_view_probs_accumulate(canvas, cnt_y, cnt_x, crop_hw, flip, acc):
  """The tail of one view as the reference's own ops on the tensors' device (inference_softmax_msc.py:135-143, 147):
  what `_ffi.view_probs_accumulate` computes in one kernel.  The path of `predict_softmax_multiscale` above 64 classes
  and the yardstick of tools/bench_softmax_msc.py."""
  rh, rw = crop_hw
  logit = canvas.unsqueeze(0) / (cnt_y.view(-1, 1) * cnt_x.view(1, -1))
  logit = logit[..., :rh, :rw]
  logit = torch.nn.functional.interpolate(logit, size=tuple(acc.shape[-2:]), mode='bilinear')
  prob = torch.softmax(logit, dim=1)[0]
  acc += torch.flip(prob, dims=[2]) if flip else prob
  return acc


def predict_softmax_multiscale(embedding_model, prediction_model, views, image_hw, crop_size, stride):
  """One image of the multi-scale + flip softmax label inference (`pyscripts/inference/inference_softmax_msc.py:95-149`).
  `views`: list of `(image [1,3,Hp,Wp], (rh, rw), is_flip)` (`flip_scale_views`: per scale the flipped view first, as
  `create_image_pyramid`); `image_hw`: the un-padded image.

  Per view the sliding windows run exactly as in `predict_softmax_full_resolution` (:107-134; consecutive views of one
  padded size -- a flip pair, or several scales that all pad up to the crop size -- send their crops through the backbone
  together, each view's windows are added into that view's canvas in the reference's order), then ONE kernel, `spml_view_probs_accumulate_f32`, divides by the overlap
  counts, crops, interpolates to the image, soft-maxes, un-flips and adds into the `[ncls,h,w]` sum (:135-143, :146-147;
  views in call order: the fp32 sum order of a pixel is the reference's).  After the last view
  `spml_argmax_channels_i64` gives the labels (:149).  Above 64 classes the tail of a view runs as the reference's torch
  ops on the device instead (`framework_view_probs_accumulate`); `combine_path` names which of the two ran, as
  `head_path` does for the classifier head.  Returns `semantic_prob` `[ncls,h,w]` (the sum over the views, :147),
  `semantic_prediction` `[h,w]` int64, `head_path` and `combine_path`."""
  _check_views('predict_softmax_multiscale', views)
  h, w = image_hw
  device = views[0][0].device
  ncls = prediction_model.num_classes
  combine_path = HIP_VIEW_PROBS_PATH if ncls <= MAX_VIEW_PROBS_CLASSES else FRAMEWORK_VIEW_PROBS_PATH
  combine = _ffi.view_probs_accumulate if combine_path == HIP_VIEW_PROBS_PATH else framework_view_probs_accumulate
  prediction_model.prepare_inference()          # once per image, as in predict_softmax_full_resolution
  acc, path = torch.zeros((ncls, h, w), dtype=torch.float32, device=device), None
  with torch.no_grad():
    for part in _group_by_padded_size(views):
      pad_h, pad_w = part[0][0].shape[-2:]
      cnt_y = torch.from_numpy(window_counts(pad_h, crop_size[0], stride[0])).to(device)
      cnt_x = torch.from_numpy(window_counts(pad_w, crop_size[1], stride[1])).to(device)
      canvases = [torch.zeros((1, ncls, pad_h, pad_w), dtype=torch.float32, device=device) for _ in part]
      path = _accumulate_window_logits(embedding_model, prediction_model, [v[0] for v in part], canvases, crop_size,
                                       stride)
      for canvas, (_, crop_hw, flip) in zip(canvases, part):
        combine(canvas[0], cnt_y, cnt_x, crop_hw, flip, acc)
    prediction = _ffi.argmax_channels(acc, h, w)
  return {'semantic_prob': acc, 'semantic_prediction': prediction, 'head_path': path, 'combine_path': combine_path}


HIP_VIEW_VOTES_PATH = 'hip_view_votes'
FRAMEWORK_VIEW_VOTES_PATH = 'framework_view_votes'


def framework_view_votes_accumulate(clu, crop_hw, topk, ncls, flip, acc):
  """The tail of one view as the reference's own ops on the tensors' device (inference_msc.py:223-234, the sum of
  :237-239): gather the retrieved labels per pixel, one-hot over the classes, mean over the k retrievals, bilinear resize
  to the image (the half-pixel mapping of `cv2.resize(..., INTER_LINEAR)`), un-flip, add.  What
  `_ffi.view_votes_accumulate` computes in two small kernels; the path of `predict_knn_multiscale` outside the kernel's
  limits and the yardstick of tools/bench_knn_msc.py.  As in the reference, a label outside `[0, ncls)` is an error."""
  rh, rw = crop_hw
  score = topk[clu.reshape(-1)]                                                          # [rh * rw, k]
  votes = torch.mean(common_utils.one_hot(score, int(ncls)).float(), dim=1)              # :223-225
  votes = votes.view(rh, rw, -1).permute(2, 0, 1).unsqueeze(0)
  votes = torch.nn.functional.interpolate(votes, size=tuple(acc.shape[-2:]), mode='bilinear', align_corners=False)[0]
  acc += torch.flip(votes, dims=[2]) if flip else votes
  return acc


def _knn_view_votes_sum(who, embedding_model, prediction_model, views, image_hw, crop_size, stride, memory_prototypes,
                        memory_prototype_labels, num_classes):
  """The per-view work of `predict_knn_multiscale` and `pseudo_labels_knn_multiscale` (inference_msc.py:157-234 =
  pseudo_inference_crf_msc.py:172-249) -> (the un-divided `[ncls,h,w]` sum of the views' vote maps, combine_path, the
  per-view dense segment ids, the per-view `[m, 20]` retrieved labels).  `who` names the caller in the errors."""
  _check_views(who, views)
  h, w = image_hw
  device = views[0][0].device
  ncls = int(num_classes)
  memory = {'semantic_memory_prototype': memory_prototypes, 'semantic_memory_prototype_label': memory_prototype_labels}
  acc = torch.zeros((ncls, h, w), dtype=torch.float32, device=device)
  combine_path, cluster_index, segment_topk = HIP_VIEW_VOTES_PATH, [], []
  with torch.no_grad():
    for image, (rh, rw), flip in views:
      embs = embed_full_resolution(embedding_model, image, crop_size, stride)[..., :rh, :rw].contiguous()
      fake = torch.zeros((1, rh, rw), dtype=torch.long, device=device)
      out = embedding_model.generate_clusters(embs, fake, fake)
      topk, clu = prediction_model.segment_predictions(out, memory)
      if topk is None:
        raise ValueError('%s needs a memory bank and a clustering' % who)
      cluster_index.append(clu)
      segment_topk.append(topk)
      if ncls <= _ffi.MAX_VIEW_VOTES_CLASSES and topk.shape[0] <= _ffi.MAX_VIEW_VOTES_SEGMENTS:
        _ffi.view_votes_accumulate(clu, (rh, rw), topk.contiguous(), ncls, flip, acc)
      else:
        framework_view_votes_accumulate(clu, (rh, rw), topk, ncls, flip, acc)
        combine_path = FRAMEWORK_VIEW_VOTES_PATH
  return acc, combine_path, cluster_index, segment_topk


def predict_knn_multiscale(embedding_model, prediction_model, views, image_hw, crop_size, stride, memory_prototypes,
                           memory_prototype_labels, num_classes):
  """One image of the multi-scale + flip kNN label inference (`pyscripts/inference/inference_msc.py:129-242`), the form
  the recipes report their numbers through.  `views`: list of `(image [1,3,Hp,Wp], (rh, rw), is_flip)`
  (`flip_scale_views`: per scale the flipped view first); `image_hw`: the un-padded image.

  Per view: `embed_full_resolution` (:157-204), the embedding cropped to the un-padded `[:rh, :rw]` BEFORE clustering
  (:208-214 -- unlike `predict_full_resolution` the k-means grid is laid over the un-padded view), `generate_clusters`
  with all-zero fake labels, `Segsort.segment_predictions` against the memory bank (:218-222: `[m, 20]` labels per
  segment and one segment id per pixel), then `spml_view_votes_accumulate_f32`: the vote table per segment, gathered by
  the id map, resized to the image, un-flipped and added into the `[ncls,h,w]` sum (:223-234; views in call order: the
  fp32 sum order of a pixel is the reference's).  After the last view the sum is divided by the number of views (:239)
  and `spml_argmax_channels_i64` gives the labels (:242; ties go to the lowest class, as `np.argmax`).  Where
  `num_classes` or a view's segment count is outside the kernel's limits, that view's tail runs as the reference's torch
  ops on the device (`framework_view_votes_accumulate`) and `combine_path` names it.  Returns `semantic_prob`
  `[ncls,h,w]`, `semantic_prediction` `[h,w]` int64 and `combine_path`; and, per view, what the tail was fed:
  `cluster_index` (list of `[rh * rw]` dense segment ids) and `segment_topk` (list of `[m, 20]`)."""
  acc, combine_path, cluster_index, segment_topk = _knn_view_votes_sum(
      'predict_knn_multiscale', embedding_model, prediction_model, views, image_hw, crop_size, stride, memory_prototypes,
      memory_prototype_labels, num_classes)
  with torch.no_grad():
    acc /= len(views)
    prediction = _ffi.argmax_channels(acc, image_hw[0], image_hw[1])
  return {'semantic_prob': acc, 'semantic_prediction': prediction, 'combine_path': combine_path,
          'cluster_index': cluster_index, 'segment_topk': segment_topk}


HIP_TAG_NORMALIZE_PATH = 'hip_tag_normalize'
FRAMEWORK_TAG_NORMALIZE_PATH = 'framework_tag_normalize'


def framework_tag_normalize_argmax(acc, num_views, tags, floor=0.15, want_prob=False):
  """The tag-normalised arg-max as torch ops on the tensors' device, what `_ffi.tag_normalize_argmax` computes in two
  launches: `acc` fp32 `[ncls, h, w]` (the sum over `num_views` views) divided by the view count, per class the maximum
  over the image, floored at `floor`, 1 where `tags` (bool `[ncls]`) is false, the division, the arg-max over the
  classes.  The path of `pseudo_labels_knn_multiscale` outside the kernel's limits and the yardstick of
  tools/bench_pseudo_knn_msc.py.  -> (labels int64 `[h, w]`, prob or None, divisor `[ncls]`)."""
  # (a 0-dim tensor, not a Python number: by a number ATen's GPU kernel multiplies with the reciprocal instead)
  mean = acc / torch.full((), float(num_views), dtype=acc.dtype, device=acc.device)
  peak = torch.amax(mean.reshape(mean.shape[0], -1), dim=1)
  divisor = torch.where(tags.bool(), torch.clamp_min(peak, float(floor)), torch.ones_like(peak))
  prob = mean / divisor.view(-1, 1, 1)
  return torch.argmax(prob, dim=0), (prob if want_prob else None), divisor


def pseudo_labels_knn_multiscale(embedding_model, prediction_model, views, image_hw, crop_size, stride, memory_prototypes,
                                 memory_prototype_labels, num_classes, label_tags, floor=0.15, return_prob=False):
  """One image of the tag recipe's pseudo-label generation by nearest-neighbour retrieval
  (`pyscripts/inference/pseudo_inference_crf_msc.py:143-275`), without the denseCRF of :273: the stage ends at the
  arg-max of what the CRF would have been fed, and `return_prob` hands that tensor out for callers who have a CRF.
  `views`, `image_hw`, the models and the memory bank are `predict_knn_multiscale`'s, and so is the work per view (one
  shared helper); `label_tags`: bool `[ncls]` device tensor (`label_tags_from_map`, :138-141).

  After the last view `spml_tag_normalize_argmax_f32` takes the un-divided sum: mean over the views, per class the
  maximum over the image floored at `floor`, 1 for the classes the image does not carry, the division (:252-263) and the
  arg-max (:275; ties to the lowest class).  Above 64 classes the same tail runs as torch ops
  (`framework_tag_normalize_argmax`) and `normalize_path` names which of the two ran.  Returns `semantic_prediction`
  `[h,w]` int64, `semantic_prob` `[ncls,h,w]` (the normalised map; None unless `return_prob`), `class_divisor` `[ncls]`,
  `combine_path`, `normalize_path`, and per view `cluster_index` and `segment_topk` as `predict_knn_multiscale`."""
  if not views:
    raise ValueError('pseudo_labels_knn_multiscale needs at least one view')
  _require_gpu(label_tags, what='label_tags on')
  if label_tags.dim() != 1 or label_tags.shape[0] != int(num_classes):
    raise ValueError('pseudo_labels_knn_multiscale expects one tag per class')
  acc, combine_path, cluster_index, segment_topk = _knn_view_votes_sum(
      'pseudo_labels_knn_multiscale', embedding_model, prediction_model, views, image_hw, crop_size, stride,
      memory_prototypes, memory_prototype_labels, num_classes)
  hip = int(num_classes) <= _ffi.MAX_TAG_NORMALIZE_CLASSES
  tail = _ffi.tag_normalize_argmax if hip else framework_tag_normalize_argmax
  with torch.no_grad():
    prediction, prob, divisor = tail(acc, len(views), label_tags, floor, return_prob)
  return {'semantic_prediction': prediction, 'semantic_prob': prob, 'class_divisor': divisor,
          'combine_path': combine_path,
          'normalize_path': HIP_TAG_NORMALIZE_PATH if hip else FRAMEWORK_TAG_NORMALIZE_PATH,
          'cluster_index': cluster_index, 'segment_topk': segment_topk}


def save_image_memory(path, prototypes, prototype_labels):
  """`np.save` of `{'prototype', 'prototype_label'}` (prototype.py:207-211)."""
  segsort_others.save_memory_bank(path, prototypes, prototype_labels)


def _walk(trans, cam, walk_steps):
  """`trans <- trans . trans` `walk_steps` times, then `cam . trans` (pseudo_camrw_crf.py:159-164 =
  pseudo_softmaxrw_crf.py:165-170): fp32 library GEMMs (rocBLAS through torch.matmul)."""
  for _ in range(walk_steps):
    trans = torch.matmul(trans, trans)
  return torch.matmul(cam.reshape(cam.shape[0], -1).float(), trans).view(cam.shape)


def affinity_random_walk(embs_list, cam, walk_steps=6, scale=5.0, power=20):
  """Random walk of class activation maps `[K,h,w]` over the pixel affinity of one image
  (pseudo_camrw_crf.py:143-164).  `embs_list`: one `[1,C,h,w]` embedding
  per augmented view at 1/8 resolution.  The affinity, its mean over the views, the 20th
  power and the column normalisation are one fused HIP kernel; the walk is six fp32
  library GEMMs (rocBLAS through torch.matmul)."""
  with torch.no_grad():
    views = []
    for embs in embs_list:
      embs = embs / torch.norm(embs, dim=1)
      views.append(embs.reshape(embs.shape[1], -1))
    emb = torch.stack(views, 0).float().contiguous()          # [B,C,n]
    trans = _ffi.affinity_transition(emb, scale, power)
    return _walk(trans, cam, walk_steps)


def label_tags_from_map(label, num_classes):
  """The classes below `num_classes` that occur in a label map -> bool `[num_classes]` on the label's device
  (pseudo_softmaxrw_crf.py:102-106)."""
  label = torch.as_tensor(label)
  present = torch.unique(label.reshape(-1).long())
  tags = torch.zeros((num_classes,), dtype=torch.bool, device=label.device)
  tags[present[(present >= 0) & (present < num_classes)]] = True
  return tags


def flip_scale_views(image, scales, is_flip, crop_size):
  """The views of one image `[1,3,h,w]` in the reference's order (`create_image_pyramid` of
  spml/utils/general/others.py + `resize_with_pad`, pseudo_softmaxrw_crf.py:109-125): per scale the flipped view first
  (when `is_flip`), then the plain one; each resized bilinearly to `round(h * scale) x round(w * scale)` and
  zero-padded at the bottom / right to at least `crop_size`.  -> list of `(image [1,3,Hp,Wp], (rh, rw), is_flip)`,
  the `views` of `pseudo_labels_softmax`.  A host-side stand-in for the loader (cv2 there): not parity-pinned -- the
  synthetic mode's and for callers with float images; a decoded file goes through `device_views`, which is pinned
  (sizes `int(scale * side)`, not `round`)."""
  if image.dim() != 4 or image.shape[0] != 1:
    raise ValueError('flip_scale_views expects one image [1,3,H,W]')
  h, w = image.shape[-2:]
  views = []
  for scale in scales:
    if scale == 1:
      scaled = image
    else:
      size = (max(int(round(h * scale)), 1), max(int(round(w * scale)), 1))
      scaled = torch.nn.functional.interpolate(image, size=size, mode='bilinear', align_corners=False)
    rh, rw = scaled.shape[-2:]
    pad_h, pad_w = max(rh, int(crop_size[0])), max(rw, int(crop_size[1]))
    for flip in ((True, False) if is_flip else (False,)):
      view = torch.zeros((1, image.shape[1], pad_h, pad_w), dtype=image.dtype, device=image.device)
      view[:, :, :rh, :rw] = torch.flip(scaled, dims=[3]) if flip else scaled
      views.append((view, (rh, rw), flip))
  return views


def view_records(plan):
  """`spml_amd.data.transforms.plan_views`' dicts -> the numpy array of `_ffi.VIEW_PARAMS` records the launch reads."""
  records = np.zeros((len(plan),), dtype=_ffi.VIEW_PARAMS)
  for k, view in enumerate(plan):
    for name in ('image_off', 'label_off', 'new_h', 'new_w', 'pad_h', 'pad_w', 'flip'):
      records[name][k] = int(view[name])
  return records


_NORMALISATION = {}       # (device, means, stds) -> the two fp32 [3] tensors on that device


def _normalisation(device, pixel_means, pixel_stds):
  key = (str(device), tuple(float(v) for v in pixel_means), tuple(float(v) for v in pixel_stds))
  if key not in _NORMALISATION:
    _NORMALISATION[key] = (torch.tensor(key[1], dtype=torch.float32, device=device),
                           torch.tensor(key[2], dtype=torch.float32, device=device))
  return _NORMALISATION[key]


def views_from_records(rgb_u8, records, params_dev, mean, std, semantic_label=None):
  """The launch behind `device_views`, for a caller that planned the views itself and already has the records on the
  device (`params_dev`: the same bytes as uint8 -- `inference_cli.ImageSource` sends them up with the image in one
  copy).  -> (views, label views or None)."""
  from spml_amd.data import transforms
  plan = [{name: int(r[name]) for name in ('image_off', 'label_off', 'new_h', 'new_w', 'pad_h', 'pad_w')} for r in records]
  image_bytes, label_bytes = transforms.view_buffer_bytes(plan)
  with torch.no_grad():
    images = torch.empty((image_bytes // 4,), dtype=torch.float32, device=rgb_u8.device)
    labels = None if semantic_label is None else torch.empty((label_bytes // 8,), dtype=torch.int64, device=rgb_u8.device)
    _ffi.image_views(rgb_u8, semantic_label, records, params_dev, mean, std, images, labels)
  views, label_views_ = [], []
  for r, p in zip(records, plan):
    at, n = p['image_off'] // 4, 3 * p['pad_h'] * p['pad_w']
    views.append((images[at:at + n].view(1, 3, p['pad_h'], p['pad_w']), (p['new_h'], p['new_w']), bool(r['flip'])))
    if labels is not None:
      at, n = p['label_off'] // 8, p['new_h'] * p['new_w']
      label_views_.append(labels[at:at + n].view(p['new_h'], p['new_w']))
  return views, (label_views_ if labels is not None else None)


def device_views(rgb_u8, scales, is_flip, crop_size, pixel_means, pixel_stds, image_size=0, semantic_label=None):
  """The views of one decoded file, made on the GPU from its bytes by ONE launch (`spml_image_views_u8`): `rgb_u8` uint8
  `[h,w,3]` on the device -> what the reference's loader and programs make on the host per view (normalise,
  `create_image_pyramid` / `resize_with_interpolation` with cv2.INTER_LINEAR, mirror, `resize_with_pad` with zeros:
  inference_softmax_msc.py:90-103, inference_softmax.py:89-103) in the reference's order, sizes
  (`spml_amd.data.transforms.plan_views`: `int(scale * side)`) and arithmetic.  -> the `views` every `predict_*` /
  `pseudo_*` function takes, `(image [1,3,Hp,Wp], (rh, rw), is_flip)`, as slices of one allocation.  With
  `semantic_label` (uint8 `[h,w]` on the device) -> `(views, label views)`: the label of every view `[rh, rw]` int64
  (cv2.INTER_NEAREST, mirrored with its view), the `label_views` of `multiscale_prototypes`.  No CPU path."""
  from spml_amd.data import transforms
  _require_gpu(rgb_u8, what='got')
  if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or rgb_u8.dtype != torch.uint8:
    raise ValueError('device_views expects one decoded image, uint8 [h,w,3]')
  records = view_records(transforms.plan_views(rgb_u8.shape[0], rgb_u8.shape[1], scales, is_flip, crop_size, image_size))
  params_dev = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).to(rgb_u8.device)
  mean, std = _normalisation(rgb_u8.device, pixel_means, pixel_stds)
  views, labels = views_from_records(rgb_u8, records, params_dev, mean, std, semantic_label)
  return views if semantic_label is None else (views, labels)


def export_label_map(prediction, valid_hw, out_hw, color_map, out=None):
  """The tail of a label-inference program (inference_softmax.py:142-160) as ONE launch (`spml_label_export_u8`):
  `prediction` int64 `[pred_h,pred_w]` on the device, its valid top-left `valid_hw` rectangle resized with
  cv2.INTER_NEAREST's rule to `out_hw` (the file's own size) -> `(gray uint8 [out_h,out_w], rgb uint8 [out_h,out_w,3])`
  on the device, `rgb = color_map[gray]` (`color_map`: uint8 `[256,3]` on the device).  `out`: the two tensors to write
  into (slices of one buffer come down in one copy)."""
  with torch.no_grad():
    return _ffi.label_export(prediction, valid_hw, out_hw, color_map, out)


def crf_guide(rgb_u8, pixel_means, pixel_stds, out_hw=None):
  """The uint8 image the reference hands to its CRF (`inference_softmax_crf_msc.py:159-164`), from a decoded file's
  bytes by ONE launch (`spml_crf_guide_u8`): `rgb_u8` uint8 `[h,w,3]` on the device -> uint8 `[rh,rw,3]`, bit for bit
  `denormalized_uint8` of the un-flipped `out_hw` view `device_views` makes of the same bytes (`out_hw` None: the
  file's own size, the multi-view programs; the un-padded `test.image_size` view for the single-view ones,
  `inference_crf.py:247-252`).  Not the bytes themselves: the reference rebuilds the image from the normalised fp32
  input and that round trip lowers some (byte, channel) pairs by one.  No CPU path."""
  _require_gpu(rgb_u8, what='got')
  if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or rgb_u8.dtype != torch.uint8:
    raise ValueError('crf_guide expects one decoded image, uint8 [h,w,3]')
  mean, std = _normalisation(rgb_u8.device, pixel_means, pixel_stds)
  with torch.no_grad():
    return _ffi.crf_guide(rgb_u8, mean, std, pixel_means, pixel_stds, out_hw)


def export_scored_label_map(refined, before, valid_hw, out_hw, color_map, truth, num_classes, scores=None, out=None):
  """The tail of a program that ends in the dense CRF (`inference_crf.py:257-261` + `benchmark_by_mIoU.py:25-53`) as ONE
  launch (`spml_label_export_scored_u8`): `export_label_map` of `refined`, the same resampling of `before` (the labels
  before the CRF, int64 `[pred_h,pred_w]`, or None), both scored at `out_hw` against `truth` (uint8 `[out_h,out_w]` on
  the device, or None), and the count of output pixels the CRF changed.  `scores`: int64 `[2 * 3 * num_classes + 1]` on
  the device, accumulated INTO over the images of a list (a fresh zero tensor when None): `scores[:-1].view(2, 3, -1)`
  are the `iou_stats` tables after and before the CRF, `scores[-1]` the changed pixels.
  -> `(gray, rgb, scores)`."""
  _require_gpu(refined, what='got')
  with torch.no_grad():
    if scores is None:
      scores = torch.zeros((2 * 3 * int(num_classes) + 1,), dtype=torch.int64, device=refined.device)
    gray, rgb = _ffi.label_export_scored(refined, before, valid_hw, out_hw, color_map, truth, num_classes, scores, out)
  return gray, rgb, scores


def _embedded_views(embedding_model, views):
  """The view loop of the random-walk functions (pseudo_softmaxrw_crf.py:116-128 = pseudo_camrw_crf.py:139-142): the
  whole padded image of every view through `generate_embeddings(..., resize_as_input=True)`, consecutive views of one
  padded size in one call, in the memory format of the model.  Yields `(b, embedding [1,C,Hp,Wp] fp32, crop_hw, flip)`
  per view, `b` counting the views in call order; the caller holds `torch.no_grad()`."""
  nhwc = _is_channels_last(embedding_model)
  b = 0
  for part in _group_by_padded_size(views):
    images = torch.cat([v[0] for v in part], 0) if len(part) > 1 else part[0][0]
    if nhwc:
      images = images.contiguous(memory_format=torch.channels_last)
    embs = embedding_model.generate_embeddings({'image': images}, resize_as_input=True)['embedding'].float()
    for i, (_, crop_hw, flip) in enumerate(part):
      yield b, embs[i:i + 1], crop_hw, flip
      b += 1


def _walk_tail(cam_rw, image_hw, refine=None):
  """Where the four random-walk functions end: the walked maps `[ncls, h//8, w//8]` up-sampled to `image_hw` and their
  arg-max (`spml_upsample_argmax_i64`, pseudo_softmaxrw_crf.py:172-176) -> `semantic_prediction`; with `refine` =
  `(image_u8, crf)` the fused up-sampling + denseCRF of `random_walk_crf_refine` instead -> its fields."""
  if refine is not None:
    return random_walk_crf_refine(refine[0], cam_rw, refine[1])
  with torch.no_grad():
    return {'semantic_prediction': _ffi.upsample_argmax(cam_rw, image_hw[0], image_hw[1])}


def _walked_cams_softmax(name, embedding_model, prediction_model, views, image_hw, label_tags, combine, walk_steps,
                         background_threshold, scale, power):
  """`pseudo_labels_softmax` up to the walked maps, shared with `pseudo_labels_softmax_crf`: the argument checks (under
  the caller's `name`), the per-view launches, the transition matrix, the class maps and the walk.
  -> (cam, cam_rw `[ncls, h//8, w//8]`, head path, transition before the squarings)."""
  if combine not in _ffi.COMBINE_MODES:
    raise ValueError("combine must be 'prob_mean' or 'logit_mean'")
  if views:                                           # (an empty list is reported first, by _check_views)
    _require_gpu(label_tags, what='label_tags on')
  _check_views(name, views)
  out_hw = _eighth_size(name, image_hw)
  n = out_hw[0] * out_hw[1]
  device = views[0][0].device
  ncls = prediction_model.num_classes
  prediction_model.prepare_inference()          # once per image, as in predict_softmax_full_resolution
  units, canvas, acc, path = None, None, torch.zeros((ncls, n), dtype=torch.float32, device=device), None
  with torch.no_grad():
    for b, emb, crop_hw, flip in _embedded_views(embedding_model, views):
      if units is None:
        units = torch.empty((len(views), emb.shape[1], n), dtype=torch.float32, device=device)
      if canvas is None or canvas.shape[-2:] != emb.shape[-2:]:             # (one canvas per group of one padded size)
        canvas = torch.empty((1, ncls) + tuple(emb.shape[-2:]), dtype=torch.float32, device=device)
      path = prediction_model.accumulate_logits(emb, canvas.zero_(), 0, 0)
      _ffi.resample_unit(emb[0], crop_hw, flip, out_hw, units, b)
      _ffi.resample_classes_accumulate(canvas[0], crop_hw, flip, out_hw, acc, combine)
    trans = _ffi.affinity_transition(units, scale, power)
    cam = _ffi.cam_finalize(acc, len(views), label_tags, combine, background_threshold).view(ncls, *out_hw)
    cam_rw = _walk(trans, cam, walk_steps)
  return cam, cam_rw, path, trans


def pseudo_labels_softmax(embedding_model, prediction_model, views, image_hw, label_tags, combine='prob_mean',
                          walk_steps=6, background_threshold=None, scale=5.0, power=20, return_transition=False):
  """One image of the pseudo-label generation (`pyscripts/inference/pseudo_softmaxrw_crf.py:116-176` with
  combine='prob_mean', walk_steps=6; `pseudo_softmax.py:115-179` with combine='logit_mean', walk_steps=0), before
  the denseCRF.  `views`: list of `(image [1,3,Hp,Wp], (rh, rw), is_flip)` (`flip_scale_views`); `image_hw`: the
  un-padded image; `label_tags`: bool `[ncls]` device tensor (`label_tags_from_map`).

  Per view the whole padded image goes through `generate_embeddings(..., resize_as_input=True)` and the classifier
  head (:127-128; consecutive views of one padded size -- a flip pair -- share the backbone call, the head runs through
  `accumulate_logits` into a zero canvas), then `spml_resample_unit_f32` (crop, un-flip, 1/8 bilinear, unit columns,
  read through the embedding's strides: no NCHW copy of a channels-last map) and
  `spml_resample_classes_accumulate_f32` (the same for the logits, soft-maxed and summed in view order).  After the
  last view: `spml_affinity_transition_f32`, `spml_cam_finalize_f32`, the walk's GEMMs, `spml_upsample_argmax_i64`.
  Returns `cam`, `cam_rw` `[ncls, h//8, w//8]`, `semantic_prediction` `[h,w]` int64, `head_path`, and `transition`
  `[n,n]` (before the squarings) only with `return_transition`."""
  cam, cam_rw, path, trans = _walked_cams_softmax('pseudo_labels_softmax', embedding_model, prediction_model, views,
                                                  image_hw, label_tags, combine, walk_steps, background_threshold,
                                                  scale, power)
  out = dict({'cam': cam, 'cam_rw': cam_rw}, **_walk_tail(cam_rw, image_hw), head_path=path)
  if return_transition:
    out['transition'] = trans
  return out


def denormalized_uint8(image, pixel_means, pixel_stds):
  """The uint8 image the reference hands to its CRF (`pyscripts/inference/inference_softmax_crf_msc.py:159-164`), on the
  image's device: `image` float `[3,h,w]` (or `[1,3,h,w]`), the network's normalised input -> uint8 `[h,w,3]`.  numpy
  computes `image *= stds` and `image += means` (float32 by float64) in float64 and rounds each result to float32,
  multiplies by 255 in float32 and truncates; the same steps here.  (A value outside 0..255 wraps modulo 256, as numpy's
  cast does on the hosts this was compared on; the reference's images do not produce one.)"""
  if image.dim() == 4 and image.shape[0] == 1:
    image = image[0]
  if image.dim() != 3 or image.shape[0] != 3:
    raise ValueError('denormalized_uint8 expects one image [3,h,w]')
  stds = torch.as_tensor(np.asarray(pixel_stds, dtype=np.float64), device=image.device).view(1, 1, 3)
  means = torch.as_tensor(np.asarray(pixel_means, dtype=np.float64), device=image.device).view(1, 1, 3)
  x = image.float().permute(1, 2, 0)
  x = (x.double() * stds).float()
  x = (x.double() + means).float()
  x = x * torch.full((), 255.0, dtype=torch.float32, device=image.device)
  return (x.to(torch.int32) & 255).to(torch.uint8).contiguous()


def dense_crf_refine(image_u8, prob, crf):
  """The denseCRF tail of the reference's `*_crf*.py` programs (`inference_softmax_crf_msc.py:166-168`): `image_u8`
  uint8 `[h,w,3]` and `prob` fp32 `[ncls,h,w]` device tensors through `crf` (`spml_amd.models.crf.DenseCRF`).  Returns
  `semantic_prob` `[ncls,h,w]` (the refined marginals), `semantic_prediction` `[h,w]` int64 (their arg-max, from the
  kernel that writes them) and `crf_path`, the route the call took."""
  prob_out, prediction = crf.refine(image_u8, prob)
  return {'semantic_prob': prob_out, 'semantic_prediction': prediction,
          'crf_path': crf.path_name(prob.shape[1], prob.shape[2], prob.shape[0])}


def random_walk_crf_refine(image_u8, cam_rw, crf):
  """The tail the two random-walk programs share (`pseudo_softmaxrw_crf.py:172-187` = `pseudo_camrw_crf.py:166-181`):
  the walked maps `cam_rw` fp32 `[ncls, oh, ow]` (the programs: `h//8 x w//8`) are up-sampled bilinearly to the image,
  their arg-max is the label before the CRF, and the up-sampled maps go with `image_u8` uint8 `[h,w,3]` through `crf`
  (`spml_amd.models.crf.DenseCRF`).  One fused call (`spml_dense_crf_infer_upsampled_f32`): the up-sampled
  maps are formed inside the CRF's first kernel, which also writes the label before the CRF.  Returns `semantic_prob`
  `[ncls,h,w]` (the refined marginals), `semantic_prediction` `[h,w]` int64 (their arg-max),
  `semantic_prediction_before_crf` `[h,w]` int64 (what `spml_upsample_argmax_i64` gives) and `crf_path`."""
  prob, prediction, before = crf.refine_upsampled(image_u8, cam_rw)
  return {'semantic_prob': prob, 'semantic_prediction': prediction, 'semantic_prediction_before_crf': before,
          'crf_path': crf.path_name(image_u8.shape[0], image_u8.shape[1], cam_rw.shape[0])}


def pseudo_labels_softmax_crf(embedding_model, prediction_model, views, image_hw, label_tags, image_u8, crf,
                              combine='prob_mean', walk_steps=6, background_threshold=None, scale=5.0, power=20,
                              return_transition=False):
  """`pseudo_labels_softmax` with the denseCRF refinement of `pseudo_softmaxrw_crf.py:172-187`: the same chain up to
  `cam_rw`, then `random_walk_crf_refine` on `image_u8` (uint8 `[h,w,3]`, `denormalized_uint8` of the un-padded image)
  with `crf`.  Returns the fields of `pseudo_labels_softmax` -- `semantic_prediction` being the refined labels -- plus
  `semantic_prob`, `semantic_prediction_before_crf` (from the fused launch; equal to `pseudo_labels_softmax`'s
  `semantic_prediction`) and `crf_path`."""
  if tuple(image_u8.shape[:2]) != tuple(image_hw):
    raise ValueError('pseudo_labels_softmax_crf: image_u8 must be the un-padded image [h,w,3]')
  cam, cam_rw, path, trans = _walked_cams_softmax('pseudo_labels_softmax_crf', embedding_model, prediction_model, views,
                                                  image_hw, label_tags, combine, walk_steps, background_threshold,
                                                  scale, power)
  out = dict({'cam': cam, 'cam_rw': cam_rw, 'head_path': path}, **_walk_tail(cam_rw, image_hw, (image_u8, crf)))
  if return_transition:
    out['transition'] = trans
  return out


def _walked_cams_cam(name, embedding_model, views, image_hw, cam_planes, cam_classes, num_classes, alpha, walk_steps,
                     scale, power):
  """`pseudo_labels_cam` up to the walked maps, shared with `pseudo_labels_cam_crf`: the argument checks (under the
  caller's `name`), the embedding and `spml_resample_unit_f32` per view as in `_walked_cams_softmax` (no classifier
  head), the transition matrix and the walk.  The ingest launch comes first: it needs nothing of the network, and a key
  out of range or given twice is refused before the views go through it.
  -> (cam, cam_rw `[ncls, h//8, w//8]`, ingest path)."""
  h, w = image_hw
  out_hw = _eighth_size(name, image_hw)
  _check_views(name, views)
  if cam_planes is not None:
    _require_gpu(cam_planes, what='cam_planes on')
  n = out_hw[0] * out_hw[1]
  units = None
  with torch.no_grad():
    cam = _ffi.cam_ingest(cam_planes, cam_classes, (h, w), num_classes, alpha)
    for b, emb, crop_hw, flip in _embedded_views(embedding_model, views):
      if units is None:
        units = torch.empty((len(views), emb.shape[1], n), dtype=torch.float32, device=views[0][0].device)
      _ffi.resample_unit(emb[0], crop_hw, flip, out_hw, units, b)
    trans = _ffi.affinity_transition(units, scale, power)
    cam_rw = _walk(trans, cam, walk_steps)
  return cam, cam_rw, _ffi.cam_ingest_path_name(len(cam_classes), h, w, num_classes)


def pseudo_labels_cam(embedding_model, views, image_hw, cam_planes, cam_classes, num_classes, alpha=6, walk_steps=6,
                      scale=5.0, power=20):
  """One image of the image-tag recipe's first pseudo-label step (`pyscripts/inference/pseudo_camrw_crf.py:103-170`),
  before the denseCRF: the class activation maps of another model walked over the pixel affinity of this one.  `views`:
  list of `(image [1,3,Hp,Wp], (rh, rw), is_flip)` (the program: the flip pair at scale 1); `image_hw`: the un-padded
  image; `cam_planes`: fp32 `[K,h,w]` device tensor, the planes the image's CAM file carries (None for K = 0);
  `cam_classes`: their K dict keys (class - 1) as host integers.

  First `spml_cam_ingest_f32` -- the background row and the 1/8 reduction of :108-111 and :151-152 in one launch,
  without the `[ncls,h,w]` array; a bad key is refused here, before the network runs.  Per view the embedding and
  `spml_resample_unit_f32` as in `pseudo_labels_softmax` (:139-146; no classifier head).  After the last view:
  `spml_affinity_transition_f32` (:147-158), the walk's GEMMs (:159-164) and `spml_upsample_argmax_i64` (:167-170).  Returns `cam`, `cam_rw` `[ncls, h//8, w//8]`, `semantic_prediction`
  `[h,w]` int64 and `cam_path`."""
  cam, cam_rw, path = _walked_cams_cam('pseudo_labels_cam', embedding_model, views, image_hw, cam_planes, cam_classes,
                                       num_classes, alpha, walk_steps, scale, power)
  return dict({'cam': cam, 'cam_rw': cam_rw}, **_walk_tail(cam_rw, image_hw), cam_path=path)


def pseudo_labels_cam_crf(embedding_model, views, image_hw, cam_planes, cam_classes, num_classes, image_u8, crf, alpha=6,
                          walk_steps=6, scale=5.0, power=20):
  """`pseudo_labels_cam` with the denseCRF refinement of `pseudo_camrw_crf.py:166-181`: the same chain up to `cam_rw`,
  then `random_walk_crf_refine` on `image_u8` (uint8 `[h,w,3]`, `denormalized_uint8` of the un-padded image) with `crf`.
  Returns `cam`, `cam_rw`, `cam_path`, `semantic_prob`, `semantic_prediction` (the refined labels),
  `semantic_prediction_before_crf` (equal to `pseudo_labels_cam`'s `semantic_prediction`) and `crf_path`."""
  if tuple(image_u8.shape[:2]) != tuple(image_hw):
    raise ValueError('pseudo_labels_cam_crf: image_u8 must be the un-padded image [h,w,3]')
  cam, cam_rw, path = _walked_cams_cam('pseudo_labels_cam_crf', embedding_model, views, image_hw, cam_planes, cam_classes,
                                       num_classes, alpha, walk_steps, scale, power)
  return dict({'cam': cam, 'cam_rw': cam_rw, 'cam_path': path}, **_walk_tail(cam_rw, image_hw, (image_u8, crf)))


HIP_SEGMENT_VOTES_PATH = 'hip_segment_votes'
FRAMEWORK_SEGMENT_VOTES_PATH = 'framework_segment_votes'


def framework_segment_votes(clu, topk, ncls, hw):
  """The CRF input of the kNN program as the reference's own ops on the tensors' device (`inference_crf.py:240-245`):
  gather the retrieved labels per pixel (`topk[clu]`, `[h * w, k]`), one-hot over the classes, sum over the k retrievals,
  divide by k, `[h, w, C]` -> `[C, h, w]` fp32.  What the fused call gathers from a per-segment table; the route of
  `knn_votes_crf_refine` outside the kernel's limits and the yardstick of tools/bench_knn_crf.py.  As in the reference,
  a label outside `[0, ncls)` is an error.  (The divisor is a 0-dim tensor, not a Python number: by a number ATen's GPU
  kernel multiplies with the reciprocal instead, and count / k is what the reference's values mean.)"""
  h, w = hw
  score = topk[clu.reshape(-1)]                                                          # [h * w, k]
  votes = common_utils.one_hot(score, max_label=int(ncls)).sum(dim=1).float()            # :240-242
  votes = votes / torch.full((), float(score.shape[1]), dtype=torch.float32, device=votes.device)
  return votes.view(h, w, -1).permute(2, 0, 1).contiguous()                               # :243-245


def knn_votes_crf_refine(image_u8, cluster_index, segment_topk, num_classes, crf):
  """The tail of the kNN program with the denseCRF (`inference_crf.py:237-257`): `cluster_index` int64 `[h * w]` (or
  `[h, w]`), the dense segment id of every pixel of `image_u8` uint8 `[h,w,3]`, and `segment_topk` int64 `[m, k]`, the
  labels retrieved per segment (`Segsort.segment_predictions`), through `crf` (`spml_amd.models.crf.DenseCRF`).  One
  fused call (`spml_dense_crf_infer_votes_f32`): votes, log p, Q_0 and both labels are formed once per
  segment and gathered inside the CRF's first kernel; with more than 4096 segments the vote map is formed by
  `framework_segment_votes` and goes through `crf.refine`, and `votes_path` names which of the two ran.  Returns
  `semantic_prob` `[ncls,h,w]` (the refined marginals), `semantic_prediction` `[h,w]` int64 (their arg-max),
  `semantic_prediction_before_crf` `[h,w]` int64 (the arg-max of the votes, lowest class on ties), `crf_path` and
  `votes_path`."""
  _require_gpu(image_u8, cluster_index, segment_topk)
  h, w = int(image_u8.shape[0]), int(image_u8.shape[1])
  ncls = int(num_classes)
  if segment_topk.shape[0] <= _ffi.MAX_DENSE_CRF_VOTE_SEGMENTS:
    prob, prediction, before = crf.refine_votes(image_u8, cluster_index, segment_topk, ncls)
    votes_path = HIP_SEGMENT_VOTES_PATH
  else:
    with torch.no_grad():
      votes = framework_segment_votes(cluster_index, segment_topk, ncls, (h, w))
      before = torch.argmax(votes, dim=0)
    prob, prediction = crf.refine(image_u8, votes)
    votes_path = FRAMEWORK_SEGMENT_VOTES_PATH
  return {'semantic_prob': prob, 'semantic_prediction': prediction, 'semantic_prediction_before_crf': before,
          'crf_path': crf.path_name(h, w, ncls), 'votes_path': votes_path}


def predict_knn_full_resolution_crf(embedding_model, prediction_model, image, valid_hw, crop_size, stride,
                                    memory_prototypes, memory_prototype_labels, num_classes, image_u8, crf,
                                    semantic_ignore_index=255):
  """One image of the kNN label inference with the denseCRF (`pyscripts/inference/inference_crf.py:145-257`): the
  embedding and clustering steps of `predict_full_resolution` (:145-229, one shared helper), then
  `Segsort.segment_predictions` against the memory bank -- `[m, 20]` labels per segment and one segment id per pixel in
  the place of the per-pixel gather of :232-237 -- and `knn_votes_crf_refine` on `image_u8` (uint8 `[h,w,3]`,
  `denormalized_uint8` of the un-padded image: :247-252) with `crf`.  Returns the fields of `knn_votes_crf_refine` plus
  `cluster_index` `[h * w]` (dense segment ids) and `segment_topk` `[m, 20]`: `segment_topk[cluster_index]` is
  `predict_full_resolution`'s `semantic_score`."""
  if tuple(image_u8.shape[:2]) != tuple(valid_hw):
    raise ValueError('predict_knn_full_resolution_crf: image_u8 must be the un-padded image [h,w,3]')
  embeddings = _clustered_full_resolution(embedding_model, image, valid_hw, crop_size, stride, semantic_ignore_index)
  with torch.no_grad():
    topk, clu = prediction_model.segment_predictions(
        embeddings, {'semantic_memory_prototype': memory_prototypes,
                     'semantic_memory_prototype_label': memory_prototype_labels})
  if topk is None:
    raise ValueError('predict_knn_full_resolution_crf needs a memory bank and a clustering')
  out = knn_votes_crf_refine(image_u8, clu, topk.contiguous(), num_classes, crf)
  out.update(cluster_index=clu, segment_topk=topk)
  return out


def cam_with_background(cam_dict, image_hw, num_classes, alpha):
  """The class activation maps of one image as `pseudo_camrw_crf.py:108-111` stacks them: `cam_dict` `{k: [h,w]}` (the
  reference's on-disk format, keyed by class - 1) -> fp32 `[num_classes, h, w]` on the entries' device with entry `k` at
  class `k + 1`, zeros for the classes the dict does not carry and the background `(1 - max over the foreground) **
  alpha` at class 0.  Framework ops (one pass over the maps, not a hot path)."""
  h, w = image_hw
  values = [torch.as_tensor(v) for v in cam_dict.values()]
  device = values[0].device if values else torch.device('cpu')
  full = torch.zeros((num_classes, h, w), dtype=torch.float32, device=device)
  for k, v in zip(cam_dict.keys(), values):
    full[int(k) + 1] = v.to(torch.float32)
  if num_classes > 1:
    full[0] = torch.pow(1 - torch.max(full[1:], dim=0).values, alpha)
  else:
    full[0] = 1
  return full


def downsampled_cam(cam_full):
  """`pseudo_camrw_crf.py:151-152`: `[ncls, h, w]` -> `[ncls, h//8, w//8]` by the framework's own
  `F.interpolate(scale_factor=1/8, mode='bilinear')` -- the same op, so its `scale_factor` semantics are kept."""
  return torch.nn.functional.interpolate(cam_full.unsqueeze(0), scale_factor=1 / 8., mode='bilinear').squeeze(0)


HIP_SEGMENT_CAM_PATH = 'hip_segment_cam'
FRAMEWORK_SEGMENT_CAM_PATH = 'framework_segment_cam'


class NoLabelledPrototypeError(ValueError):
  """`densepose_segment_cam` found no segment with a label below `num_classes`: the image has no tag to propagate."""


def framework_densepose_segment_cam(nn_index, nn_value, proto_label, threshold, cluster_index, ncls, half_hw, out_hw):
  """The class maps of the DensePose pseudo-label program before their normalisation, as the reference's own ops on the
  tensors' device (`pseudo_denseposerw_crf.py:159-182`, with the body of
  `gather_multiset_labels_per_batch_by_nearest_neighbor` for `top_k = 1` from the retrieval on): the label of every
  pixel's nearest labelled prototype (`num_classes` where `nn_value < threshold`), one-hot over `ncls + 1` classes, `> 0`,
  the first `ncls` columns, `segment_mean` by the segment id, every row divided by its sum, `index_select` back to the
  pixels, `[h2, w2, ncls]` -> `[1, ncls, h2, w2]`, `F.interpolate(mode='bilinear')` to `out_hw` -> fp32 `[ncls, oh, ow]`.
  What `_ffi.segment_tag_cam` computes from a per-segment table; the route of `densepose_segment_cam` outside the
  kernel's limits and the yardstick of tools/bench_densepose_pseudo.py.  Two things are pinned where the reference is
  undefined, as the kernel pins them: a label outside `[0, ncls)` is no class (the reference's one_hot fails above
  `ncls`), and a row without a counted pixel is zeros (the reference has 0 / 0)."""
  ncls = int(ncls)
  (h2, w2), n = half_hw, nn_index.numel()
  labs = proto_label.reshape(-1)[nn_index.reshape(-1)].view(n, 1)
  labs = labs.masked_fill(nn_value.reshape(n, 1) < threshold, ncls)                      # models/utils.py:207-211
  labs = labs.masked_fill((labs < 0) | (labs > ncls), ncls)
  tags = (common_utils.one_hot(labs, ncls + 1).sum(dim=1) > 0).long()[:, :ncls]          # models/utils.py:217-221
  clu = cluster_index.reshape(-1)
  probs = common_utils.segment_mean(tags.float(), clu)                                   # :172-173
  total = probs.sum(dim=1, keepdim=True)
  probs = torch.where(total > 0, probs / total, torch.zeros_like(probs))                 # :174
  pixel = torch.index_select(probs, 0, clu).view(1, h2, w2, -1).permute(0, 3, 1, 2).contiguous()      # :175-180
  return torch.nn.functional.interpolate(pixel, size=tuple(out_hw), mode='bilinear')[0]  # :181-182


def densepose_segment_cam(clustered, label_tags, half_hw, out_hw, num_classes, label_divisor,
                          background_threshold=None):
  """The class activation maps of the DensePose pseudo-label program from the clustering of the half-resolution map
  (`pseudo_denseposerw_crf.py:153-190`).  `clustered`: what `generate_clusters` returns for that map (no pixel dropped:
  N = h2 * w2 rows); `label_tags`: bool `[num_classes]` device tensor.

  `prepare_prototype_labels` splits the segments by their semantic label and `calculate_prototypes_from_labels` forms
  their prototypes (:153-158); `ops.topk_affinity(k = 1)` retrieves every pixel's nearest prototype among those with a
  label below `num_classes` (:159-168: the masked retrieval of the training path, threshold -1, one image);
  `spml_segment_tag_cam_f32` counts the retrieved labels per segment, divides every row by its sum and resamples the map
  of rows bilinearly to `out_hw` (:169-182) -- above 64 classes or 4096 segments the same runs as framework ops
  (`framework_densepose_segment_cam`) and `cam_path` names which of the two ran; `spml_cam_finalize_f32` divides every
  class by its maximum, zeroes the classes the image does not carry and sets class 0 to `background_threshold` when one
  is given (:183-190; one view, so its division by the view count is exact).  `label_divisor` is what the reference
  passes to its retrieval, which does not read it.  Raises `NoLabelledPrototypeError` (a ValueError) when no prototype
  carries a label below `num_classes` (the reference's maps are NaN everywhere then).  Returns `cam` fp32 `[num_classes, oh, ow]`, `cam_path`,
  and what the new stage was fed: `nn_index`, `nn_value` `[N]`, `proto_label` `[S]`, `cluster_index` `[N]` (the
  re-indexed segment ids) and `num_segments`."""
  ncls = int(num_classes)
  _require_gpu(label_tags, what='label_tags on')
  if label_tags.dim() != 1 or label_tags.shape[0] != ncls:
    raise ValueError('densepose_segment_cam expects one tag per class')
  sem, embs = clustered['cluster_semantic_label'], clustered['cluster_embedding']
  (h2, w2) = half_hw
  if sem.numel() != h2 * w2:
    raise ValueError('densepose_segment_cam: %d clustered pixels for a %d x %d map (an ignored label drops pixels; map it '
                     'to num_classes first)' % (sem.numel(), h2, w2))
  with torch.no_grad():
    proto_label, clu = segsort_common.prepare_prototype_labels(sem, clustered['cluster_index'], sem.max() + 1)
    num_segments = int(proto_label.shape[0])
    protos = segsort_common.calculate_prototypes_from_labels(embs, clu, num_segments)
    valid = proto_label < ncls
    if not bool(valid.any()):
      raise NoLabelledPrototypeError('densepose_segment_cam: no prototype carries a label below num_classes = %d' % ncls)
    groups = torch.zeros_like(sem), torch.zeros_like(proto_label)
    nn_index, nn_value = ops.topk_affinity(embs, protos, 1, groups[0], groups[1], valid, masked_value=-2.0)
    nn_index, nn_value = nn_index.view(-1), nn_value.view(-1)
    if ncls <= _ffi.MAX_SEGMENT_TAG_CAM_CLASSES and num_segments <= _ffi.MAX_SEGMENT_TAG_CAM_SEGMENTS:
      acc = _ffi.segment_tag_cam(nn_index, nn_value, proto_label, -1.0, clu, num_segments, ncls, half_hw, out_hw)
      cam_path = HIP_SEGMENT_CAM_PATH
    else:
      acc = framework_densepose_segment_cam(nn_index, nn_value, proto_label, -1.0, clu, ncls, half_hw,
                                            out_hw).contiguous()
      cam_path = FRAMEWORK_SEGMENT_CAM_PATH
    cam = _ffi.cam_finalize(acc, 1, label_tags, 'prob_mean', background_threshold)
  return {'cam': cam, 'cam_path': cam_path, 'nn_index': nn_index, 'nn_value': nn_value, 'proto_label': proto_label,
          'cluster_index': clu, 'num_segments': num_segments}


def pseudo_labels_densepose_crf(embedding_model, image, valid_hw, semantic_label, instance_label, label_tags, image_u8,
                                crf, walk_steps=6, background_threshold=None, scale=5.0, power=20):
  """One image of the DensePose pseudo-label generation (`pyscripts/inference/pseudo_denseposerw_crf.py:112-222`): tags
  propagated from the labelled points to the segments, a random walk over the pixel affinity, the denseCRF.  `image`:
  the padded image `[1,3,Hp,Wp]`; `valid_hw`: the un-padded `(h, w)`; `semantic_label`, `instance_label`: int64 `[h,w]`
  (255 = ignore, a value from `num_classes` up = unlabelled); `label_tags`: bool `[num_classes]` (`label_tags_from_map`);
  `image_u8`: uint8 `[h,w,3]` (`denormalized_uint8` of the un-padded image); `crf`: `spml_amd.models.crf.DenseCRF`.

  `generate_embeddings(..., resize_as_input=True)` (:128-129), `F.interpolate` to half the padded size, cropped to
  `h//2 x w//2` (:130-135; framework ops, one pass); `spml_resample_unit_f32` to `h//8 x w//8` and
  `spml_affinity_transition_f32` on that one view (:137-142, :193-195); `resize_labels` to the half map with 255 mapped to
  `num_classes` so that no pixel is dropped (:121-123, :145-149); `generate_clusters` (:150-151);
  `densepose_segment_cam` (:153-190); the walk's GEMMs (:196-201); `random_walk_crf_refine` (:203-218: the up-sampling
  fused into the CRF's first kernel); the ignored pixels of the original label map set to 255 (:220-222).  Returns `cam`,
  `cam_rw` `[ncls, h//8, w//8]`, `semantic_prob` `[ncls,h,w]`, `semantic_prediction` `[h,w]` int64 (refined, 255 where
  ignored), `semantic_prediction_before_crf`, `crf_path`, `cam_path`, `cluster_index` `[h//2 * w//2]` and
  `num_segments`."""
  name = 'pseudo_labels_densepose_crf'
  if image.dim() != 4 or image.shape[0] != 1:
    raise ValueError(name + ' expects one image [1,3,Hp,Wp]')
  h, w = valid_hw
  if tuple(image_u8.shape[:2]) != (h, w) or tuple(semantic_label.shape) != (h, w) or \
      tuple(instance_label.shape) != (h, w):
    raise ValueError(name + ': image_u8 must be the un-padded image [h,w,3] and the labels [h,w]')
  out_hw = _eighth_size(name, valid_hw)
  _require_gpu(image, what='the image on')
  pad_h, pad_w = image.shape[-2:]
  half_hw = (h // 2, w // 2)
  ncls = int(embedding_model.num_classes)
  ignore = int(embedding_model.semantic_ignore_index)
  with torch.no_grad():
    if _is_channels_last(embedding_model):
      image = image.contiguous(memory_format=torch.channels_last)
    embs = embedding_model.generate_embeddings({'image': image}, resize_as_input=True)['embedding'].float()
    embs = torch.nn.functional.interpolate(embs, size=(pad_h // 2, pad_w // 2), mode='bilinear')
    embs = embs[:, :, :half_hw[0], :half_hw[1]].contiguous()
    units = torch.empty((1, embs.shape[1], out_hw[0] * out_hw[1]), dtype=torch.float32, device=image.device)
    _ffi.resample_unit(embs[0], half_hw, False, out_hw, units, 0)
    trans = _ffi.affinity_transition(units, scale, power)
    semantic_label = semantic_label.to(image.device).long()
    kept = torch.where(semantic_label == ignore, torch.full_like(semantic_label, ncls), semantic_label)
    s_lab = common_utils.resize_labels(kept.unsqueeze(0), half_hw)
    i_lab = common_utils.resize_labels(instance_label.to(image.device).long().unsqueeze(0), half_hw)
    clustered = embedding_model.generate_clusters(embs, s_lab, i_lab)
  stage = densepose_segment_cam(clustered, label_tags, half_hw, out_hw, ncls, embedding_model.label_divisor,
                                background_threshold)
  with torch.no_grad():
    cam_rw = _walk(trans, stage['cam'], walk_steps)
  out = {'cam': stage['cam'], 'cam_rw': cam_rw, 'cam_path': stage['cam_path'], 'cluster_index': stage['cluster_index'],
         'num_segments': stage['num_segments']}
  out.update(random_walk_crf_refine(image_u8, cam_rw, crf))
  out['semantic_prediction'] = out['semantic_prediction'].masked_fill(semantic_label == ignore, ignore)
  return out
