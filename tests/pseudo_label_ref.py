"""Plain fp32 torch restatement (CPU) of the pseudo-label scripts of the reference, the yardstick of
tests/test_pseudo_labels.py and tests/test_pseudo_labels_gpu.py.  Line numbers: `pyscripts/inference/
pseudo_softmaxrw_crf.py` ("rw") and `pyscripts/inference/pseudo_softmax.py` ("sm") of twke18/SPML.  The fixture
tests/golden/n7_pseudo_labels.npz was exec'd from those lines themselves (tools/gen_golden.py); this file is checked
against it, and the HIP kernels are checked against both."""
import torch
import torch.nn.functional as F

LOW_MARGIN = 2e-4        # labels are compared where top-1 minus top-2 >= LOW_MARGIN * max|cam_rw| (as for N6)


def network_output(coarse, pad_hw):
  """The stub network of the fixture: a stride-8 map [C, Hp/8+1, Wp/8+1] -> [1, C, Hp, Wp], what
  `resize_as_input=True` does to the real model's output (resnet_deeplab.py: bilinear, align_corners=False)."""
  return F.interpolate(coarse.float().unsqueeze(0), size=tuple(pad_hw), mode='bilinear', align_corners=False)


def resample_view(x, crop_hw, flip, out_hw):
  """rw:130-135 / 141-142: crop `x` [1, C, Hp, Wp] to the un-padded region, flip back, bilinear to `out_hw`."""
  x = x[:, :, :crop_hw[0], :crop_hw[1]]
  if flip:
    x = torch.flip(x, dims=[3])
  return F.interpolate(x, size=tuple(out_hw), mode='bilinear')


def view_unit_embedding(emb, crop_hw, flip, out_hw):
  """rw:130-136 -> [1, C, oh, ow] with unit columns (plain division, no epsilon)."""
  embs = resample_view(emb, crop_hw, flip, out_hw)
  return embs / torch.norm(embs, dim=1)


def view_classes(logit, crop_hw, flip, out_hw, combine):
  """rw:131-144 (`prob_mean`: softmax per view) / sm:130-144 (`logit_mean`: the resampled logits) -> [1, ncls, oh, ow]."""
  out = resample_view(logit, crop_hw, flip, out_hw)
  return F.softmax(out, dim=1) if combine == 'prob_mean' else out


def cams(view_terms, label_tags, combine, threshold=None):
  """rw:146-157 / sm:146-160: mean over the views, (softmax for `logit_mean`), every class over its maximum, untagged
  classes 0, class 0 = threshold when given -> [ncls, oh, ow]."""
  probs = torch.mean(torch.cat(view_terms, dim=0), dim=0)
  if combine == 'logit_mean':
    probs = F.softmax(probs, dim=0)
  ncls = probs.shape[0]
  max_prob = torch.max(probs.view(ncls, -1), dim=1)[0]
  cam = probs / max_prob.view(ncls, 1, 1)
  cam = cam.masked_fill((~label_tags).view(-1, 1, 1).expand(-1, cam.shape[1], cam.shape[2]), 0)
  if threshold is not None:
    cam[0] = threshold
  return cam


def transition(units, scale=5.0, power=20):
  """rw:137-139, 159-164: per view exp(scale * E^T E - scale), mean, ** power, column-normalised -> [n, n]."""
  affs = []
  for embs in units:
    flat = embs.view(embs.shape[1], -1)
    affs.append(torch.matmul(flat.t(), flat).mul_(scale).add_(-scale).exp_())
  aff = torch.mean(torch.stack(affs, dim=0), dim=0) ** power
  return aff / torch.sum(aff, dim=0, keepdim=True)


def random_walk(cam, trans, walk_steps):
  """rw:165-170: T <- T T `walk_steps` times, cam . T."""
  for _ in range(walk_steps):
    trans = torch.matmul(trans, trans)
  return torch.matmul(cam.reshape(cam.shape[0], -1), trans).view(cam.shape)


def upsampled(cam_rw, image_hw):
  """rw:173-175 (`cv2.resize(..., INTER_LINEAR)`: the same half-pixel mapping) -> [ncls, h, w]."""
  return F.interpolate(cam_rw.unsqueeze(0), size=tuple(image_hw), mode='bilinear', align_corners=False)[0]


def labels_and_margin(cam_rw, image_hw):
  """rw:176 -> (int64 [h, w], top-1 minus top-2 of the up-sampled maps)."""
  up = upsampled(cam_rw, image_hw)
  top2 = up.topk(2, dim=0).values
  return up.argmax(0), top2[0] - top2[1]


def pseudo_labels(outputs, view_meta, image_hw, label_tags, combine, walk_steps, threshold=None):
  """The whole chain for one image.  outputs: per view (embedding [1,C,Hp,Wp], logit [1,ncls,Hp,Wp]); view_meta: per
  view (rh, rw, flip)."""
  out_hw = (image_hw[0] // 8, image_hw[1] // 8)
  units, terms = [], []
  for (emb, logit), (rh, rw, flip) in zip(outputs, view_meta):
    units.append(view_unit_embedding(emb, (rh, rw), flip, out_hw))
    terms.append(view_classes(logit, (rh, rw), flip, out_hw, combine))
  cam = cams(terms, label_tags, combine, threshold)
  trans = transition(units)
  cam_rw = random_walk(cam, trans, walk_steps)
  pred, margin = labels_and_margin(cam_rw, image_hw)
  return {'units': units, 'cam': cam, 'trans': trans, 'cam_rw': cam_rw, 'semantic_prediction': pred, 'margin': margin}


# ---- the fixture ------------------------------------------------------------------------------------------------
RECIPES = (('rw', 'prob_mean', 6), ('sm0', 'logit_mean', 0), ('sm6', 'logit_mean', 6))    # tag, combine, squarings
NUM_CASES = 2


def fixture_case(g, ci):
  """Inputs of case `ci` of n7_pseudo_labels.npz -> (per-view network outputs on the CPU, view_meta, image_hw, tags)."""
  t = 'c%d_' % ci
  meta = [tuple(int(v) for v in row) for row in g[t + 'views']]             # (Hp, Wp, rh, rw, flip)
  outputs = [(network_output(g[t + 'emb%d' % vi], m[:2]), network_output(g[t + 'logit%d' % vi], m[:2]))
             for vi, m in enumerate(meta)]
  image_hw = tuple(int(v) for v in g[t + 'image_hw'])
  return outputs, [(m[2], m[3], bool(m[4])) for m in meta], image_hw, g[t + 'tags'].bool()
