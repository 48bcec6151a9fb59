"""Inputs and yardsticks of the kNN + dense-CRF tests (tests/test_knn_crf.py, test_knn_crf_gpu.py): the tail of
`pyscripts/inference/inference_crf.py:237-257` of twke18/SPML, restated on the CPU from the existing yardstick
(tests/dense_crf_ref.py, fp64 over all pixel pairs) and the reference's one-hot lines in numpy.  Nothing here touches the
code under test."""
import functools

import numpy as np

import dense_crf_ref

# (h, w, C): one pixel; N below one 32-pixel tile; two classes; ragged N; N a multiple of the tile; many tiles; both
# 32-class tiles with long rows; one row; one class (Q must be all ones)
SHAPES = [(1, 1, 3), (7, 5, 2), (16, 24, 2), (33, 47, 5), (32, 40, 21), (64, 64, 21), (17, 129, 64), (1, 300, 4), (9, 9, 1)]
MARGIN = 1e-3                      # labels are compared where the yardstick's top two marginals are further apart
LABEL_CAP = 0.02                   # largest share of pixels that may fall under MARGIN, for every shape
SEED = 1


def votes_case(h, w, c, seed, k=20):
  """-> (image uint8 [h, w, 3], clu int64 [h * w], topk int64 [m, k]): what the retrieval hands to the tail.  The segments
  are a min(4, h) x min(6, w) grid over the image with shuffled ids; every segment has a dominant class d < live (live =
  c - 1 when c > 2: the last class gets no vote at all) with nd in [k/2 + 1, k] votes, the rest drawn uniformly from
  [0, live), the row shuffled -- so no row has a tied maximum."""
  image = dense_crf_ref.blocky(h, w, c, seed)[0]
  gy, gx = min(4, h), min(6, w)
  m = gy * gx
  cell = (np.arange(h) * gy // h)[:, None] * gx + (np.arange(w) * gx // w)[None, :]
  clu = np.random.RandomState(seed + 200).permutation(m)[cell].reshape(-1).astype(np.int64)
  rng = np.random.RandomState(seed + 201)
  live = c - 1 if c > 2 else c
  topk = np.empty((m, k), np.int64)
  for s in range(m):
    d = rng.randint(0, live)
    nd = rng.randint(k // 2 + 1, k + 1)
    row = np.concatenate([np.full(nd, d), rng.randint(0, live, size=k - nd)])
    topk[s] = rng.permutation(row)
  return image, clu, topk


def vote_map(clu, topk, c, hw):
  """`inference_crf.py:240-245` in numpy: one-hot of the gathered labels, sum over k, float32, / k, [h, w, C] -> [C, h, w].
  (A label outside [0, c) matches no column here; the reference's one_hot would refuse it.)"""
  semantic_topk = topk[clu.reshape(-1)]                                           # [h * w, k]
  semantic_prob = (semantic_topk[:, :, None] == np.arange(c)[None, None, :]).astype(np.int64)
  semantic_prob = semantic_prob.sum(axis=1).astype(np.float32) / semantic_topk.shape[1]
  semantic_prob = semantic_prob.reshape(hw[0], hw[1], -1).astype(np.float32)
  return np.ascontiguousarray(semantic_prob.transpose(2, 0, 1))


def under_margin(want):
  """-> (keep: bool [h, w], the pixels outside the margin; the share left out).  One class: every pixel is kept."""
  if want.shape[0] < 2:
    return np.ones(want.shape[1:], bool), 0.0
  top = np.sort(want, axis=0)
  keep = (top[-1] - top[-2]) > MARGIN
  return keep, 1.0 - float(keep.mean())


@functools.lru_cache(maxsize=None)
def yardstick(shape, parameters, seed=SEED):
  """(image, clu, topk, votes fp32 [c, h, w], fp64 Q [c, h, w]) of one case, computed once and shared by the tests;
  read-only."""
  h, w, c = shape
  image, clu, topk = votes_case(h, w, c, seed)
  votes = vote_map(clu, topk, c, (h, w))
  want = dense_crf_ref.dense_crf(image, votes, **dense_crf_ref.PARAMETER_SETS[parameters])
  for a in (image, clu, topk, votes, want):
    a.setflags(write=False)
  return image, clu, topk, votes, want
