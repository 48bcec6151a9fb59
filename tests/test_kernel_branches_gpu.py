"""Every dispatch branch of the kernels that the training step and the kNN inference rest on -- the up-sampled
cross-entropy backward (csrc/upsample_ce.hip), top-k retrieval (csrc/topk.hip), the segment prototypes (csrc/segsum.hip)
and the affinity transition (csrc/affinity.hip) -- case by case: the comment beside a case names the template instance
or branch it reaches.  The yardstick is always a plain fp64 evaluation of the same operation in torch, never the kernel
under test nor another kernel of this library; every bound is the one the older tests of the same kernel hold
(profiles/kernel_branch_parity.md lists the margins)."""
import pytest
import torch

from spml_amd import _ffi
from test_edge_cases_gpu import unit
from test_upsample_ce_gpu import _case, check_loss_and_gradient

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture
def deterministic():
  before = _ffi.set_deterministic(True)
  yield
  _ffi.set_deterministic(before)


# ---------------------------------------------------------------------------------------------------------------------
# up-sampled cross-entropy: the un-tiled backward uce_bwd<24 | 32 | 64> and its out_range
# (N, C, h, w, H, W, share of ignored pixels, channels-last input)
UCE_GATHER_CASES = [
    (2, 21, 9, 9, 65, 65, 0.2, True),      # uce_bwd<24>, the recipe's 21 classes, ratio 7.2, two images
    (1, 2, 4, 4, 48, 48, 0.1, True),       # uce_bwd<24>, lower end of its class range (22 padded channels), ratio 12
    (1, 24, 9, 7, 60, 50, 0.3, True),      # uce_bwd<24>, upper end: no padded channel; h != w, ratios 6.7 / 7.1
    (1, 25, 5, 6, 41, 47, 0.2, True),      # uce_bwd<32>, lower end: the first width uce_bwd<24> would truncate
    (2, 32, 9, 7, 60, 50, 0.1, False),     # uce_bwd<32>, upper end; NCHW-contiguous input
    (1, 33, 6, 5, 47, 41, 0.0, True),      # uce_bwd<64>, lower end; no ignored pixel; odd sizes
    (1, 64, 4, 4, 40, 40, 0.5, True),      # uce_bwd<64>, upper end; exact ratio 10; one block, 16 of 256 threads live
    (1, 64, 17, 17, 65, 65, 0.1, True),    # uce_bwd<64>, two blocks (289 low-resolution pixels); 76 912 B of LDS asked
    (1, 21, 5, 6, 41, 47, 0.2, True),      # just above the limit: 75 936 B (the tiled kernel runs up to 73 728 B)
]
# kept beside them for contrast: the tiled kernel next to its limit, 68 592 B (a case of tests/test_upsample_ce_gpu.py)
UCE_TILED_NEIGHBOUR = (3, 40, 17, 17, 65, 66, 0.5, False)


@pytest.mark.parametrize('n,c,h,w,hh,ww,ign,cl', UCE_GATHER_CASES)
def test_upsample_ce_gather_backward(n, c, h, w, hh, ww, ign, cl):
  # a later change of the LDS formula must not move the case back onto the tiled kernel unnoticed
  assert _ffi.upsample_ce_bwd_path_name(n, c, h, w, hh, ww) == 'gather'
  check_loss_and_gradient(n, c, h, w, hh, ww, ign, cl)


def test_upsample_ce_tiled_neighbour_of_the_limit():
  n, c, h, w, hh, ww, ign, cl = UCE_TILED_NEIGHBOUR
  assert _ffi.upsample_ce_bwd_path_name(n, c, h, w, hh, ww) == 'tiled'
  check_loss_and_gradient(n, c, h, w, hh, ww, ign, cl)
  assert _ffi.upsample_ce_bwd_path_name(0, c, h, w, hh, ww) == 'unsupported'
  assert _ffi.upsample_ce_bwd_path_name(n, 65, h, w, hh, ww) == 'unsupported'
  assert _ffi.upsample_ce_bwd_path_name(65536, 5, 7, 9, 7, 9) == 'gather'      # N beyond gridDim.z


def test_upsample_ce_gather_backward_is_bit_identical_run_to_run():
  """The header's "deterministic, no atomics" holds for the gather kernel too."""
  n, c, h, w, hh, ww = 2, 21, 9, 9, 65, 65
  assert _ffi.upsample_ce_bwd_path_name(n, c, h, w, hh, ww) == 'gather'
  logits, labels = _case(n, c, h, w, hh, ww, 0.2, seed=12)
  nhwc = logits.permute(0, 2, 3, 1).contiguous()
  scale = torch.full((1,), 1.0 / (n * hh * ww), device=DEV)
  outs = []
  for _ in range(2):
    result, lse = _ffi.upsample_ce_fwd(nhwc, labels, 255)
    outs.append((result.clone(), lse.clone(), _ffi.upsample_ce_bwd(nhwc, labels, lse, 255, scale).clone()))
  assert all(torch.equal(a, b) for a, b in zip(*outs))
  assert outs[0][2].abs().max().item() > 0


# ---------------------------------------------------------------------------------------------------------------------
# top-k: the seven KS widths, the k = 8 / 9 split, k > M, exact ties, the masked form
def _topk_check(idx, val, sim64, k, exact=None, tag=''):
  """idx / val [Q, k] against the stable descending sort of the fp64 matrix `sim64` [Q, M]: values within 3e-6; indices
  equal wherever both neighbouring gaps of the reference exceed 1e-5 (the rule of test_topk_small_and_limit_shapes) or
  where `exact` marks the reference value as one the kernel reproduces bit for bit (masked entries: ties by index);
  at most 1 % of the entries may be left out.  With k > M: M entries by that rule, then idx == 0 and val == -inf."""
  q, m = sim64.shape
  kk = min(k, m)
  want_v, want_i = torch.sort(sim64, dim=1, descending=True, stable=True)
  idx, val = idx.cpu(), val.cpu()
  err = (val[:, :kk].double() - want_v[:, :kk]).abs().max().item()
  nxt = torch.cat([want_v, torch.full((q, 1), -float('inf'), dtype=torch.float64)], 1)[:, 1:kk + 1]
  gaps = want_v[:, :kk] - nxt                                          # (+inf behind the last of M candidates)
  prev = torch.cat([torch.full((q, 1), float('inf'), dtype=torch.float64), gaps[:, :-1]], 1)
  safe = (gaps > 1e-5) & (prev > 1e-5)
  if exact is not None:
    safe |= exact(want_v[:, :kk])
  left_out = 1.0 - safe.double().mean().item()
  print('topk %s: max value error %.3e (bound 3e-6), %.2f %% of the indices left out (bound 1 %%)' % (tag, err, 100 * left_out))
  assert err <= 3e-6, err
  assert left_out <= 0.01, left_out
  assert torch.equal(idx[:, :kk][safe], want_i[:, :kk][safe])
  assert bool(((idx >= 0) & (idx < m)).all())
  if k > m:
    assert bool((idx[:, m:] == 0).all()) and bool((val[:, m:] == -float('inf')).all())
  return want_v, want_i


def _topk_inputs(q, m, d):
  gen = torch.Generator().manual_seed(q + m + d)
  return unit(gen, q, d), unit(gen, m, d), gen


@pytest.mark.parametrize('q,m,d,k', [
    (37, 300, 40, 8),       # KS = 3 (D 33..48), <KMAX 8, WAVES 4>, k = 8: the last list size of the four-wave kernel
    (5, 40, 48, 8),         # KS = 3 upper edge; 2 prototype tiles for 4 waves: waves 0 and 2 stream nothing
    (70, 200, 144, 8),      # KS = 9 upper edge (D 81..144); three query tiles
    (33, 129, 130, 9),      # KS = 9; k = 9: first size of <KMAX 32, WAVES 2>; M = 4 tiles + 1 row, Q = 1 tile + 1 row
    (35, 161, 272, 9),      # KS = 17 upper edge (D 145..272)
    (40, 257, 258, 20),     # KS = 17; the recipe's k = 20
    (33, 97, 33, 32),       # KS = 3 lower edge (D = 33); k = 32, the limit
    (64, 95, 32, 32),       # KS = 2 upper edge (D <= 32); M one row short of three tiles
    (31, 64, 80, 1),        # KS = 5 upper edge (D 65..80); k = 1; Q one row short of a tile
])
def test_topk_width_buckets_and_the_k_split(q, m, d, k):
  qs, pr, _ = _topk_inputs(q, m, d)
  idx, val = _ffi.topk_affinity(qs.to(DEV), pr.to(DEV), k)
  _topk_check(idx, val, qs.double() @ pr.double().t(), k, tag=str((q, m, d, k)))


def test_topk_width_limit():
  with pytest.raises(_ffi.SpmlHipError):                               # KS = 34: refused, D <= 528
    _ffi.topk_affinity(torch.zeros(4, 529, device=DEV), torch.zeros(6, 529, device=DEV), 3)
  assert _ffi.lib().spml_topk_workspace_bytes(4, 6, 529, 3) == 0


@pytest.mark.parametrize('q,m,d,k', [(7, 5, 64, 8),       # k > M in the four-wave kernel: one tile, three idle waves
                                     (7, 20, 66, 32)])    # k > M in the two-wave kernel
def test_topk_more_neighbours_asked_than_prototypes_exist(q, m, d, k):
  """include/spml_hip.h, A11/B3: the first M entries are all M candidates in order, the rest idx == 0, val == -inf."""
  qs, pr, _ = _topk_inputs(q, m, d)
  idx, val = _ffi.topk_affinity(qs.to(DEV), pr.to(DEV), k)
  _topk_check(idx, val, qs.double() @ pr.double().t(), k, tag=str((q, m, d, k)))
  assert torch.equal(idx.cpu()[:, :m].sort(1).values, torch.arange(m).expand(q, m))


@pytest.mark.parametrize('k', [8, 20])
def test_topk_exact_ties_of_a_zero_query(k):
  """Every product is exactly 0: the ties span all ten tiles, both lane halves and every wave, so the answer rests on
  both tie-breaks -- the strict `>` of the per-lane insertion (a later row never displaces an equal earlier one) and
  the `v == bv && x < bx` branch of the merge of the 2 * WAVES lists."""
  gen = torch.Generator().manual_seed(300 + 40)
  pr = unit(gen, 300, 40)
  qs = torch.zeros(3, 40)
  qs[1] = unit(gen, 1, 40)[0]                                          # (an ordinary row between the two zero rows)
  idx, val = _ffi.topk_affinity(qs.to(DEV), pr.to(DEV), k)
  for row in (0, 2):
    assert torch.equal(idx[row].cpu(), torch.arange(k)), idx[row].tolist()
    assert bool((val[row] == 0).all())
  _topk_check(idx[1:2], val[1:2], qs[1:2].double() @ pr.double().t(), k, tag='zero-query neighbour, k=%d' % k)


@pytest.mark.parametrize('k', [8, 20])
def test_topk_exact_ties_of_duplicated_prototypes(k):
  """Prototype rows duplicated at known positions -- inside one lane's list (rows 1, 2), across the lane halves (3, 4),
  across a 32-row tile boundary (31, 32), across the wave split (63, 64 with four waves, 159, 160 with two) and far
  apart (10, 290) -- give bit-equal affinities (the same operands meet in the same order): the list must be
  non-increasing and, wherever two consecutive values are bit-equal, ascending in the index."""
  gen = torch.Generator().manual_seed(77)
  m, d = 300, 40
  pr = unit(gen, m, d)
  pairs = [(1, 2), (3, 4), (31, 32), (63, 64), (159, 160), (10, 290)]
  for a, b in pairs:
    pr[b] = pr[a]
  # three queries close to every duplicated row: both copies are in their top-k
  qs = torch.cat([torch.nn.functional.normalize(pr[a].view(1, d) + 0.1 * torch.randn(3, d, generator=gen), dim=1)
                  for a, _ in pairs])
  idx, val = _ffi.topk_affinity(qs.to(DEV), pr.to(DEV), k)
  idx, val = idx.cpu(), val.cpu()
  assert bool((val[:, :-1] >= val[:, 1:]).all())
  equal = val[:, :-1] == val[:, 1:]
  assert bool((idx[:, :-1][equal] < idx[:, 1:][equal]).all())
  found = set()
  for row in range(qs.shape[0]):
    a, b = pairs[row // 3]
    assert idx[row, 0].item() == a and idx[row, 1].item() == b, (row, idx[row, :3].tolist(), val[row, :3].tolist())
    if equal[row, 0]:
      found.add((a, b))
  assert found == set(pairs), found                                    # not vacuous: every pair tied bit for bit
  sim = qs.double() @ pr.double().t()
  want_v = torch.sort(sim, dim=1, descending=True).values[:, :k]
  assert (val.double() - want_v).abs().max().item() <= 3e-6


@pytest.mark.parametrize('q,m,d,k', [(37, 300, 40, 8),      # masked form in <KMAX 8, WAVES 4>, KS = 3
                                     (33, 129, 130, 9)])    # ... and in <KMAX 32, WAVES 2>, KS = 9
def test_topk_masked_form_orders_the_disallowed_candidates_too(q, m, d, k):
  """Four groups.  Groups 0 and 1 share the prototypes at random, about 30 % of them invalid; group 2 owns six
  prototypes, all invalid (query 0: every entry is masked_value, idx == arange(k)); group 3 owns five, three of them
  valid (query 1: the three allowed ones in descending order, then the disallowed ones by ascending index).  All k
  columns are compared: a masked entry's value is reproduced exactly, so its index is never left out."""
  qs, pr, gen = _topk_inputs(q, m, d)
  pg = torch.randint(0, 2, (m,), generator=gen)
  valid = torch.rand(m, generator=gen) > 0.3
  special = torch.randperm(m, generator=gen)[:11]
  pg[special[:6]] = 2
  valid[special[:6]] = False
  pg[special[6:]] = 3
  valid[special[6:9]] = True
  valid[special[9:]] = False
  qg = torch.randint(0, 2, (q,), generator=gen)
  qg[0], qg[1] = 2, 3
  qg[q - 1] = 3                                                         # (and once in the last, partial query tile)
  masked_value = -2.0
  idx, val = _ffi.topk_affinity(qs.to(DEV), pr.to(DEV), k, qg.to(DEV), pg.to(DEV), valid.to(torch.uint8).to(DEV),
                                masked_value)
  sim = qs.double() @ pr.double().t()
  allowed = (qg.view(-1, 1) == pg.view(1, -1)) & valid.view(1, -1)
  ref = torch.where(allowed, sim, torch.full_like(sim, masked_value))
  _topk_check(idx, val, ref, k, exact=lambda v: v == masked_value, tag='masked ' + str((q, m, d, k)))
  idx, val = idx.cpu(), val.cpu()
  assert torch.equal(idx[0], torch.arange(k)) and bool((val[0] == masked_value).all())
  for row in (1, q - 1):
    mine = special[6:9]
    order = mine[torch.argsort(sim[row, mine], descending=True)]
    others = torch.tensor([j for j in range(m) if j not in mine.tolist()][:k - 3])
    assert torch.equal(idx[row], torch.cat([order, others])), idx[row].tolist()
    assert bool((val[row, 3:] == masked_value).all()) and bool((val[row, :3] > -1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# segment prototypes: the NC widths, both accumulation modes, id handling, the eps branch, `accumulate`
EPS = 1e-12                                                             # kEps of csrc/common.hpp (normalize_embedding)


def _segment_reference(x, ids, m, gsel):
  """fp64: index_add_ over the in-range ids, s / max(|s|, eps); d(sum(protos * gsel)) / dx by autograd."""
  xr = x.double().requires_grad_(True)
  inside = (ids >= 0) & (ids < m)
  sums = torch.zeros(m, x.shape[1], dtype=torch.float64).index_add(0, ids[inside], xr[inside])
  protos = sums / sums.norm(dim=1, keepdim=True).clamp(min=EPS)
  (protos * gsel.double()).sum().backward()
  return protos.detach(), xr.grad, inside


def _segment_check(x, ids, m, gen, det, tag):
  """Forward and backward of one scene against the fp64 expression, at the bounds of test_segment_prototypes_fwd_bwd
  (2e-6 on the prototypes, 1e-5 * max(scale, 1) on dx) and, in deterministic mode, of test_determinism_gpu.py (2e-7)."""
  p, d = x.shape
  gsel = torch.randn(m, d, generator=gen)
  want, want_dx, inside = _segment_reference(x, ids, m, gsel)
  assert _ffi.deterministic() == det
  protos, sums = _ffi.segment_sum_normalize(x.to(DEV), ids.to(DEV), m)
  bound = 2e-7 if det else 2e-6
  err = (protos.cpu().double() - want).abs().max().item()
  dx = _ffi.segment_sum_normalize_bwd(gsel.to(DEV), sums, ids.to(DEV), p).cpu()
  scale = want_dx.abs().max().item()
  err_dx = (dx.double() - want_dx).abs().max().item()
  print('segment prototypes %s%s: error %.3e (bound %.0e), dx error %.3e (bound %.3e)' % (
      tag, ' deterministic' if det else '', err, bound, err_dx, 1e-5 * max(scale, 1.0)))
  assert err <= bound, err
  assert err_dx < 1e-5 * max(scale, 1.0), (err_dx, scale)
  empty = torch.ones(m, dtype=torch.bool)
  empty[ids[inside]] = False
  assert bool((protos.cpu()[empty] == 0).all())                          # segments without pixels: exact zeros
  assert bool((dx[~inside] == 0).all())                                  # pixels of no segment: no gradient
  return protos.cpu(), dx


def _runs(gen, p, m, lengths):
  """ids [p]: runs of the given lengths (cycled), a fresh random segment per run."""
  out = []
  i = 0
  while sum(len(o) for o in out) < p:
    out.append(torch.full((lengths[i % len(lengths)],), int(torch.randint(0, m, (1,), generator=gen))))
    i += 1
  return torch.cat(out)[:p].contiguous()


def _segment_width_case(d, det):
  gen = torch.Generator().manual_seed(1500 + d)
  p, m = 1500, 40
  x = torch.nn.functional.normalize(torch.randn(p, d, generator=gen), dim=1)
  ids = _runs(gen, p, m, [50, 7, 33, 1, 64, 20])
  ids[ids == 1] = 0                                                      # segment 1 stays empty
  _segment_check(x, ids, m, gen, det, 'D=%d' % d)


SEGMENT_WIDTHS = [
    130,       # NC = 3 (D 129..192), two live columns in the last 64
    192,       # NC = 3 upper edge
    320,       # NC = 5 upper edge (D 193..320)
    321,       # NC = 9 lower edge (six columns per lane in use)
    576,       # NC = 9 upper edge
    577,       # NC = 17 lower edge (ten columns per lane in use)
    1088,      # NC = 17 upper edge: the widest row the kernel takes
]


@pytest.mark.parametrize('d', SEGMENT_WIDTHS)
def test_segment_prototype_widths(d):
  _segment_width_case(d, False)                                          # segsum_kernel<NC, false>: fp32 atomics


@pytest.mark.parametrize('d', SEGMENT_WIDTHS)
def test_segment_prototype_widths_deterministic(deterministic, d):
  _segment_width_case(d, True)                                           # segsum_kernel<NC, true>: fixed-point sums


@pytest.mark.parametrize('det', [False, True])
def test_segment_prototype_width_limit(det):
  before = _ffi.set_deterministic(det)
  try:
    with pytest.raises(_ffi.SpmlHipError):                               # NC would be 18: refused, D <= 1088
      _ffi.segment_sum_normalize(torch.zeros(64, 1089, device=DEV), torch.zeros(64, dtype=torch.long, device=DEV), 3)
  finally:
    _ffi.set_deterministic(before)


def _id_pattern(name, gen, m):
  if name == 'run1':                       # run length 1: every pixel flushes the one before
    return torch.randint(0, m, (700,), generator=gen)
  if name == 'run32':                      # runs end exactly on the 32-pixel chunk boundary: one flush per wave
    return _runs(gen, 32 * 21, m, [32])
  if name == 'run64':                      # a run spans two chunks exactly: two waves add into the same segment
    return _runs(gen, 64 * 11, m, [64])
  if name in ('p1', 'p31', 'p33'):         # fewer pixels than a chunk / one pixel into the second wave
    return _runs(gen, int(name[1:]), m, [5, 9])
  assert name == 'outside'
  # a mixture of out-of-range ids between real runs: -1, M, and two ids whose LOW half is the real segment 3 -- a kernel
  # that dropped the high half of its two-readlane id would add their rows to segment 3
  ids = _runs(gen, 600, m, [11, 4, 32])
  for at, bad in ((5, -1), (40, m), (64, 2 ** 32 + 3), (65, 2 ** 32 + 3), (130, -(2 ** 32) + 3), (300, m + 7),
                  (301, -1), (599, 2 ** 32 + 3)):
    ids[at] = bad
  ids[131:140] = -(2 ** 32) + 3                                          # a run of them
  ids[200:210] = 3                                                       # segment 3 itself has pixels
  return ids


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('d', [66, 130])                                 # NC = 2 and NC = 3
@pytest.mark.parametrize('pattern', ['run1', 'run32', 'run64', 'p1', 'p31', 'p33', 'outside'])
def test_segment_prototype_id_patterns(pattern, d, det):
  """include/spml_hip.h, A4: an id outside [0, M) marks a pixel of no segment -- it adds nothing to any prototype
  (the fp64 reference sums the in-range pixels only, so rows leaking into segment 3 would show) and gets dx == 0."""
  before = _ffi.set_deterministic(det)
  try:
    m = 40
    gen = torch.Generator().manual_seed(len(pattern) * 1000 + d)
    ids = _id_pattern(pattern, gen, m)
    x = torch.nn.functional.normalize(torch.randn(ids.shape[0], d, generator=gen), dim=1)
    _segment_check(x, ids, m, gen, det, '%s D=%d' % (pattern, d))
  finally:
    _ffi.set_deterministic(before)


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('d', [66, 130])
def test_segment_prototype_of_a_zero_sum_takes_the_eps_branch(d, det):
  """Segment 5 is the run x, -x, y, -y inside one chunk: its sum is exactly zero in any arithmetic, so its prototype is
  zero and proto_bwd_rows takes `|s| < eps`: its pixels get d_protos / eps (the fp64 expression gives the same: the
  clamp passes no gradient to the norm)."""
  before = _ffi.set_deterministic(det)
  try:
    m = 12
    gen = torch.Generator().manual_seed(5 + d)
    ids = _runs(gen, 256, m, [16, 9, 32])
    ids[ids == 5] = 6
    ids[64:68] = 5
    x = torch.nn.functional.normalize(torch.randn(256, d, generator=gen), dim=1)
    x[65], x[67] = -x[64], -x[66]
    gsel = torch.randn(m, d, generator=gen)
    want, want_dx, _ = _segment_reference(x, ids, m, gsel)
    assert bool((want[5] == 0).all())
    protos, sums = _ffi.segment_sum_normalize(x.to(DEV), ids.to(DEV), m)
    assert bool((sums[5] == 0).all()) and bool((protos[5] == 0).all())
    torch.testing.assert_close(protos.cpu().double(), want, rtol=0, atol=2e-7 if det else 2e-6)
    dx = _ffi.segment_sum_normalize_bwd(gsel.to(DEV), sums, ids.to(DEV), 256).cpu().double()
    zero = ids == 5
    # the pixels of the zero-sum segment: 1e-5 of THEIR scale (|d_protos| / eps ~ 1e12) ...
    scale = want_dx[zero].abs().max().item()
    assert scale > 1e11
    err = (dx[zero] - want_dx[zero]).abs().max().item()
    # ... and everything else at 1e-5 of its own: one bound over both would hide the ordinary pixels behind 1e12
    scale_rest = want_dx[~zero].abs().max().item()
    err_rest = (dx[~zero] - want_dx[~zero]).abs().max().item()
    print('segment eps branch D=%d%s: relative dx error %.3e on the zero-sum segment, %.3e elsewhere (bound 1e-5)' % (
        d, ' deterministic' if det else '', err / scale, err_rest / max(scale_rest, 1.0)))
    assert err < 1e-5 * scale and err_rest < 1e-5 * max(scale_rest, 1.0)
  finally:
    _ffi.set_deterministic(before)


@pytest.mark.parametrize('d', [66, 130])
def test_segment_prototype_backward_accumulates_into_dx(d):
  """`accumulate` != 0: gather_rows<true> adds the gradient to what dx holds (out-of-range pixels keep their value)."""
  m = 40
  gen = torch.Generator().manual_seed(900 + d)
  ids = _id_pattern('outside', gen, m)
  p = ids.shape[0]
  x = torch.nn.functional.normalize(torch.randn(p, d, generator=gen), dim=1)
  gsel = torch.randn(m, d, generator=gen)
  _, want_dx, inside = _segment_reference(x, ids, m, gsel)
  prefill = torch.randn(p, d, generator=gen)
  protos, sums = _ffi.segment_sum_normalize(x.to(DEV), ids.to(DEV), m)
  dx = prefill.clone().to(DEV)
  out = _ffi.segment_sum_normalize_bwd(gsel.to(DEV), sums, ids.to(DEV), p, accumulate=1, dx=dx)
  assert out.data_ptr() == dx.data_ptr()
  want = prefill.double() + want_dx
  scale = want.abs().max().item()
  err = (dx.cpu().double() - want).abs().max().item()
  print('segment accumulate D=%d: dx error %.3e (bound %.3e)' % (d, err, 1e-5 * max(scale, 1.0)))
  assert err < 1e-5 * max(scale, 1.0)
  assert torch.equal(dx.cpu()[~inside], prefill[~inside])
  # ... and the default of the wrapper overwrites
  plain = _ffi.segment_sum_normalize_bwd(gsel.to(DEV), sums, ids.to(DEV), p).cpu()
  assert (plain.double() - want_dx).abs().max().item() < 1e-5 * max(want_dx.abs().max().item(), 1.0)
  with pytest.raises(_ffi.SpmlHipError):
    _ffi.segment_sum_normalize_bwd(gsel.to(DEV), sums, ids.to(DEV), p, accumulate=1)


# ---------------------------------------------------------------------------------------------------------------------
# affinity transition: partial tiles, C = 1, KS > 4, the branches of ipow, more than three views
def _affinity_views(views, c, n, gen):
  """Unit columns around two directions (so that the 20th power leaves more than the diagonal); C = 1: signs."""
  centres = torch.randn(2, c, generator=gen)
  which = torch.arange(n) % 2
  e = centres[which].t().unsqueeze(0) + 0.35 * torch.randn(views, c, n, generator=gen)
  return (e / e.norm(dim=1, keepdim=True)).contiguous()


@pytest.mark.parametrize('scale', [5.0, 1.0])
@pytest.mark.parametrize('power', [1,       # ipow: one pass, r = x
                                   3,       # odd: the `p & 1` branch taken twice
                                   20])     # 0b10100: the branch skipped and taken in turn (the recipe's value)
@pytest.mark.parametrize('views,c,n', [
    (1, 1, 15),       # C = 1 (KS = 1, 15 of 16 channels padding); n < 32: one partial tile
    (2, 17, 33),      # KS = 2 with one live channel in the second slice; n = 32 + 1: a second tile of one row / column
    (4, 130, 70),     # KS = 9 (> 4); four views; three tiles, the last with 6 rows
    (1, 64, 32),      # exactly one full tile
])
def test_affinity_transition_branches(views, c, n, power, scale):
  """include/spml_hip.h: T = A^power / column sums, A = mean over the views of exp(scale * E^T E - scale), in fp64."""
  gen = torch.Generator().manual_seed(views * 1000 + c + n)
  emb = _affinity_views(views, c, n, gen)
  got = _ffi.affinity_transition(emb.to(DEV), scale=scale, power=power).cpu()
  e64 = emb.double()
  aff = torch.exp(scale * torch.bmm(e64.transpose(1, 2), e64) - scale).mean(0)
  want = aff ** power
  want = want / want.sum(0, keepdim=True)
  big = want > 1e-6
  rel = ((got.double() - want).abs()[big] / want[big]).max().item()
  print('affinity %s power %d scale %g: max relative error %.3e over the entries above 1e-6 (bound 2e-4), column sums '
        'off by %.3e (bound 1e-5)' % ((views, c, n), power, scale, rel, (got.sum(0) - 1).abs().max().item()))
  torch.testing.assert_close(got.double(), want, rtol=2e-4, atol=1e-9)
  torch.testing.assert_close(got.sum(0), torch.ones(n), rtol=1e-5, atol=1e-5)


def test_affinity_transition_width_limit():
  with pytest.raises(_ffi.SpmlHipError):                                 # C > 1024: refused
    _ffi.affinity_transition(torch.zeros(1, 1025, 8, device=DEV))
