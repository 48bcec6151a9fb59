"""Batched NLL entry points (spml_segsort_nll_batched_*, csrc/nll.hip): N independent problems, one launch per kernel.

Yardstick: the CPU oracle evaluated per problem, with the bounds `nll_check` of tests/test_kernels_gpu.py holds for the
single-problem kernels (at most 0.5 % of the pixels off by more than 2e-5 relative, none by 5e-3, the mean within 1e-5;
gradients within 1e-4 of their scale outside the ill-conditioned pixels, 1e-3 inside, 2e-5 on average), on inputs of
the recipe of `test_nll_vs_oracle_weighted_grad` -- and bit-equality with the single-problem entry points called once
per problem on the same slices."""
import functools

import pytest
import torch

from oracle import spml_oracle as O
from test_kernels_gpu import ill_conditioned_pixels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C32 = 4

SIZES_P = (64, 31, 0, 1000, 33)     # below a tile, an empty problem, several workgroups, a grid smaller than the launch's
SIZES_M = (5, 1, 3, 97, 33)         # a single prototype, two prototype tiles (33), four (97)
# upstream gradient: another magnitude per problem (powers of two and not), so that a gscale shared between
# problems would push the small ones' transposed fragments into the f16 subnormals
GRAD_SCALES = (1.0, 2.0 ** -10, 1.0, 3.0e-3, 700.0)


def ffi():
  from spml_amd import _ffi
  return _ffi


def _plain_nll(emb, sem, own, protos, p_sem, kappa):
  """loss.py:56-82 with group_mode != 'segsort+' (:71-72) in the oracle's operations: the numerator is the own
  segment's similarity alone."""
  sim = ((emb @ protos.t()) * kappa).exp()
  same = sem.view(-1, 1) == p_sem.view(1, -1)
  num = sim.gather(1, own.view(-1, 1))
  den = (sim * (~same).float()).sum(1, keepdim=True) + num
  return -(num / den).log()


class Problem:
  pass


def _problem(p, m, d, kappa, mode, seed, gscale):
  """One problem of the recipe of test_nll_vs_oracle_weighted_grad + its oracle values and gradients (CPU)."""
  gen = torch.Generator().manual_seed(seed)
  q = Problem()
  q.p, q.m = p, m
  q.protos = O.normalize_embedding(torch.randn(m, d, generator=gen))
  q.own = torch.randint(0, m, (p,), generator=gen)
  q.emb = O.normalize_embedding(q.protos[q.own] + 0.8 * torch.randn(p, d, generator=gen))
  p_sem = torch.randint(0, 21, (m,), generator=gen)
  sem = p_sem[q.own].clone()
  flip = torch.rand(p, generator=gen) < 0.2
  sem[flip] = torch.randint(0, 21, (int(flip.sum()),), generator=gen)
  q.wgt = torch.rand(p, generator=gen) * 1e-4 * gscale          # non-uniform upstream gradient
  if mode & 1:                                                    # tag sets: the class bit (+ a second bit on some prototypes)
    extra = torch.randint(0, 21, (m,), generator=gen)
    has = torch.rand(m, generator=gen) < 0.3
    p_tags = O.one_hot(p_sem, 21) | (O.one_hot(extra, 21) * has.view(-1, 1).long())
    tags = O.one_hot(sem, 21)
    w = (2 ** torch.arange(21, dtype=torch.long)).view(1, -1)
    q.px_code, q.pr_code = (tags * w).sum(1), (p_tags * w).sum(1)
  else:
    q.px_code, q.pr_code = sem, p_sem
  q.nll = q.de = q.dp = q.ill = q.de64 = None
  if p:
    def oracle(dtype):
      e = q.emb.to(dtype, copy=True).requires_grad_(True)
      pr = q.protos.to(dtype, copy=True).requires_grad_(True)
      if mode & 2:
        nll = _plain_nll(e, sem, q.own, pr, p_sem, kappa)
      elif mode & 1:
        nll = O.set_segsort_nll(e, tags, q.own, pr, p_tags, kappa)
      else:
        nll = O.segsort_nll(e, sem, q.own, pr, p_sem, kappa)
      (nll.view(-1) * q.wgt.to(dtype)).sum().backward()
      return nll.detach().view(-1), e.grad, pr.grad
    q.nll, q.de, q.dp = oracle(torch.float32)
    q.de64 = oracle(torch.float64)[1]           # the yardstick's own error: see _check_vs_oracle
    q.ill = ill_conditioned_pixels(q.emb, q.own, q.px_code, q.protos, q.pr_code, kappa, mode) if not (mode & 2) \
        else torch.zeros(p, dtype=torch.bool)
  return q


@functools.lru_cache(maxsize=None)
def _case(sizes_p, sizes_m, d, kappa, mode, seed, scales=None):
  """The problems of a case (computed once, shared by the tests that use it, never modified)."""
  scales = scales or tuple(GRAD_SCALES[i % len(GRAD_SCALES)] for i in range(len(sizes_p)))
  return tuple(_problem(p, m, d, kappa, mode, seed + 101 * i, scales[i])
               for i, (p, m) in enumerate(zip(sizes_p, sizes_m)))


def _concat(probs):
  first, own_abs = 0, []
  for q in probs:
    own_abs.append(q.own + first)
    first += q.m
  cat = lambda name: torch.cat([getattr(q, name) for q in probs]).to(DEV).contiguous()
  return (cat('emb'), torch.cat(own_abs).to(DEV), cat('px_code'), cat('protos'), cat('pr_code'), cat('wgt'),
          [q.p for q in probs], [q.m for q in probs])


def _run_batched(probs, kappa, mode):
  F = ffi()
  emb, own_abs, px_code, protos, pr_code, wgt, ps, ms = _concat(probs)
  nll, stats = F.segsort_nll_batched_fwd(emb, own_abs, px_code, ps, protos, pr_code, ms, kappa, mode)
  de, dp = F.segsort_nll_batched_bwd(emb, own_abs, px_code, ps, protos, pr_code, ms, kappa, mode, stats, wgt)
  torch.cuda.synchronize()
  return nll, stats, de, dp


def _check_vs_oracle(probs, nll, de, dp):
  """The assertions of nll_check (tests/test_kernels_gpu.py), problem by problem -- except its two pixel COUNTS (the
  inputs' own ill-conditioned pixels and the pixels off by more than 2e-5, 0.5 % each), which are taken over the
  pixels of the call: one such pixel is already 1 - 3 % of a problem of 31 .. 90 pixels (the seeds are chosen, by
  the oracle's count alone, so that the call stays under the cap)."""
  nll, de, dp = nll.cpu(), de.cpu(), dp.cpu()
  lo = first = 0
  n_px = sum(q.p for q in probs)
  n_ill = sum(int(q.ill.sum()) for q in probs if q.p)
  assert n_ill <= 5e-3 * n_px, 'the inputs themselves are ill-conditioned: %d of %d pixels' % (n_ill, n_px)
  # `ill_conditioned_pixels` is a threshold (pos < own / 256): a pixel just outside it (own / pos = 251 in one seed
  # tried) cancels nearly as badly, and there the fp32 oracle itself is off from its own fp64 evaluation by more than
  # the 1e-4 the kernels are held to.  The seeds are chosen, on the CPU alone, so that the yardstick's own error
  # outside the flagged pixels takes at most a quarter of that bound.
  for i, q in enumerate(probs):
    if q.p:
      own_err = (q.de.double() - q.de64).abs()[~q.ill]
      assert not own_err.numel() or own_err.max().item() <= 2.5e-5 * q.de.abs().max().item() + 1e-12, \
          'problem %d: the fp32 oracle itself is off by %.3g of the gradient scale outside the ill-conditioned ' \
          'pixels: choose another seed' % (i, own_err.max().item() / q.de.abs().max().item())
  n_off = 0
  for i, q in enumerate(probs):
    got_nll, got_de, got_dp = nll[lo:lo + q.p], de[lo:lo + q.p], dp[first:first + q.m]
    lo, first = lo + q.p, first + q.m
    if q.p == 0:
      assert not got_dp.any(), 'problem %d has no pixels: its prototypes receive no gradient' % i
      continue
    rel = (got_nll - q.nll).abs() / q.nll.abs().clamp(min=1.0)
    print('problem %d (P %d, M %d): off %.3g max rel %.3g mean diff %.3g' % (
        i, q.p, q.m, (rel > 2e-5).float().mean(), rel.max(), abs(got_nll.mean().item() - q.nll.mean().item())))
    n_off += int((rel > 2e-5).sum())
    assert rel.max().item() < 5e-3, i
    assert abs(got_nll.mean().item() - q.nll.mean().item()) <= 1e-5 * max(1.0, abs(q.nll.mean().item())), i
    for g_, w_, name in ((got_de, q.de, 'd_emb'), (got_dp, q.dp, 'd_protos')):
      scale = w_.abs().max().item()
      err = (g_ - w_).abs()
      print('  %s: max err %.3g mean err %.3g scale %.3g' % (name, err.max(), err.mean(), scale))
      assert err.max().item() <= 1e-3 * scale + 1e-12, (i, name)
      assert err.mean().item() <= 2e-5 * scale + 1e-12, (i, name)
      good = err[~q.ill] if name == 'd_emb' else (err if not q.ill.any() else err[:0])
      if good.numel():
        assert good.max().item() <= 1e-4 * scale + 1e-12, (i, name, int(q.ill.sum()))
  print('pixels off by more than 2e-5: %d of %d' % (n_off, n_px))
  assert n_off <= 5e-3 * n_px, 'too many pixels off: %d of %d' % (n_off, n_px)


def _check_vs_single(probs, kappa, mode, nll, stats, de, dp, exact_dp):
  """Once per problem through the single-problem entry points, on the same slices."""
  F = ffi()
  lo = first = 0
  for i, q in enumerate(probs):
    sl, sm = slice(lo, lo + q.p), slice(first, first + q.m)
    lo, first = lo + q.p, first + q.m
    if q.p == 0:
      continue
    args = (q.emb.to(DEV), q.own.to(DEV), q.px_code.to(DEV), q.protos.to(DEV), q.pr_code.to(DEV), kappa, mode)
    nll1, stats1 = F.segsort_nll_fwd(*args)
    de1, dp1 = F.segsort_nll_bwd(*args, stats1, q.wgt.to(DEV))
    assert torch.equal(nll[sl], nll1), i
    assert torch.equal(stats[sl], stats1), i
    assert torch.equal(de[sl], de1), i
    if exact_dp:
      assert torch.equal(dp[sm], dp1), (i, (dp[sm] - dp1).abs().max().item())
    else:                       # reordered fp32 atomics (the bound of test_nll_32_bit_code_path_is_identical)
      torch.testing.assert_close(dp[sm], dp1, rtol=1e-5, atol=2e-5 * dp1.abs().max().item())


@pytest.fixture
def deterministic():
  before = ffi().set_deterministic(True)
  yield
  ffi().set_deterministic(before)


@pytest.mark.parametrize('mode', [C32, 1 | C32, 2 | C32])
def test_mixed_sizes_against_the_oracle_and_the_single_problem_calls(mode):
  """Cases 1, 2, 5 and 6: a problem below a tile, an empty one, a single prototype, two prototype tiles, grids smaller
  than the launch's; another gradient magnitude per problem; LABEL, TAGSET and PLAIN."""
  probs = _case(SIZES_P, SIZES_M, 66, 16.0, mode, 7)
  nll, stats, de, dp = _run_batched(probs, 16.0, mode)
  _check_vs_oracle(probs, nll, de, dp)
  _check_vs_single(probs, 16.0, mode, nll, stats, de, dp, exact_dp=False)


@pytest.mark.parametrize('mode', [C32, 1 | C32])
def test_prototype_gradient_equals_the_single_problem_calls_in_deterministic_mode(deterministic, mode):
  probs = _case(SIZES_P, SIZES_M, 66, 16.0, mode, 7)
  out = _run_batched(probs, 16.0, mode)
  _check_vs_single(probs, 16.0, mode, *out, exact_dp=True)
  again = _run_batched(probs, 16.0, mode)
  for a, b in zip(out, again):
    assert torch.equal(a, b)


def _small_sizes(n, seed):
  gen = torch.Generator().manual_seed(seed)
  return (tuple(int(v) for v in torch.randint(1, 91, (n,), generator=gen)),
          tuple(int(v) for v in torch.randint(1, 41, (n,), generator=gen)))


@pytest.mark.parametrize('n', [33, 1])
def test_more_problems_than_one_descriptor_takes_and_a_single_one(n):
  """Case 3: 33 problems cross the 32-problem descriptor (two launches per kernel); one problem."""
  ps, ms = _small_sizes(n, 5) if n > 1 else ((1000,), (97,))
  probs = _case(ps, ms, 66, 12.0, C32, 10 if n > 1 else 21)
  nll, stats, de, dp = _run_batched(probs, 12.0, C32)
  _check_vs_oracle(probs, nll, de, dp)
  _check_vs_single(probs, 12.0, C32, nll, stats, de, dp, exact_dp=False)


@pytest.mark.parametrize('d', [80, 65])
def test_both_ends_of_the_width_bucket(d):
  """Case 4: D = 80 (five full k-steps) and D = 65 (one channel in the fifth k-step and in the third d-tile)."""
  probs = _case(SIZES_P, SIZES_M, d, 16.0, C32, 9)
  nll, stats, de, dp = _run_batched(probs, 16.0, C32)
  _check_vs_oracle(probs, nll, de, dp)
  _check_vs_single(probs, 16.0, C32, nll, stats, de, dp, exact_dp=False)


def test_nothing_to_do_and_refusals():
  F = ffi()
  lib = F.lib()
  assert lib.spml_segsort_nll_batched_supported(66, C32) == 1
  assert lib.spml_segsort_nll_batched_supported(64, C32) == 0
  assert lib.spml_segsort_nll_batched_supported(66, 0) == 0
  e = torch.zeros(0, 66, device=DEV)
  i64 = torch.zeros(0, dtype=torch.int64, device=DEV)
  pr = torch.nn.functional.normalize(torch.randn(7, 66), dim=1).to(DEV)
  code = torch.zeros(7, dtype=torch.int64, device=DEV)
  nll, stats = F.segsort_nll_batched_fwd(e, i64, i64, [0, 0], pr, code, [3, 4], 10.0, C32)     # no pixel at all
  assert nll.shape == (0,)
  probs = _case((40,), (5,), 66, 10.0, C32, 3)
  emb, own_abs, px_code, protos, pr_code, wgt, _, _ = _concat(probs)
  with pytest.raises(F.SpmlHipError, match='refused|invalid'):          # pixels without prototypes
    F.segsort_nll_batched_fwd(emb, own_abs, px_code, [20, 20], protos, pr_code, [5, 0], 10.0, C32)
  with pytest.raises(F.SpmlHipError, match='unsupported|not supported'):
    F.segsort_nll_batched_fwd(emb, own_abs, px_code, [40], protos, pr_code, [5], 10.0, 0)       # 64-bit codes


@pytest.mark.parametrize('d', [64, 32])
def test_the_op_falls_back_to_the_looped_path_outside_the_bucket(d):
  """Case 7: D = 64 (the pipelined kernels' bucket) and D = 32 (the DensePose predictor's): `ops.segsort_nll_batched`
  evaluates the problems one by one -- the values and gradients of `ops.segsort_nll` per problem."""
  from spml_amd import ops
  assert not ops.segsort_nll_batched_supported(d, C32)
  probs = _case((64, 0, 300, 33), (5, 3, 40, 33), d, 12.0, C32, 29)
  emb, own_abs, px_code, protos, pr_code, wgt, ps, ms = _concat(probs)
  with ffi_deterministic():
    e, pr = emb.clone().requires_grad_(True), protos.clone().requires_grad_(True)
    nll = ops.segsort_nll_batched(e, own_abs, px_code, ps, pr, pr_code, ms, 12.0, C32)
    (nll * wgt).sum().backward()
    lo = first = 0
    for q in probs:
      if q.p:
        e1, pr1 = q.emb.to(DEV).requires_grad_(True), q.protos.to(DEV).requires_grad_(True)
        nll1 = ops.segsort_nll(e1, q.own.to(DEV), q.px_code.to(DEV), pr1, q.pr_code.to(DEV), 12.0, C32)
        (nll1 * q.wgt.to(DEV)).sum().backward()
        assert torch.equal(nll[lo:lo + q.p], nll1)
        assert torch.equal(e.grad[lo:lo + q.p], e1.grad)
        assert torch.equal(pr.grad[first:first + q.m], pr1.grad)
      lo, first = lo + q.p, first + q.m


class ffi_deterministic:
  def __enter__(self):
    self.before = ffi().set_deterministic(True)

  def __exit__(self, *exc):
    ffi().set_deterministic(self.before)


IMG_SIM_SWITCHES = ('SPML_IMG_SIM_BATCHED_PROTOS', 'SPML_IMG_SIM_BATCHED', 'SPML_IMG_SIM_STREAMS',
                    'SPML_IMG_SIM_RECORD_STREAM')


def _loss_head(monkeypatch, batched, env=None):
  """The loss head of tests/step_helpers.py (batch 4, crop 257), no SPML_IMG_SIM_STREAMS set; `env`: further
  SPML_IMG_SIM_* switches."""
  from step_helpers import loss_head
  for switch in IMG_SIM_SWITCHES:
    monkeypatch.delenv(switch, raising=False)
  if not batched:
    monkeypatch.setenv('SPML_IMG_SIM_BATCHED', '0')
  for k, v in (env or {}).items():
    monkeypatch.setenv(k, v)
  step = loss_head(DEV)
  calls = []
  from spml_amd import _ffi
  real = _ffi.segsort_nll_batched_fwd
  monkeypatch.setattr(_ffi, 'segsort_nll_batched_fwd', lambda *a, **k: (calls.append(len(a[3])), real(*a, **k))[1])
  out, emb, _ = step()
  loss = out['sem_ann_loss'] + out['sem_occ_loss'] + out['img_sim_loss']
  loss.backward()
  torch.cuda.synchronize()
  monkeypatch.setattr(_ffi, 'segsort_nll_batched_fwd', real)
  return out['img_sim_loss'].detach().clone(), emb.grad.clone(), calls


def test_call_site_batched_against_looped(deterministic, monkeypatch):
  """Case 8: the predictor's image-similarity term, SPML_IMG_SIM_BATCHED=0 against the default: the loss to 1e-6
  relative (only the final reduction differs: at most 2^15 positive terms per image), d loss / d embedding
  bit-identical in deterministic mode, and the batched path bit-identical to itself."""
  loop_loss, loop_grad, loop_calls = _loss_head(monkeypatch, batched=False)
  loss, grad, calls = _loss_head(monkeypatch, batched=True)
  assert loop_calls == [] and calls == [4]                 # one batched call for the four images / none
  print('img_sim looped %.9g batched %.9g' % (loop_loss.item(), loss.item()))
  assert abs(loss.item() - loop_loss.item()) <= 1e-6 * abs(loop_loss.item())
  assert torch.equal(grad, loop_grad), (grad - loop_grad).abs().max().item()
  loss2, grad2, _ = _loss_head(monkeypatch, batched=True)
  assert torch.equal(loss2, loss) and torch.equal(grad2, grad)


@pytest.mark.parametrize('env', [{'SPML_IMG_SIM_BATCHED_PROTOS': '0'}, {'SPML_IMG_SIM_RECORD_STREAM': '0'}],
                         ids=['per-image-protos', 'no-record-stream'])
def test_call_site_looped_routes_against_the_default_loop(deterministic, monkeypatch, env):
  """Case 8, the other two looped routes against the default loop (SPML_IMG_SIM_BATCHED=0), in deterministic mode: the
  loss and d loss / d embedding are bit-identical.  Prototypes per image instead of from one call: the segment sums
  are 64-bit fixed point with one constant scale (csrc/segsum.hip), so a sum over one image's pixels has the same bits
  whichever launch forms it.  No record_stream calls: they move no data."""
  loop_loss, loop_grad, loop_calls = _loss_head(monkeypatch, batched=False)
  loss, grad, calls = _loss_head(monkeypatch, batched=False, env=env)
  assert loop_calls == [] and calls == []
  print('img_sim default loop %.9g %s %.9g, max |d grad| %.3e' % (loop_loss.item(), env, loss.item(),
                                                                  (grad - loop_grad).abs().max().item()))
  assert torch.equal(loss, loop_loss), (loss.item(), loop_loss.item())
  assert torch.equal(grad, loop_grad), (grad - loop_grad).abs().max().item()
