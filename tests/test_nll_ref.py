"""The fp64 NLL reference (tests/nll_ref.py) against the oracle, the committed goldens and finite differences, and
the guarantees of the case table (tests/nll_cases.py) that tests/test_nll_branches_gpu.py relies on: every pixel of
every case keeps the margin and its kind, every case names its route.  CPU only."""
import collections

import pytest
import torch

import nll_cases as NC
import nll_ref as R
from conftest import load_golden
from oracle import spml_oracle as O
from test_nll_batched_gpu import _plain_nll


def _tags_to_mask(tags):
  w = (2 ** torch.arange(tags.shape[1], dtype=torch.long)).view(1, -1)
  return (tags.long() * w).sum(1)


def _random_problem(p, m, d, seed, n_cls=5):
  gen = torch.Generator().manual_seed(seed)
  protos = NC.unit(torch.randn(m, d, generator=gen, dtype=torch.float64))
  own = torch.randint(0, m, (p,), generator=gen)
  emb = NC.unit(protos[own] + 0.8 * torch.randn(p, d, generator=gen, dtype=torch.float64))
  p_sem = torch.randint(0, n_cls, (m,), generator=gen)
  sem = p_sem[own].clone()
  flip = torch.rand(p, generator=gen) < 0.3
  sem[flip] = torch.randint(0, n_cls, (int(flip.sum()),), generator=gen)
  wgt = torch.rand(p, generator=gen, dtype=torch.float64)
  return emb, own, sem, protos, p_sem, wgt


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_reference_equals_the_oracle_in_fp64(mode):
  """Same inputs, fp64 on both sides: O.segsort_nll, O.set_segsort_nll, and _plain_nll of the batched tests."""
  emb, own, sem, protos, p_sem, wgt = _random_problem(211, 37, 19, 5 + mode)
  gen = torch.Generator().manual_seed(99)
  p_tags = O.one_hot(p_sem, 5) | (O.one_hot(torch.randint(0, 5, (37,), generator=gen), 5) *
                                  (torch.rand(37, generator=gen) < 0.3).view(-1, 1).long())
  tags = O.one_hot(sem, 5)
  e = emb.clone().requires_grad_(True)
  pr = protos.clone().requires_grad_(True)
  if mode == 2:
    want = _plain_nll(e, sem, own, pr, p_sem, 12.0)
  elif mode == 1:
    want = O.set_segsort_nll(e, tags, own, pr, p_tags, 12.0)
  else:
    want = O.segsort_nll(e, sem, own, pr, p_sem, 12.0)
  (want.view(-1) * wgt).sum().backward()
  codes = (_tags_to_mask(tags), _tags_to_mask(p_tags)) if mode == 1 else (sem, p_sem)
  r = R.evaluate(emb, own, codes[0], protos, codes[1], 12.0, mode, wgt)
  assert r.nll.dtype == torch.float64
  torch.testing.assert_close(r.nll, want.detach().view(-1), rtol=1e-13, atol=1e-13)
  torch.testing.assert_close(r.d_emb, e.grad, rtol=1e-11, atol=1e-13)
  torch.testing.assert_close(r.d_protos, pr.grad, rtol=1e-11, atol=1e-13)
  fb = r.stats[:, 3] != 0
  assert fb.all() if mode == 2 else (0 < int(fb.sum()) < 211)      # both branches of the fallback are in the comparison
  assert torch.equal(fb, torch.ones_like(fb) if mode == 2 else ~(r.pos > 0))


@pytest.mark.parametrize('tag', ['tiny', 'small', 'loc'])
def test_reference_reproduces_the_committed_goldens(tag):
  """a09_loss_*: fp32 outputs of the original formula.  The reference evaluated in fp32 must agree to fp32 rounding,
  and its fp64 evaluation to the golden's own precision on the mean loss."""
  g = load_golden('a09_loss_' + tag)
  p = g.emb.shape[0]
  d_nll = torch.full((p,), 1.0 / p)
  for mode, px, prc, nll, loss, de, dp in (
      (0, g.sem, g.p_sem, g.nll, g.loss, g.d_emb, g.d_protos),
      (1, _tags_to_mask(g.tags), _tags_to_mask(g.p_tags), g.set_nll, g.set_loss, g.set_d_emb, g.set_d_protos)):
    r32 = R.evaluate(g.emb, g.own, px, g.protos, prc, g.kappa, mode, d_nll, dtype=torch.float32)
    torch.testing.assert_close(r32.nll, nll.view(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r32.d_emb, de, rtol=1e-4, atol=1e-7 * de.abs().max().item() + 1e-12)
    torch.testing.assert_close(r32.d_protos, dp, rtol=1e-4, atol=1e-7 * dp.abs().max().item() + 1e-12)
    r64 = R.evaluate(g.emb, g.own, px, g.protos, prc, g.kappa, mode, d_nll)
    assert abs(r64.nll.mean().item() - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    scale = r64.d_emb.abs().max().item()
    assert (r64.d_emb - de.double()).abs().mean().item() <= 1e-5 * scale


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_reference_gradients_equal_finite_differences(mode):
  """Five pixels, seven prototypes, D = 3, all four pixel kinds (asserted): central differences in fp64."""
  case = NC.C('fd', 5, 7, 3, 4.0, mode, '', '')
  gen = torch.Generator().manual_seed(3)
  protos = NC.unit(torch.randn(7, 3, generator=gen, dtype=torch.float64))
  pr_code = torch.tensor([0, 0, 0, 1, 1, 1, 2])
  own = torch.tensor([0, 6, 3, 4, 1])
  px_cls = torch.tensor([0, 2, 0, 0, 1])             # kinds a, b, c, d and one more (asserted below)
  emb = NC.unit(protos[own] + 0.7 * torch.randn(5, 3, generator=gen, dtype=torch.float64))
  if mode & 1:
    px_code, pr_code = 1 << px_cls, (1 << pr_code) | torch.tensor([0, 2, 0, 0, 0, 0, 0])
  else:
    px_code = px_cls
  wgt = torch.tensor([1.0, 0.3, 2.0, 0.01, 0.5], dtype=torch.float64)
  r = R.evaluate(emb, own, px_code, protos, pr_code, case.kappa, mode, wgt)
  kinds = NC.kinds_of(R.evaluate(emb, own, px_code, protos, pr_code, case.kappa, mode & ~R.PLAIN))
  assert set(kinds) == set('abcd'), kinds

  def loss(e, pr):
    return float((R.forward(e, own, px_code, pr, pr_code, case.kappa, mode)[0] * wgt).sum())
  h = 1e-6
  for x, grad, f in ((emb, r.d_emb, lambda v: loss(v, protos)), (protos, r.d_protos, lambda v: loss(emb, v))):
    for i in range(x.shape[0]):
      for j in range(x.shape[1]):
        hi, lo = x.clone(), x.clone()
        hi[i, j] += h
        lo[i, j] -= h
        fd = (f(hi) - f(lo)) / (2 * h)
        assert abs(fd - grad[i, j].item()) <= 1e-6 * max(1.0, grad.abs().max().item()), (i, j, fd, grad[i, j].item())


def test_d_protos_rows_rule():
  dp = torch.ones(70, 3)
  assert R.d_protos_rows(dp, -1)[:2] == (70, 70) and R.d_protos_rows(dp, 75)[:2] == (70, 70)
  assert R.d_protos_rows(dp, 33)[:2] == (33, 64) and R.d_protos_rows(dp, 32)[:2] == (32, 32)
  assert R.d_protos_rows(dp, 0)[:2] == (0, 0) and R.d_protos_rows(dp, 65)[:2] == (65, 70)


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize('case', NC.CASES, ids=[c.name for c in NC.CASES])
def test_case_inputs_keep_the_margin_and_the_kinds(case):
  """No pixel of any case may need an exclusion: on the fp64 reference pos == 0 exactly or |pos| >= own / 16, every
  pixel is of the kind it was drawn for, and each kind has at least four pixels."""
  q = NC.build(case)
  assert q.emb.shape == (case.p, case.d) and q.protos.shape == (case.m, case.d)
  assert bool(NC.margin_ok(q.seg).all())
  assert NC.kinds_of(q.seg) == q.want_kinds
  assert torch.isfinite(q.ref.nll).all() and torch.isfinite(q.ref.d_emb).all() and torch.isfinite(q.ref.d_protos).all()
  count = collections.Counter(q.want_kinds)
  if q.full:
    assert all(count[k] >= 4 for k in 'abcd'), count
    b = torch.tensor([k == 'b' for k in q.want_kinds])
    assert bool((q.seg.pos[b] == 0).all())                                  # exactly: one positive, itself
  else:
    assert case.p < 31 or case.m < 31
  if case.mode & R.PLAIN:
    assert bool((q.ref.stats[:, 3] == 1).all())
  if case.mode & R.CODE32:
    assert int(q.px_code.max()) < 2 ** 31 and int(q.pr_code.max()) < 2 ** 31
  if case.bit40:
    assert int(q.px_code.max()) >= 2 ** 40 and int(q.pr_code.max()) >= 2 ** 40
  uni, straddle = NC.tile_kinds(q.pr_code, case.m)
  if case.runs:                          # the one-predicate epilogue of nll_fwd2 AND the general one, >= 3 tiles
    assert case.mode & R.CODE32 and case.d <= 80 and uni >= 2 and straddle >= 1 and case.m % 32 != 0, (uni, straddle)
  else:
    assert uni == 0 or case.m < 64
  if case.mode & R.TAGSET and case.m >= 31:
    two = (q.pr_code & (q.pr_code - 1)) != 0
    assert 0.1 * case.m < int(two.sum()) < 0.5 * case.m                     # a second bit on about 30 %
  w = q.d_nll[q.d_nll > 0]
  assert case.p < 31 or w.max() / w.min() > 100.0
  assert int((q.d_nll == 0).sum()) == (32 if case.zero_block else 0) and (not case.zero_block or case.p >= 64)


@pytest.mark.parametrize('case', NC.CASES, ids=[c.name for c in NC.CASES])
def test_case_names_its_route(case):
  assert NC.path_names(case) == (case.fwd, case.bwd)


def test_m_grad_calls_name_their_route():
  for name, m_grad, bwd in NC.MGRAD:
    assert NC.path_names(NC.BY_NAME[name], m_grad)[1] == bwd, (name, m_grad)
  for name in {n for n, _, _ in NC.MGRAD}:
    m = NC.BY_NAME[name].m
    assert sorted(g for n, g, _ in NC.MGRAD if n == name) == sorted({0, 1, 31, 32, 33, m - 1, m, m + 5})


def test_three_strips_start_at_513_pixels():
  """SPML_NLL_TCACHE_MB=1 with 18 prototype tiles: strips of 8 pixel tiles, so 512 pixels are two strips."""
  case = NC.BY_NAME['wide_d528_3strips']
  assert 'strips=3' in NC.path_names(case)[1]
  assert 'strips=2' in NC.path_names(case._replace(p=512))[1]
  assert 'strips=1' in NC.path_names(case._replace(env=()))[1]


def test_route_query_refuses_what_the_calls_refuse():
  from spml_amd import _ffi
  assert _ffi.segsort_nll_path_name(10, 10, 529, 0) == 'unsupported'
  assert _ffi.segsort_nll_path_name(10, 0, 64, 0) == 'unsupported'
  assert _ffi.segsort_nll_path_name(10, 10, 64, 8) == 'unsupported'
  assert _ffi.segsort_nll_path_name(10, 10, 528, 0) == 'fwd<33,1,label,c64>'
  # no pixels: the calls return before their first launch (every width and direction; 272 < D has no strip to count)
  for d in (2, 64, 80, 144, 273, 528):
    for backward in (False, True):
      assert _ffi.segsort_nll_path_name(0, 10, d, 5, backward) == 'nothing'
  assert _ffi.segsort_nll_path_name(0, 10, 529, 0) == 'unsupported'


def test_every_route_of_the_dispatch_is_in_the_table():
  """Each kernel family and each launch shape the host dispatch can choose appears in an asserted path name."""
  fwd = {c.fwd.split(' ')[0] for c in NC.CASES}
  for ks, mtb in ((2, 4), (3, 4), (4, 4), (5, 2)):
    for t in ('label', 'tag'):
      assert 'fwd2<%d,%d,%s>' % (ks, mtb, t) in fwd and 'fwd2_plain<%d,%d,%s>' % (ks, mtb, t) in fwd
  for ks in (2, 3, 4, 5, 9, 17, 33):
    for t in ('label', 'tag'):
      assert 'fwd<%d,1,%s,c64>' % (ks, t) in fwd
      assert ks <= 5 or 'fwd<%d,1,%s,c32>' % (ks, t) in fwd
  assert {c.fwd.split('chunks=')[1] for c in NC.CASES if 'chunks=' in c.fwd} == {'1', '2', '9'}
  bwd = ' | '.join([c.bwd for c in NC.CASES] + [b for _, _, b in NC.MGRAD])
  for t in ('label', 'tag'):
    for piece in ['de3<%s> rows=1 + dp3<%s>', 'de3<%s> rows=1 + dp<4,2,%s>',
                  'de2<4,2,%s> rows=1 + dp<4,2,%s>', 'de2<2,1,%s> rows=1 + dp<2,1,%s>',
                  'de2<3,2,%s> rows=1 + dp<3,2,%s>', 'de<2,1,%s> + dp<2,1,%s>', 'de<3,2,%s> + dp<3,2,%s>',
                  'de<4,2,%s> + dp<4,2,%s>', 'de<5,3,%s> + dp<5,3,%s>', 'de<9,5,%s> + dp<9,5,%s>',
                  'de<17,9,%s> + dp<17,9,%s>']:
      assert piece % (t, t) in bwd, piece % (t, t)
    for piece in ['wide<%s> strips=1 launches=1+1', 'wide<%s> strips=1 launches=1+2', 'wide<%s> strips=3 launches=1+2']:
      assert piece % t in bwd, piece % t
  runs = [c for c in NC.CASES if c.runs]
  assert {(c.mode & 3) for c in runs} == {0, 1, 2, 3} and {c.m for c in runs} >= {130, 161, 3100}
  for piece in ['rows=2 + dp3', 'rows=2 + dp<3,2', 'rows=8 + dp3', 'rows=8 + dp<3,2', 'de2<4,2,tag> rows=2', 'strips=3 launches=1+1', 'no dp', 'fix64',
                'dp3<tag> mt=5 fix64', 'launches=1+2 mt=5 fix64', 'dp<5,3,tag> chunks=2 mt=5 fix64']:
    assert piece in bwd, piece
