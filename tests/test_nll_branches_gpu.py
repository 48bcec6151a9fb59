"""Every launch branch of the pixel-to-segment NLL (csrc/nll.hip, nll_de3.hip, nll_dp3.hip) against a plain fp64
evaluation of the header's formula (tests/nll_ref.py), case by case of ONE table (tests/nll_cases.py: the comment
beside a case names the template instances it reaches; the `uni_*` cases have prototypes in runs of one code, for
the one-predicate epilogue that nll_fwd2 / nll_fwd2_plain take on tiles of a single code).  Every case first asserts the library's own route query
(spml_segsort_nll_path_name), so that a moved threshold cannot take a case onto another kernel unnoticed.

No pixel is left out of any comparison: the inputs are drawn so that the reference itself is well-conditioned
(tests/test_nll_ref.py asserts the margin for every pixel on the CPU).  Bounds (profiles/nll_branch_parity.md has the
measured figures):
  nll       |got - ref| / max(|ref|, 1) <= 2e-5 for every pixel
  gradients every element within 1e-4 of the reference gradient's largest magnitude, the mean error within 2e-6 of it
            (the fp64 bounds of test_nll_at_the_eight_gpu_prototype_count_against_the_oracle, without its exclusion).
            With a single prototype nll = 0 for every input and the gradient vanishes identically,
            kappa g_p (s/den - s/num) pr = kappa g_p (1 - 1) pr: the scale is then kappa * max(d_nll), the size of the
            two terms that cancel
  stats     the fallback flag equals the reference's decision exactly; num, den, own_sim: relative error at most
            max(4 x the error of torch's fp32 evaluation of the same formula on the same inputs, STATS_FLOOR)
"""
import pytest
import torch

import nll_cases as NC
import nll_ref as R
from spml_amd import _ffi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# Largest relative error of num / den / own_sim of torch's own fp32 evaluation (nll_ref.evaluate with dtype float32, CPU)
# over all cases of the table, measured once: 7.2e-6 (own_sim at D = 321, three strips), rounded up.  Not a kernel figure.
STATS_FLOOR = 8e-6
NLL_BOUND, GRAD_MAX, GRAD_MEAN = 2e-5, 1e-4, 2e-6


def _dev(q):
  return [t.to(DEV).contiguous() for t in (q.emb, q.own, q.px_code, q.protos, q.pr_code, q.d_nll)]


def _backward(emb, own, px_code, protos, pr_code, kappa, mode, stats, d_nll, m_grad, d_protos):
  """spml_segsort_nll_bwd_f32 adding into the d_protos given (spml_amd._ffi.segsort_nll_bwd always starts from zeros)."""
  p, d = emb.shape
  m = protos.shape[0]
  d_emb = torch.empty_like(emb)
  ws = _ffi.workspace(_ffi.lib().spml_segsort_nll_workspace_bytes(p, m, d), emb.device)
  _ffi.check(_ffi.lib().spml_segsort_nll_bwd_f32(
      _ffi.ptr(emb, torch.float32), _ffi.ptr(own, torch.int64), _ffi.ptr(px_code, torch.int64), p,
      _ffi.ptr(protos, torch.float32), _ffi.ptr(pr_code, torch.int64), m, d, float(kappa), int(mode),
      _ffi.ptr(stats, torch.float32), _ffi.ptr(d_nll, torch.float32), _ffi.ptr(d_emb), _ffi.ptr(d_protos),
      int(m_grad), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr()), 'spml_segsort_nll_bwd_f32')
  return d_emb


def run(case, q, m_grad=None, init=None):
  """One forward + backward call of a case under its switches -> nll, stats, d_emb, d_protos (CPU); the route is
  asserted first."""
  m_grad = case.m_grad if m_grad is None else m_grad
  emb, own, px_code, protos, pr_code, d_nll = _dev(q)
  with NC.applied(case):
    nll, stats = _ffi.segsort_nll_fwd(emb, own, px_code, protos, pr_code, case.kappa, case.mode)
    dp = torch.zeros_like(protos) if init is None else init.to(DEV).clone()
    de = _backward(emb, own, px_code, protos, pr_code, case.kappa, case.mode, stats, d_nll, m_grad, dp)
    torch.cuda.synchronize()
  return nll.cpu(), stats.cpu(), de.cpu(), dp.cpu()


def grad_scale(case, q, ref_grad):
  if case.m == 1:                      # the gradient vanishes identically: the size of the two terms that cancel
    return case.kappa * q.d_nll.max().item()
  return ref_grad.abs().max().item()


def figures_forward(q, nll, stats):
  ref, r32 = q.ref, q.ref32
  f = {'nll': ((nll.double() - ref.nll).abs() / ref.nll.abs().clamp(min=1.0)).max().item(),
       'nll32': ((r32.nll.double() - ref.nll).abs() / ref.nll.abs().clamp(min=1.0)).max().item()}
  for j, name in enumerate(('num', 'den', 'own')):
    f[name] = ((stats[:, j].double() - ref.stats[:, j]).abs() / ref.stats[:, j].abs()).max().item()
    f[name + '32'] = ((r32.stats[:, j].double() - ref.stats[:, j]).abs() / ref.stats[:, j].abs()).max().item()
  f['flags_off'] = int((stats[:, 3].double() != ref.stats[:, 3]).sum())
  return f


def figures_grad(case, q, got, want, want32, name):
  scale = grad_scale(case, q, want)
  err = (got.double() - want).abs()
  return {name + '_max': err.max().item() / scale, name + '_mean': err.mean().item() / scale,
          name + '32_max': (want32.double() - want).abs().max().item() / scale}


def report(case, what, f):
  print('NLLFIG %s %s %s' % (case.name, what, ' '.join('%s=%.3g' % kv for kv in sorted(f.items()))))


def assert_forward(case, f):
  assert f['flags_off'] == 0, (case.name, f)
  assert f['nll'] <= NLL_BOUND, (case.name, f)
  for name in ('num', 'den', 'own'):
    assert f[name] <= max(4.0 * f[name + '32'], STATS_FLOOR), (case.name, name, f)


def assert_grad(case, f, name):
  assert f[name + '_max'] <= GRAD_MAX and f[name + '_mean'] <= GRAD_MEAN, (case.name, name, f)


def add_rounding(case, init, want):
  """What adding into a buffer that is not zero may cost on top of the gradient's own error: a prototype element
  receives at most one fp32 atomic add per pixel tile (one in all in deterministic mode), each rounded to half an ulp
  of the running sum, which |init| + |gradient| bounds."""
  return (case.p + 31) // 32 * 2.0 ** -24 * (init.abs().double() + want.abs())


def assert_d_protos_rows(case, q, dp, m_grad, init=None):
  """Rows below m_grad match the reference, rows from ceil32(m_grad) on are exactly what they were, rows in between
  are either untouched or the reference's (include/spml_hip.h)."""
  lo, hi, want = R.d_protos_rows(q.ref.d_protos, m_grad)
  before = torch.zeros_like(dp) if init is None else init
  assert torch.equal(dp[hi:], before[hi:]), (case.name, m_grad, 'rows past the last tile were written')
  scale = grad_scale(case, q, q.ref.d_protos)
  err = (dp.double() - before.double() - want).abs()
  if lo:
    assert err[:lo].max().item() <= GRAD_MAX * scale and err[:lo].mean().item() <= GRAD_MEAN * scale, (case.name, m_grad)
  for r in range(lo, hi):
    assert torch.equal(dp[r], before[r]) or err[r].max().item() <= GRAD_MAX * scale, (case.name, m_grad, r)


@pytest.mark.parametrize('case', NC.CASES, ids=[c.name for c in NC.CASES])
def test_branch_against_the_fp64_reference(case):
  assert NC.path_names(case) == (case.fwd, case.bwd)
  q = NC.build(case)
  init = None
  if case.dp_init:                     # d_protos is ADDED into: start from a buffer that is not zero
    init = torch.randn(case.m, case.d, generator=torch.Generator().manual_seed(5)) * q.ref.d_protos.abs().max().item()
  nll, stats, de, dp = run(case, q, init=init)
  again = run(case, q, init=init)
  f = figures_forward(q, nll, stats)
  report(case, 'forward ' + case.fwd.replace(' ', '_'), f)
  g = figures_grad(case, q, de, q.ref.d_emb, q.ref32.d_emb, 'de')
  base = dp if init is None else (dp.double() - init.double())
  g.update(figures_grad(case, q, base, q.ref.d_protos, q.ref32.d_protos, 'dp'))
  g['dp_run_to_run'] = (dp - again[3]).abs().max().item() / grad_scale(case, q, q.ref.d_protos)
  report(case, 'backward ' + case.bwd.replace(' ', '_'), g)
  # run-to-run: nll, stats and d_emb bit-identical on every route; d_protos in deterministic mode
  assert torch.equal(nll, again[0]) and torch.equal(stats, again[1]) and torch.equal(de, again[2]), case.name
  if case.det:
    assert torch.equal(dp, again[3]), case.name
  assert_forward(case, f)
  assert_grad(case, g, 'de')
  if init is None:
    assert_grad(case, g, 'dp')
  else:
    scale = grad_scale(case, q, q.ref.d_protos)
    err = ((dp.double() - init.double() - q.ref.d_protos).abs() - add_rounding(case, init, q.ref.d_protos)).clamp(min=0)
    assert err.max().item() <= GRAD_MAX * scale and err.mean().item() <= GRAD_MEAN * scale, (case.name, g)


@pytest.mark.parametrize('name', sorted({n for n, _, _ in NC.MGRAD}))
def test_m_grad_takes_whole_tiles_and_nothing_past_them(name):
  case = NC.BY_NAME[name]
  q = NC.build(case)
  for n, m_grad, bwd in NC.MGRAD:
    if n != name:
      continue
    assert NC.path_names(case, m_grad)[1] == bwd
    nll, stats, de, dp = run(case, q, m_grad=m_grad)
    assert_d_protos_rows(case, q, dp, m_grad)
    g = figures_grad(case, q, de, q.ref.d_emb, q.ref32.d_emb, 'de')      # d_emb does not depend on m_grad
    assert_grad(case, g, 'de')


def test_m_grad_adds_into_a_buffer_that_is_not_zero():
  case = NC.BY_NAME['c32_d64_l']
  q = NC.build(case)
  scale = q.ref.d_protos.abs().max().item()
  init = torch.randn(case.m, case.d, generator=torch.Generator().manual_seed(6)) * scale
  _, _, _, dp = run(case, q, m_grad=33, init=init)
  lo, hi, want = R.d_protos_rows(q.ref.d_protos, 33)
  assert (lo, hi) == (33, 64) and torch.equal(dp[hi:], init[hi:])
  err = (dp.double() - init.double() - want).abs() - add_rounding(case, init, want)
  assert err[:lo].max().item() <= GRAD_MAX * scale


@pytest.mark.parametrize('name', ['c32_d17', 'c32_d48', 'c32_d64_l', 'c32_d65', 'c32_d64', 'uni_d64_l', 'uni_d80_tp'])
def test_fwd2_pixel_does_not_depend_on_the_other_pixels_of_the_call(name):
  """csrc/nll.hip, nll_fwd2: "a pixel's result does not depend on which other pixels are in the call" -- the first 70
  rows of a 257-pixel call are bit-identical to a 70-pixel call (two pixel tiles and a ragged third instead of nine)."""
  case = NC.BY_NAME[name]
  assert case.p == 257 and case.fwd.startswith(('fwd2<', 'fwd2_plain<'))
  q = NC.build(case)
  emb, own, px_code, protos, pr_code, _ = _dev(q)
  with NC.applied(case):
    assert NC.path_names(case)[0] == case.fwd
    nll, stats = _ffi.segsort_nll_fwd(emb, own, px_code, protos, pr_code, case.kappa, case.mode)
    assert _ffi.segsort_nll_path_name(70, case.m, case.d, case.mode) == case.fwd
    nll70, stats70 = _ffi.segsort_nll_fwd(emb[:70].contiguous(), own[:70].contiguous(), px_code[:70].contiguous(),
                                          protos, pr_code, case.kappa, case.mode)
    torch.cuda.synchronize()
  assert torch.equal(nll[:70], nll70) and torch.equal(stats[:70], stats70)


def test_batched_entry_points_in_mode_tagset_plain_code32():
  """The mode tests/test_nll_batched_gpu.py lacks, 1 | 2 | 4, under the same reference and bounds: three problems of
  the table's recipe in one call."""
  mode, d, kappa = R.TAGSET | R.PLAIN | R.CODE32, 66, 12.0
  assert _ffi.segsort_nll_batched_supported(d, mode)
  # the third problem's prototypes come in runs of 48 of one code: nll_fwd2_plain_batched's one-predicate epilogue
  cases = [NC.C('batched_%d' % i, p, m, d, kappa, mode, '', '', runs=r)
           for i, (p, m, r) in enumerate(((70, 33, 0), (31, 97, 0), (257, 130, 48)))]
  qs = [NC.build(c) for c in cases]
  assert NC.tile_kinds(qs[2].pr_code, 130)[0] >= 2
  first, own_abs = 0, []
  for q in qs:
    assert bool(NC.margin_ok(q.seg).all()) and NC.kinds_of(q.seg) == q.want_kinds
    own_abs.append(q.own + first)
    first += q.case.m
  cat = lambda name: torch.cat([getattr(q, name) for q in qs]).to(DEV).contiguous()
  ps, ms = [c.p for c in cases], [c.m for c in cases]
  args = (cat('emb'), torch.cat(own_abs).to(DEV), cat('px_code'), ps, cat('protos'), cat('pr_code'), ms, kappa, mode)
  nll, stats = _ffi.segsort_nll_batched_fwd(*args)
  de, dp = _ffi.segsort_nll_batched_bwd(*args, stats, cat('d_nll'))
  torch.cuda.synchronize()
  nll, stats, de, dp = nll.cpu(), stats.cpu(), de.cpu(), dp.cpu()
  lo = mlo = 0
  for case, q in zip(cases, qs):
    f = figures_forward(q, nll[lo:lo + case.p], stats[lo:lo + case.p])
    g = figures_grad(case, q, de[lo:lo + case.p], q.ref.d_emb, q.ref32.d_emb, 'de')
    g.update(figures_grad(case, q, dp[mlo:mlo + case.m], q.ref.d_protos, q.ref32.d_protos, 'dp'))
    report(case, 'batched', dict(f, **g))
    assert_forward(case, f)
    assert_grad(case, g, 'de')
    assert_grad(case, g, 'dp')
    lo, mlo = lo + case.p, mlo + case.m
