"""Inputs of tests/test_nll_branches_gpu.py: one table of cases, and for each case inputs on which the fp64 reference
(tests/nll_ref.py) itself is well-conditioned, so that NO pixel is left out of any comparison.  CPU only.

Recipe: classes round-robin over the prototypes (every class has several), class centres random unit vectors,
protos = unit(centre[class] + unit(noise)), emb = unit(protos[own] + 1.5 unit(noise)).  Four prototypes at the end
have a class of their own each.  Pixel kinds (at least 4 of each in every case with P >= 31 and M >= 31):
  a  own prototype of the pixel's class, other positives present          no fallback, own in the positive set
  b  own prototype the only one of its class: pos is exactly 0 in every precision         fallback, own in the set
  c  code switched to another class, emb and own kept                     fallback, own outside the positive set
  d  own moved to a prototype of another class, emb and code kept         no fallback, own outside: weight 1 / num
Margin, asserted on the fp64 reference for every pixel: pos == 0 exactly or |pos| >= own_sim / 16.  A pixel that
misses its kind or the margin is drawn again with a fresh seed (rejection on the reference alone, before any kernel
runs); P stays what the case says and nothing is masked.
"""
import collections
import functools

import torch

import nll_ref as R

MARGIN = 1.0 / 16.0
MAX_DRAWS = 400

Case = collections.namedtuple(
    'Case', 'name p m d kappa mode fwd bwd m_grad env det bit40 zero_block dp_init runs')


def C(name, p, m, d, kappa, mode, fwd, bwd, m_grad=-1, env=None, det=False, bit40=False, zero_block=False,
      dp_init=False, runs=0):
  return Case(name, p, m, d, kappa, mode, fwd, bwd, m_grad, tuple(sorted((env or {}).items())), det, bit40,
              zero_block, dp_init, runs)


def unit(x):
  return x / x.norm(dim=-1, keepdim=True)


class Inputs:
  pass


def _classes(m, runs=0):
  """(class of every prototype, number of round-robin classes, number of single-prototype classes).  runs > 0: the
  classes change every `runs` prototypes (image-major prototypes: whole 32-prototype tiles of one code)."""
  n_single = 4 if m >= 12 else (1 if m < 2 else 0)
  n_cls = max(1, min(7, (m - n_single) // 3)) if m > n_single else 0
  cls = torch.empty(m, dtype=torch.long)
  if n_cls and runs:
    n_cls = min(7, (m - n_single + runs - 1) // runs)
    cls[:m - n_single] = (torch.arange(m - n_single) // runs) % n_cls
  elif n_cls:
    cls[:m - n_single] = torch.arange(m - n_single) % n_cls
  cls[m - n_single:] = n_cls + torch.arange(n_single)
  return cls, n_cls, n_single


def _draw_pixel(kind, cls, n_cls, n_single, protos, gen):
  """One pixel of a kind: (emb row, own, class the pixel's code names)."""
  m, d = protos.shape
  if kind == 'b':
    near = m - n_single + int(torch.randint(0, n_single, (1,), generator=gen))
  else:
    near = int(torch.randint(0, m - n_single, (1,), generator=gen))
  e = unit(protos[near] + 1.5 * unit(torch.randn(d, generator=gen, dtype=torch.float64)))
  own, c = near, int(cls[near])
  if kind == 'c':                        # the code names another round-robin class
    c = (c + 1 + int(torch.randint(0, n_cls - 1, (1,), generator=gen))) % n_cls
  if kind == 'd':                        # own: a prototype of another round-robin class
    other = (cls != c) & (cls < n_cls)
    idx = other.nonzero().view(-1)
    own = int(idx[int(torch.randint(0, idx.numel(), (1,), generator=gen))])
  return e, own, c


def _codes(case, cls, n_cls, px_cls, gen):
  """px_code [P], pr_code [M]: labels, or tag sets (the class bit, + a second round-robin class bit on ~30 % of the
  prototypes).  bit40: class 0 lives at bit 40 / label 2^40 (the 64-bit predicate)."""
  m = cls.numel()
  if case.mode & R.TAGSET:
    bit = lambda c: torch.where(c == 0, torch.full_like(c, 40), c) if case.bit40 else c
    pr = torch.ones(m, dtype=torch.long) << bit(cls)
    if n_cls > 1 and case.runs:        # a second bit on every third run: the tiles inside a run stay uniform
      rid = torch.arange(m) // case.runs
      extra, has = (cls + 1) % n_cls, (rid % 3 == 1) & (cls < n_cls)
      pr = torch.where(has, pr | (torch.ones(m, dtype=torch.long) << bit(extra)), pr)
    elif n_cls > 1:
      extra = torch.randint(0, n_cls, (m,), generator=gen)
      has = torch.rand(m, generator=gen) < 0.3
      pr = torch.where(has, pr | (torch.ones(m, dtype=torch.long) << bit(extra)), pr)
    return torch.ones_like(px_cls) << bit(px_cls), pr
  if case.bit40:
    f = lambda c: torch.where(c == 0, torch.full_like(c, 1 << 40), c)
    return f(px_cls), f(cls)
  return px_cls.clone(), cls.clone()


def kinds_of(ref_seg):
  """Kind letter of every pixel, from the reference evaluated WITHOUT the PLAIN flag."""
  fb = ref_seg.stats[:, 3] != 0
  out = []
  for f, s in zip(fb.tolist(), ref_seg.own_same.tolist()):
    out.append('b' if f and s else 'c' if f else 'a' if s else 'd')
  return out


def margin_ok(ref_seg):
  own = ref_seg.stats[:, 2]
  return (ref_seg.pos == 0) | (ref_seg.pos.abs() >= own * MARGIN)


@functools.lru_cache(maxsize=None)
def build(case):
  """Inputs (fp32 / int64 CPU tensors) + the fp64 reference of a case; computed once, shared, never modified."""
  gen = torch.Generator().manual_seed(20240 + sum(map(ord, case.name)))
  p, m, d = case.p, case.m, case.d
  cls, n_cls, n_single = _classes(m, case.runs)
  centres = unit(torch.randn(max(1, n_cls + n_single), d, generator=gen, dtype=torch.float64))
  protos = unit(centres[cls] + unit(torch.randn(m, d, generator=gen, dtype=torch.float64))).float()
  # the kinds this (P, M) can hold; spread over the tiles by a permutation
  want = ['a'] * p
  full = p >= 31 and m >= 31
  if n_cls == 0:
    want = ['b'] * p
  elif full:
    perm = torch.randperm(p, generator=gen).tolist()
    n_each = 4 + p // 16
    for j, kind in enumerate('bcd'):
      for i in perm[j * n_each:(j + 1) * n_each]:
        want[i] = kind
  emb = torch.empty(p, d, dtype=torch.float32)
  own = torch.empty(p, dtype=torch.long)
  px_cls = torch.empty(p, dtype=torch.long)
  todo, draws = list(range(p)), 0
  seg_mode = case.mode & ~R.PLAIN
  while todo:
    draws += 1
    assert draws <= MAX_DRAWS, 'case %s: %d pixels still miss their kind or the margin' % (case.name, len(todo))
    for i in todo:
      e, o, c = _draw_pixel(want[i], cls, n_cls, n_single, protos.double(), gen)
      emb[i], own[i], px_cls[i] = e.float(), o, c
    cgen = torch.Generator().manual_seed(77 + sum(map(ord, case.name)))      # the same codes in every round
    px_code, pr_code = _codes(case, cls, n_cls, px_cls, cgen)
    seg = R.evaluate(emb, own, px_code, protos, pr_code, case.kappa, seg_mode)
    ok = margin_ok(seg) & torch.isfinite(seg.nll)
    got = kinds_of(seg)
    todo = [i for i in range(p) if not ok[i] or got[i] != want[i]]
  # upstream gradient: non-uniform over three decades; optionally a block of exactly zero weights
  d_nll = (10.0 ** (-3.0 * torch.rand(p, generator=gen)) / max(p, 1)).float()
  if case.zero_block:
    d_nll[32:64] = 0.0
  q = Inputs()
  q.case, q.emb, q.own, q.px_code, q.protos, q.pr_code, q.d_nll = case, emb, own, px_code, protos, pr_code, d_nll
  q.want_kinds, q.draws, q.full = want, draws, full
  q.seg = seg                                                               # reference without PLAIN: kinds, margin
  q.ref = R.evaluate(emb, own, px_code, protos, pr_code, case.kappa, case.mode & 3, d_nll)
  q.ref32 = R.evaluate(emb, own, px_code, protos, pr_code, case.kappa, case.mode & 3, d_nll, dtype=torch.float32)
  return q


L, T, PL, C32 = 0, R.TAGSET, R.PLAIN, R.CODE32
DE3_OFF, DP3_OFF = {'SPML_NLL_DE3': '0'}, {'SPML_NLL_DP3': '0'}
STRIPS3 = {'SPML_NLL_TCACHE_MB': '1'}

# name, P, M, D, kappa, mode, forward path, backward path [, options].  The paths are what
# spml_segsort_nll_path_name must answer; the comment names the kernel instances the case reaches.
CASES = [
    # ---- narrow embeddings, 32-bit codes: nll_fwd2<KS,4|2,TAG> (PLAIN: nll_fwd2_plain); nll_bwd_de2<2|3,..> +
    #      nll_bwd_dp, or the pipelined nll_bwd_de3<4,2,TAG> + nll_bwd_dp3<4,2,TAG>; above 64 channels the round-2 pair
    C('c32_d2', 33, 31, 2, 6.0, L | C32, 'fwd2<2,4,label> chunks=1',
      'de2<2,1,label> rows=1 + dp<2,1,label> chunks=1 mt=1'),      # one pixel tile + 1 row, one prototype tile
    C('c32_d17', 257, 130, 17, 12.0, T | C32, 'fwd2<2,4,tag> chunks=1',
      'de2<2,1,tag> rows=1 + dp<2,1,tag> chunks=2 mt=5'),      # KS 2, odd width; two workgroups, ragged last tile
    C('c32_d32', 70, 97, 32, 12.0, L | PL | C32, 'fwd2_plain<2,4,label> chunks=1',
      'de2<2,1,label> rows=1 + dp<2,1,label> chunks=1 mt=4'),      # KS 2 upper edge, PLAIN: all fallback on de2
    C('c32_d33', 129, 33, 33, 12.0, T | PL | C32, 'fwd2_plain<3,4,tag> chunks=1',
      'de2<3,2,tag> rows=1 + dp<3,2,tag> chunks=1 mt=2'),      # KS 3 lower edge, M one past a tile
    C('c32_d48', 257, 130, 48, 16.0, L | C32, 'fwd2<3,4,label> chunks=1',
      'de2<3,2,label> rows=1 + dp<3,2,label> chunks=2 mt=5', zero_block=True),      # KS 3 upper edge
    C('c32_d49', 257, 130, 49, 12.0, T | C32, 'fwd2<4,4,tag> chunks=1',
      'de3<tag> rows=1 + dp3<tag> mt=5'),      # KS 4 lower edge: pipelined pair, 15 padded channels
    C('c32_d50', 70, 97, 50, 12.0, L | C32, 'fwd2<4,4,label> chunks=1',
      'de3<label> rows=1 + dp3<label> mt=4'),      # KS 4, even width
    C('c32_d63', 129, 33, 63, 12.0, L | PL | C32, 'fwd2_plain<4,4,label> chunks=1',
      'de3<label> rows=1 + dp3<label> mt=2'),      # KS 4, PLAIN: every pixel a fallback on de3 / dp3
    C('c32_d64', 257, 130, 64, 16.0, T | PL | C32, 'fwd2_plain<4,4,tag> chunks=1',
      'de3<tag> rows=1 + dp3<tag> mt=5', dp_init=True),      # KS 4 upper edge, tag sets + PLAIN
    C('c32_d64_l', 257, 130, 64, 12.0, L | C32, 'fwd2<4,4,label> chunks=1',
      'de3<label> rows=1 + dp3<label> mt=5'),      # KS 4, labels
    C('c32_d64_m1', 31, 1, 64, 12.0, L | C32, 'fwd2<4,4,label> chunks=1',
      'de3<label> rows=1 + dp3<label> mt=1'),      # a single prototype: every pixel kind b
    C('c32_d64_p1', 1, 31, 64, 12.0, T | C32, 'fwd2<4,4,tag> chunks=1',
      'de3<tag> rows=1 + dp3<tag> mt=1'),      # a single pixel
    C('c32_d65', 257, 130, 65, 12.0, T | C32, 'fwd2<5,2,tag> chunks=1',
      'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=5'),      # KS 5 lower edge: fwd2 with MTB 2, round-2 backward
    C('c32_d80', 70, 97, 80, 12.0, L | PL | C32, 'fwd2_plain<5,2,label> chunks=1',
      'de<5,3,label> + dp<5,3,label> chunks=1 mt=4', zero_block=True),      # KS 5 upper edge, PLAIN
    # PLAIN at the remaining (bucket, predicate) pairs: nll_fwd2_plain<2,4,true>, <3,4,false>, <5,2,true>
    C('c32_d17_plain', 129, 33, 17, 12.0, T | PL | C32, 'fwd2_plain<2,4,tag> chunks=1',
      'de2<2,1,tag> rows=1 + dp<2,1,tag> chunks=1 mt=2'),
    C('c32_d48_plain', 70, 97, 48, 12.0, L | PL | C32, 'fwd2_plain<3,4,label> chunks=1',
      'de2<3,2,label> rows=1 + dp<3,2,label> chunks=1 mt=4'),
    C('c32_d65_plain', 129, 130, 65, 16.0, T | PL | C32, 'fwd2_plain<5,2,tag> chunks=1',
      'de<5,3,tag> + dp<5,3,tag> chunks=1 mt=5'),
    C('c32_d80_l', 257, 33, 80, 6.0, L | C32, 'fwd2<5,2,label> chunks=1',
      'de<5,3,label> + dp<5,3,label> chunks=2 mt=2'),      # KS 5, labels, kappa 6
    # ---- prototypes in runs of 48 of one code: tiles inside a run take the one-predicate epilogue of nll_fwd2 (UNI), tiles
    #      that straddle two runs and the ragged last tile the general one.  Tiles 0, 2, 3 of every 6 lie inside a run.
    C('uni_d64_l', 257, 130, 64, 12.0, L | C32, 'fwd2<4,4,label> chunks=1',
      'de3<label> rows=1 + dp3<label> mt=5', runs=48),      # 5 tiles (odd): uniform 0, 2; straddling 1; mixed 3; ragged 4
    C('uni_d33_t', 129, 161, 33, 12.0, T | C32, 'fwd2<3,4,tag> chunks=1',
      'de2<3,2,tag> rows=1 + dp<3,2,tag> chunks=1 mt=6', runs=48),      # 6 tiles (even); a second bit on the whole run 1
    C('uni_d17_lp', 70, 130, 17, 12.0, L | PL | C32, 'fwd2_plain<2,4,label> chunks=1',
      'de2<2,1,label> rows=1 + dp<2,1,label> chunks=1 mt=5', runs=48),      # the inverted predicate of the UNI epilogue
    C('uni_d80_tp', 257, 161, 80, 12.0, T | PL | C32, 'fwd2_plain<5,2,tag> chunks=1',
      'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=6', runs=48),      # ... with tag sets, MTB 2
    C('uni_d64_2chunks_t', 70, 3100, 64, 12.0, T | C32, 'fwd2<4,4,tag> chunks=2',
      'de3<tag> rows=2 + dp3<tag> mt=97', runs=48),      # 65 runs over two chunks: every class has several runs
    C('uni_d48_2chunks_lp', 70, 3100, 48, 12.0, L | PL | C32, 'fwd2_plain<3,4,label> chunks=2',
      'de2<3,2,label> rows=2 + dp<3,2,label> chunks=1 mt=97', runs=48),
    # ---- prototype chunks of 3072: the forward's partial sums, the chunk-to-row wrap of the v2 / v3 backward
    C('c32_d33_2chunks', 70, 3100, 33, 12.0, L | C32, 'fwd2<3,4,label> chunks=2',
      'de2<3,2,label> rows=2 + dp<3,2,label> chunks=1 mt=97'),      # two forward chunks, two backward rows
    C('c32_d64_2chunks', 70, 3100, 64, 12.0, T | C32, 'fwd2<4,4,tag> chunks=2',
      'de3<tag> rows=2 + dp3<tag> mt=97'),      # two chunks on de3 / dp3
    C('c32_d80_2chunks', 70, 3100, 80, 16.0, T | C32, 'fwd2<5,2,tag> chunks=2',
      'de<5,3,tag> + dp<5,3,tag> chunks=1 mt=97'),      # two forward chunks of fwd2<5,2>
    C('c32_d64_9chunks', 70, 24700, 64, 16.0, L | C32, 'fwd2<4,4,label> chunks=9',
      'de3<label> rows=8 + dp3<label> mt=772'),      # nine chunks on eight rows: row 0 takes chunks 0 and 8 (de3)
    C('c32_d48_9chunks', 70, 24700, 48, 16.0, T | C32, 'fwd2<3,4,tag> chunks=9',
      'de2<3,2,tag> rows=8 + dp<3,2,tag> chunks=1 mt=772'),      # nine chunks on eight rows (de2<3,2>)
    C('c32_d80_9chunks', 70, 24700, 80, 16.0, L | C32, 'fwd2<5,2,label> chunks=9',
      'de<5,3,label> + dp<5,3,label> chunks=1 mt=772'),      # nine forward chunks
    # ---- the switches of the 64-channel backward: de3 + re-prepared fragments + nll_bwd_dp<4,2>; nll_bwd_de2<4,2>
    C('c32_d49_dp3off', 257, 130, 49, 12.0, L | C32, 'fwd2<4,4,label> chunks=1',
      'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=5', env=DP3_OFF),
    C('c32_d49_de3off', 257, 130, 49, 12.0, L | C32, 'fwd2<4,4,label> chunks=1',
      'de2<4,2,label> rows=1 + dp<4,2,label> chunks=2 mt=5', env=DE3_OFF),
    C('c32_d50_dp3off', 257, 130, 50, 12.0, T | PL | C32, 'fwd2_plain<4,4,tag> chunks=1',
      'de3<tag> rows=1 + dp<4,2,tag> chunks=2 mt=5', env=DP3_OFF),
    C('c32_d50_de3off', 257, 130, 50, 12.0, T | PL | C32, 'fwd2_plain<4,4,tag> chunks=1',
      'de2<4,2,tag> rows=1 + dp<4,2,tag> chunks=2 mt=5', env=DE3_OFF),
    C('c32_d63_dp3off', 257, 130, 63, 12.0, T | C32, 'fwd2<4,4,tag> chunks=1',
      'de3<tag> rows=1 + dp<4,2,tag> chunks=2 mt=5', env=DP3_OFF),
    C('c32_d63_de3off', 257, 130, 63, 12.0, T | C32, 'fwd2<4,4,tag> chunks=1',
      'de2<4,2,tag> rows=1 + dp<4,2,tag> chunks=2 mt=5', env=DE3_OFF),
    C('c32_d64_dp3off', 257, 130, 64, 12.0, L | PL | C32, 'fwd2_plain<4,4,label> chunks=1',
      'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=5', env=DP3_OFF),
    C('c32_d64_de3off', 257, 130, 64, 12.0, L | PL | C32, 'fwd2_plain<4,4,label> chunks=1',
      'de2<4,2,label> rows=1 + dp<4,2,label> chunks=2 mt=5', env=DE3_OFF),
    C('c32_d64_2chunks_de3off', 70, 3100, 64, 12.0, T | C32, 'fwd2<4,4,tag> chunks=2',
      'de2<4,2,tag> rows=2 + dp<4,2,tag> chunks=1 mt=97', env=DE3_OFF),      # de2<4,2> on two rows
    # ---- 64-bit codes: nll_fwd<KS,1,TAG,false>, nll_bwd_de<KS,DT,TAG,false> + nll_bwd_dp<KS,DT,TAG,false>
    C('c64_d2', 33, 31, 2, 6.0, L, 'fwd<2,1,label,c64>',
      'de<2,1,label> + dp<2,1,label> chunks=1 mt=1'),      # KS 2
    C('c64_d17', 129, 130, 17, 12.0, T, 'fwd<2,1,tag,c64>',
      'de<2,1,tag> + dp<2,1,tag> chunks=1 mt=5'),      # KS 2, two workgroups of nll_fwd
    C('c64_d32', 70, 97, 32, 12.0, L | PL, 'fwd<2,1,label,c64>',
      'de<2,1,label> + dp<2,1,label> chunks=1 mt=4'),      # KS 2 upper edge, PLAIN
    C('c64_d33', 257, 33, 33, 12.0, L | PL, 'fwd<3,1,label,c64>',
      'de<3,2,label> + dp<3,2,label> chunks=2 mt=2'),      # KS 3 lower edge, PLAIN
    C('c64_d48', 129, 130, 48, 12.0, T, 'fwd<3,1,tag,c64>',
      'de<3,2,tag> + dp<3,2,tag> chunks=1 mt=5', bit40=True),      # KS 3 upper edge, class 0 at bit 40
    C('c64_d49', 257, 130, 49, 12.0, L, 'fwd<4,1,label,c64>',
      'de<4,2,label> + dp<4,2,label> chunks=2 mt=5', bit40=True),      # KS 4 lower edge, class 0 = label 2^40
    C('c64_d64', 70, 97, 64, 16.0, T | PL, 'fwd<4,1,tag,c64>',
      'de<4,2,tag> + dp<4,2,tag> chunks=1 mt=4'),      # KS 4 upper edge
    C('c64_d65', 129, 33, 65, 12.0, L | PL, 'fwd<5,1,label,c64>',
      'de<5,3,label> + dp<5,3,label> chunks=1 mt=2'),      # KS 5 lower edge
    C('c64_d80', 257, 130, 80, 12.0, T, 'fwd<5,1,tag,c64>',
      'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=5', dp_init=True),      # KS 5 upper edge
    C('c64_d81', 70, 97, 81, 12.0, L, 'fwd<9,1,label,c64>',
      'de<9,5,label> + dp<9,5,label> chunks=1 mt=4'),      # KS 9 lower edge
    C('c64_d96', 129, 130, 96, 12.0, T | PL, 'fwd<9,1,tag,c64>',
      'de<9,5,tag> + dp<9,5,tag> chunks=1 mt=5'),      # KS 6 in the 9 bucket: three padded k-steps
    C('c64_d144', 257, 33, 144, 12.0, T, 'fwd<9,1,tag,c64>',
      'de<9,5,tag> + dp<9,5,tag> chunks=2 mt=2'),      # KS 9 upper edge
    C('c64_d145', 70, 130, 145, 12.0, L | PL, 'fwd<17,1,label,c64>',
      'de<17,9,label> + dp<17,9,label> chunks=1 mt=5'),      # KS 17 lower edge
    C('c64_d160', 129, 97, 160, 16.0, L, 'fwd<17,1,label,c64>',
      'de<17,9,label> + dp<17,9,label> chunks=1 mt=4'),      # KS 10 in the 17 bucket: seven padded k-steps
    C('c64_d272', 257, 130, 272, 12.0, T, 'fwd<17,1,tag,c64>',
      'de<17,9,tag> + dp<17,9,tag> chunks=2 mt=5'),      # KS 17 upper edge
    # ---- 32-bit codes above 80 channels: nll_fwd<9|17|33,1,TAG,true>; the backward is the 64-bit one
    C('c32_d81', 129, 130, 81, 12.0, T | C32, 'fwd<9,1,tag,c32>',
      'de<9,5,tag> + dp<9,5,tag> chunks=1 mt=5'),      # KS 9 lower edge
    C('c32_d96', 257, 97, 96, 12.0, L | C32, 'fwd<9,1,label,c32>',
      'de<9,5,label> + dp<9,5,label> chunks=2 mt=4'),      # KS 6 in the 9 bucket
    C('c32_d144', 70, 33, 144, 12.0, L | PL | C32, 'fwd<9,1,label,c32>',
      'de<9,5,label> + dp<9,5,label> chunks=1 mt=2'),      # KS 9 upper edge, PLAIN
    C('c32_d145', 129, 130, 145, 12.0, T | PL | C32, 'fwd<17,1,tag,c32>',
      'de<17,9,tag> + dp<17,9,tag> chunks=1 mt=5'),      # KS 17 lower edge
    C('c32_d160', 257, 130, 160, 12.0, L | C32, 'fwd<17,1,label,c32>',
      'de<17,9,label> + dp<17,9,label> chunks=2 mt=5', zero_block=True),      # KS 10 in the 17 bucket
    C('c32_d272', 70, 97, 272, 12.0, T | C32, 'fwd<17,1,tag,c32>',
      'de<17,9,tag> + dp<17,9,tag> chunks=1 mt=4'),      # KS 17 upper edge
    # ---- wide embeddings: nll_fwd<33,..>; nll_bwd_de / _dp<33,3,TAG,false,1> + <33,7,TAG,false,2> once or twice
    C('wide_d273', 257, 130, 273, 12.0, L, 'fwd<33,1,label,c64>',
      'wide<label> strips=1 launches=1+1 mt=5'),      # KS 33 lower edge: a TM = 2 launch with 177 live channels of 224
    C('wide_d320', 129, 97, 320, 12.0, T | C32, 'fwd<33,1,tag,c32>',
      'wide<tag> strips=1 launches=1+1 mt=4'),      # the last width of one TM = 2 launch
    C('wide_d321', 257, 130, 321, 12.0, L | PL | C32, 'fwd<33,1,label,c32>',
      'wide<label> strips=1 launches=1+2 mt=5'),      # second TM = 2 launch with one live channel, PLAIN
    C('wide_d400', 70, 33, 400, 12.0, T | PL, 'fwd<33,1,tag,c64>',
      'wide<tag> strips=1 launches=1+2 mt=2'),      # tag sets + PLAIN
    C('wide_d528', 257, 130, 528, 16.0, T, 'fwd<33,1,tag,c64>',
      'wide<tag> strips=1 launches=1+2 mt=5', dp_init=True),      # the widest
    # three strips (8, 8 and 1 pixel tiles): P = 513 is the smallest, see test_three_strips_start_at_513_pixels
    C('wide_d273_3strips', 513, 545, 273, 12.0, T | C32, 'fwd<33,1,tag,c32>',
      'wide<tag> strips=3 launches=1+1 mt=18', env=STRIPS3),
    C('wide_d321_3strips', 513, 545, 321, 12.0, L, 'fwd<33,1,label,c64>',
      'wide<label> strips=3 launches=1+2 mt=18', env=STRIPS3),
    C('wide_d528_3strips', 513, 545, 528, 12.0, T | PL | C32, 'fwd<33,1,tag,c32>',
      'wide<tag> strips=3 launches=1+2 mt=18', env=STRIPS3),
    # ---- deterministic mode, one case per dPr route: 64-bit fixed-point sums
    C('det_dp', 257, 130, 80, 12.0, T | C32, 'fwd2<5,2,tag> chunks=1',
      'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=5 fix64', det=True),      # nll_bwd_dp
    C('det_dp3', 257, 130, 64, 12.0, T | C32, 'fwd2<4,4,tag> chunks=1',
      'de3<tag> rows=1 + dp3<tag> mt=5 fix64', det=True),      # nll_bwd_dp3 and dp3_own_term_kernel
    C('det_wide', 257, 130, 321, 12.0, T, 'fwd<33,1,tag,c64>',
      'wide<tag> strips=1 launches=1+2 mt=5 fix64', det=True),      # the wide strips
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# extra backward calls on a case's inputs: (case, m_grad, backward path)
MGRAD = [
    ('c64_d80', 0, 'de<5,3,tag> + no dp'),                                  # the round-2 pair
    ('c64_d80', 1, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=1'),
    ('c64_d80', 31, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=1'),
    ('c64_d80', 32, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=1'),
    ('c64_d80', 33, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=2'),
    ('c64_d80', 129, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=5'),
    ('c64_d80', 130, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=5'),
    ('c64_d80', 135, 'de<5,3,tag> + dp<5,3,tag> chunks=2 mt=5'),
    ('c32_d64_l', 0, 'de3<label> rows=1 + no dp'),                          # nll_bwd_dp3 + its own-term kernel
    ('c32_d64_l', 1, 'de3<label> rows=1 + dp3<label> mt=1'),
    ('c32_d64_l', 31, 'de3<label> rows=1 + dp3<label> mt=1'),
    ('c32_d64_l', 32, 'de3<label> rows=1 + dp3<label> mt=1'),
    ('c32_d64_l', 33, 'de3<label> rows=1 + dp3<label> mt=2'),
    ('c32_d64_l', 129, 'de3<label> rows=1 + dp3<label> mt=5'),
    ('c32_d64_l', 130, 'de3<label> rows=1 + dp3<label> mt=5'),
    ('c32_d64_l', 135, 'de3<label> rows=1 + dp3<label> mt=5'),
    ('wide_d321', 0, 'wide<label> strips=1 launches=1+2 mt=0'),             # the wide strips
    ('wide_d321', 1, 'wide<label> strips=1 launches=1+2 mt=1'),
    ('wide_d321', 31, 'wide<label> strips=1 launches=1+2 mt=1'),
    ('wide_d321', 32, 'wide<label> strips=1 launches=1+2 mt=1'),
    ('wide_d321', 33, 'wide<label> strips=1 launches=1+2 mt=2'),
    ('wide_d321', 129, 'wide<label> strips=1 launches=1+2 mt=5'),
    ('wide_d321', 130, 'wide<label> strips=1 launches=1+2 mt=5'),
    ('wide_d321', 135, 'wide<label> strips=1 launches=1+2 mt=5'),
    ('c32_d49_dp3off', 0, 'de3<label> rows=1 + no dp'),                     # round-2 dPr after the v3 dE kernel
    ('c32_d49_dp3off', 1, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=1'),
    ('c32_d49_dp3off', 31, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=1'),
    ('c32_d49_dp3off', 32, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=1'),
    ('c32_d49_dp3off', 33, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=2'),
    ('c32_d49_dp3off', 129, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=5'),
    ('c32_d49_dp3off', 130, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=5'),
    ('c32_d49_dp3off', 135, 'de3<label> rows=1 + dp<4,2,label> chunks=2 mt=5'),
]


class applied:
  """The case's environment switches and deterministic mode for the duration of a `with` block."""

  def __init__(self, case):
    self.case = case

  def __enter__(self):
    import os
    from spml_amd import _ffi
    self.saved = {k: os.environ.get(k) for k in ('SPML_NLL_DE3', 'SPML_NLL_DP3', 'SPML_NLL_TCACHE_MB')}
    for k in self.saved:
      os.environ.pop(k, None)
    os.environ.update(dict(self.case.env))
    self.det = _ffi.set_deterministic(self.case.det)
    return self

  def __exit__(self, *exc):
    import os
    from spml_amd import _ffi
    _ffi.set_deterministic(self.det)
    for k, v in self.saved.items():
      os.environ.pop(k, None)
      if v is not None:
        os.environ[k] = v
    return False


def tile_kinds(pr_code, m):
  """(uniform, straddling) counts of the full 32-prototype tiles by their codes' low words, as nll_fwd2 decides."""
  low = pr_code & 0xffffffff
  uni = sum(1 for t in range(m // 32) if bool((low[32 * t:32 * t + 32] == low[32 * t]).all()))
  return uni, m // 32 - uni


def path_names(case, m_grad=None):
  """(forward, backward) path names of a case from the library's route query (no GPU)."""
  from spml_amd import _ffi
  with applied(case):
    return (_ffi.segsort_nll_path_name(case.p, case.m, case.d, case.mode, False),
            _ffi.segsort_nll_path_name(case.p, case.m, case.d, case.mode, True, case.m_grad if m_grad is None else m_grad))

