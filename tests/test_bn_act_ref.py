"""tests/bn_act_ref.py (the float64 batch-norm reference the GPU cases are held to) against torch's own
double-precision batch_norm + autograd, its chunk statistics pooled back with Chan's formula, its hl8 decoder on a
hand-packed buffer, the geometry table against a restatement of the host functions, and the two bound formulas
against the float64 outputs on every input the GPU cases use."""
import pytest
import torch
import torch.nn.functional as F

import bn_act_ref as ref

EPS = 1e-5
SMALL = ((7, 4), (33, 8), (130, 12))


def _close(a, b, tol=1e-12):
  assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (a, b)


@pytest.mark.parametrize('relu,res', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('r,c', SMALL)
def test_reference_is_torch_double_batch_norm(r, c, relu, res):
  t = {k: v.double() for k, v in ref.make_inputs(r, c).items()}
  x = t['x'].clone().requires_grad_(True)
  rs = t['res'].clone().requires_grad_(True)
  gamma = t['gamma'].clone().requires_grad_(True)
  beta = t['beta'].clone().requires_grad_(True)
  rm, rv = torch.linspace(-1, 1, c).double(), torch.linspace(0.5, 2, c).double()
  rm0, rv0 = rm.clone(), rv.clone()
  y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, EPS)
  if res:
    y = y + rs
  if relu:
    y = torch.relu(y)
  (y * t['dy']).sum().backward()
  f = ref.forward(t['x'], t['gamma'], t['beta'], EPS, 0.1, relu, t['res'] if res else None, rm0, rv0)
  _close(f['y'], y.detach())
  _close(f['mean'], t['x'].mean(0))
  _close(f['m2'], t['x'].var(0, unbiased=False) * r)
  _close(f['invstd'], 1.0 / torch.sqrt(t['x'].var(0, unbiased=False) + EPS))
  assert torch.equal(f['cmax'], t['x'].max(0).values) and torch.equal(f['cmin'], t['x'].min(0).values)
  _close(f['running_mean'], rm)
  _close(f['running_var'], rv)
  b = ref.backward(t['dy'], t['x'], f['mean'], f['invstd'], t['gamma'], (f['y'] > 0) if relu else None)
  _close(b['dx'], x.grad)
  _close(b['s0'], beta.grad)
  _close(b['s1'], gamma.grad)
  _close(b['max_dz'], b['dz'].abs().max(0).values)
  if res:
    _close(b['d_residual'], rs.grad, 0.0)


def test_one_row_uses_the_divisor_one():
  t = ref.make_inputs(1, 8)
  f = ref.forward(t['x'], t['gamma'], t['beta'], EPS, 0.25, False, None, torch.zeros(8), torch.ones(8))
  assert torch.equal(f['m2'], torch.zeros(8, dtype=torch.float64))
  _close(f['invstd'], torch.full((8,), EPS ** -0.5, dtype=torch.float64))
  _close(f['y'], t['beta'].double().view(1, 8))
  _close(f['running_var'], torch.full((8,), 0.75, dtype=torch.float64))


@pytest.mark.parametrize('r,c,chunk_rows', [(7, 4, 3), (33, 8, 32), (130, 12, 129), (130, 12, 200), (64, 8, 32)])
def test_chunk_statistics_pool_back_to_the_whole_tensor(r, c, chunk_rows):
  t = ref.make_inputs(r, c)
  f = ref.forward(t['x'], t['gamma'], t['beta'], EPS, relu=True)
  st = ref.chunk_stats_fwd(t['x'], chunk_rows)
  assert st.shape == (4, (r + chunk_rows - 1) // chunk_rows, c)
  mean, m2, hi, lo = ref.pool_chunk_stats_fwd(st, r, chunk_rows)
  _close(mean, f['mean'])
  _close(m2, f['m2'])
  assert torch.equal(hi, f['cmax']) and torch.equal(lo, f['cmin'])
  b = ref.backward(t['dy'], t['x'], f['mean'], f['invstd'], t['gamma'], f['y'] > 0)
  sb = ref.chunk_stats_bwd(b['dz'], t['x'], f['mean'], chunk_rows)
  assert sb.shape == (3, st.shape[1], c)
  _close(sb[0].sum(0), b['s0'])
  _close(sb[1].sum(0) * f['invstd'], b['s1'])
  assert torch.equal(sb[2].max(0).values, b['max_dz'])
  # the rank form of the same pooling: three unequal row ranges
  cuts = [(0, r // 3), (r // 3, r // 3 + 1), (r // 3 + 1, r)]
  parts = [ref.forward(t['x'][a:b_], t['gamma'], t['beta'], EPS) for a, b_ in cuts]
  counts = torch.tensor([[float(b_ - a)] * c for a, b_ in cuts])
  total, mean3, m23 = ref.pool_rank_stats(counts, torch.stack([p['mean'] for p in parts]),
                                          torch.stack([p['m2'] for p in parts]))
  assert torch.equal(total, torch.full((c,), float(r), dtype=torch.float64))
  _close(mean3, f['mean'])
  _close(m23, f['m2'])


class _Packed(object):
  def __init__(self, data, bound, rows, channels):
    self.data, self.bound, self.rows, self.channels = data, bound, rows, channels


def test_decode_hl8_on_a_hand_packed_buffer():
  # 2 rows x 16 channels, bound 3.0 -> e = 2, S = 2^12.  Unit order: (row, channel octet, part): h then l.
  vals = torch.arange(32, dtype=torch.float64).view(2, 16) * 0.25 - 3.0
  s = 2.0 ** 12
  h = (vals * s).to(torch.float16)
  l = torch.full((2, 16), 2.0 ** -24, dtype=torch.float16)             # the smallest f16 subnormal in every low half
  units = []
  for row in range(2):
    for octet in range(2):
      units += [h[row, 8 * octet:8 * octet + 8], l[row, 8 * octet:8 * octet + 8]]
  data = torch.cat(units).view(torch.uint8)
  assert data.numel() == 2 * 16 * 4
  assert ref.pow2_scale(3.0) == s and ref.pow2_scale(4.0) == 2.0 ** 11 and ref.pow2_scale(0.75) == 2.0 ** 14
  got = ref.decode_hl8(_Packed(data, torch.tensor([3.0]), 2, 16))
  assert torch.equal(got, vals + 2.0 ** -24 / s)
  halves = ref.hl8_halves(_Packed(data, torch.tensor([3.0]), 2, 16))
  assert torch.equal(halves[1, 1, 0], h[1, 8:]) and torch.equal(halves[0, 0, 1], l[0, :8])
  for bad in (0.0, -1.0, float('nan'), float('inf'), 2e38):             # bn_pow2_scale: scale 1
    assert ref.pow2_scale(bad) == 1.0
    got = ref.decode_hl8(_Packed(data, torch.tensor([bad]), 2, 16))
    assert torch.equal(got, vals * s + 2.0 ** -24)
  assert ref.pow2_scale(1e-38) == 2.0 ** 100 and ref.pow2_scale(1e38) == 2.0 ** -100      # the clamp of the exponent


def test_mask_bits():
  mask = torch.tensor([0b0001, 0b1010, 0b1111, 0b0100], dtype=torch.uint8)      # 2 rows x 2 quads
  want = torch.tensor([[1, 0, 0, 0, 0, 1, 0, 1], [1, 1, 1, 1, 0, 0, 1, 0]]).bool()
  assert torch.equal(ref.mask_bits(mask, 2, 8), want)


def test_geometry_table_is_what_the_host_functions_compute():
  for row in ref.GEOMETRY:
    assert ref.host_geometry(row[0], row[1]) == row
  cqs = {ref.host_geometry(r, c)[2] for r, c in ref.SHAPES}
  assert cqs == {4, 8, 16, 32, 64}
  assert ref.host_geometry(9, 4)[2:5] == (4, 1, 64) and ref.host_geometry(130, 12)[2:5] == (4, 1, 64)


def _bound_cases():
  for r, c in ref.SHAPES + ref.FP32_ONLY_SHAPES + ((1, 8),):
    yield r, c, False, False
  yield ref.OUTLIER_SHAPE + (True, False)
  yield ref.OUTLIER_SHAPE + (False, True)


@pytest.mark.parametrize('r,c,outlier,constant', list(_bound_cases()))
def test_bound_formulas_bound_the_float64_outputs(r, c, outlier, constant):
  """Forward: max |y| <= formula for residual / ReLU / both / neither.  Backward: max |dx| <= formula with and without
  the mask, on every input of the GPU cases.  (The formulas are evaluated from exact statistics here: no slack.)"""
  t = ref.make_inputs(r, c, outlier=outlier, constant=constant)
  resb = float(t['res'].abs().max())
  for relu in (False, True):
    for res in (False, True):
      f = ref.forward(t['x'], t['gamma'], t['beta'], EPS, 0.1, relu, t['res'] if res else None)
      fb = ref.bound_fwd(f['mean'], f['invstd'], t['gamma'], t['beta'], f['cmax'], f['cmin'], resb if res else 0.0)
      assert float(f['y'].abs().max()) <= fb * (1 + 1e-12)
      b = ref.backward(t['dy'], t['x'], f['mean'], f['invstd'], t['gamma'], (f['y'] > 0) if relu else None)
      args = (f['mean'], f['invstd'], t['gamma'], f['cmax'], f['cmin'], b['s0'], b['s1'], b['max_dz'], float(r))
      bb = ref.bound_bwd(*args)
      assert float(b['dx'].abs().max()) <= bb * (1 + 1e-12) + 1e-300
      assert torch.isfinite(f['y']).all() and torch.isfinite(b['dx']).all()
      if outlier:
        # the case exists so that a bound without its third term is unsound: the outlier channel carries the tensor's
        # bound, its third term is the largest, and max |dx| lies above the sum of the other two
        t0, t1, t2 = ref.bound_bwd_terms(*args)
        k = int((t0 + t1 + t2).argmax())
        assert k == ref.OUTLIER_CHANNEL and float(t2[k]) > float(t0[k] + t1[k])
        assert float(b['dx'].abs().max()) > 1.05 * float((t0 + t1).max())
