"""tests/conv_ref.py (the numpy restatement of the hl8 format the GPU converters are compared with bit for bit) against
fp64, on its own.  The bounds are derived, not measured:

  bound in [2^(e-1), 2^e) and S = 2^(14-e), so S * bound in [2^13, 2^14).
  |x| >= 2^-15 * bound:  |x S| >= 2^-2, h = f16(x S) is a normal half, |x S - h| <= 2^-11 |x S|; l = f16(x S - h)
      rounds that residual to 2^-11 of itself (normal) or to half a subnormal step, 2^-25 <= 2^-23 |x S|:
      |(h + l) / S - x| <= 2^-22 |x|.
  below that: the residual is below 2^-13, a subnormal half or nearly one: |(h + l) - x S| <= 2^-25, i.e. an absolute
      error of at most 2^-25 / S <= 2^-38 * bound.

Bounds below 2^-86 (and above 2^114) are kept out: the clamp of the scale's exponent to [-100, 100] stops S from
following the bound there, and the relative bound does not hold."""
import numpy as np
import pytest

import conv_ref

REL = 2.0 ** -22
ABS = 2.0 ** -38


def _draw(rng, bound, n=2048):
  # magnitudes from the bound itself down to 2^-40 of it, both signs, the bound among them, zeros
  x = bound * np.exp2(-rng.uniform(0, 40, size=n)) * rng.choice([-1.0, 1.0], size=n)
  x[0], x[1], x[2] = bound, -bound, 0.0
  x[3] = bound * 2.0 ** -15
  return x.astype(np.float32).reshape(-1, 8)


@pytest.mark.parametrize('seed', range(6))
def test_round_trip_stays_inside_the_derived_bounds(seed):
  rng = np.random.default_rng(seed)
  worst_rel, worst_abs = 0.0, 0.0
  for _ in range(50):
    bound = np.float32(10.0 ** rng.uniform(-20, 20))
    x = _draw(rng, float(bound))
    bound = np.float32(np.abs(x).max())                     # (the computed bound: max |x| in fp32)
    s = float(conv_ref.pow2_scale(bound))
    assert 2.0 ** 13 <= s * float(bound) < 2.0 ** 14
    back = conv_ref.hl8_decode(conv_ref.hl8_encode(x, bound), x.shape[0], x.shape[1], bound)
    x64 = x.astype(np.float64)
    err = np.abs(back - x64)
    big = np.abs(x64) >= 2.0 ** -15 * float(bound)
    assert (err[big] <= REL * np.abs(x64[big])).all()
    assert (err[~big] <= ABS * float(bound)).all()
    worst_rel = max(worst_rel, float((err[big] / np.abs(x64[big])).max()))
    worst_abs = max(worst_abs, float(err[~big].max() / float(bound)))
  print('worst relative %.3f x 2^-22, worst absolute %.3f x 2^-38 of the bound' % (worst_rel / REL, worst_abs / ABS))


def test_a_loose_bound_keeps_the_absolute_error():
  """A given bound above max |x| (the batch norm's bound is an upper bound): the same two regimes relative to it."""
  rng = np.random.default_rng(11)
  x = _draw(rng, 1.0)
  for bound in (1.0, 1.5, 3.999, 4.0, 1000.0):
    back = conv_ref.hl8_decode(conv_ref.hl8_encode(x, bound), x.shape[0], x.shape[1], bound)
    x64 = x.astype(np.float64)
    err = np.abs(back - x64)
    big = np.abs(x64) >= 2.0 ** -15 * bound
    assert (err[big] <= REL * np.abs(x64[big])).all() and (err[~big] <= ABS * bound).all()


def test_scale_edges():
  one = np.float32(1.0)
  for bound in (None, 0.0, -1.0, float('inf'), float('nan'), 2e38):
    assert conv_ref.pow2_scale(bound) == one
  assert conv_ref.pow2_scale(1.0) == np.float32(2.0 ** 13)             # 1 < 2^1: an exact power of two takes the next e
  assert conv_ref.pow2_scale(np.nextafter(np.float32(1.0), np.float32(0))) == np.float32(2.0 ** 14)
  assert conv_ref.pow2_scale(16384.0) == np.float32(0.5)
  for e in range(-80, 100, 7):
    b = np.float32(2.0 ** e)
    assert float(conv_ref.pow2_scale(b)) * float(b) == 2.0 ** 13       # the scaled tensor stays below 2^14
  # the clamp: past it the scale no longer follows the bound
  assert conv_ref.pow2_scale(2.0 ** -90) == np.float32(2.0 ** 100) == conv_ref.pow2_scale(2.0 ** -120)
  assert conv_ref.pow2_scale(1e38) == np.float32(2.0 ** -100)


def test_layout_of_the_units_and_the_weight_operands():
  rows, c = 3, 16
  x = (np.arange(rows * c, dtype=np.float32) + 1).reshape(rows, c)      # small integers: h exact, l zero
  raw = conv_ref.hl8_encode(x, None).view(np.float16)
  for r in range(rows):
    for ch in range(c):
      for part in range(2):
        unit = (r * (c // 8) + ch // 8) * 2 + part
        assert raw[unit * 8 + ch % 8] == (x[r, ch] if part == 0 else 0)
  # a value with a non-zero low part lands in part 1 of the same unit
  y = np.zeros((1, 8), np.float32)
  y[0, 5] = 1.0 + 2.0 ** -12
  raw = conv_ref.hl8_encode(y, None).view(np.float16)
  assert raw[5] == 1.0 and raw[8 + 5] == np.float16(2.0 ** -12)
  assert conv_ref.hl8_decode(raw.view(np.uint8), 1, 8, None)[0, 5] == 1.0 + 2.0 ** -12
  # weights: forward [Cout][tap][Cin]; transposed [Cin][taps - 1 - tap][Cout]
  cout, cin = 8, 16
  w = np.random.default_rng(3).standard_normal((cout, cin, 3, 3)).astype(np.float32)
  f, t = conv_ref.weight_forward(w), conv_ref.weight_transposed(w)
  assert f.shape == (cout, 9 * cin) and t.shape == (cin, 9 * cout)
  for co, ci, kh, kw in [(0, 0, 0, 0), (7, 15, 2, 1), (3, 4, 1, 1), (5, 9, 0, 2)]:
    tap = 3 * kh + kw
    assert f[co, tap * cin + ci] == w[co, ci, kh, kw]
    assert t[ci, (8 - tap) * cout + co] == w[co, ci, kh, kw]
  w1 = w[:, :, :1, :1]
  assert (conv_ref.weight_transposed(w1) == w1[:, :, 0, 0].T).all()


def test_subnormal_halves_are_kept():
  x = np.zeros((1, 8), np.float32)
  x[0, 0] = 2.0 ** -20                   # below the smallest normal half (2^-14): a subnormal h
  x[0, 1] = 1.0 + 2.0 ** -20             # low part 2^-20: a subnormal l
  h, l = conv_ref.hl8_parts(x, None)
  assert float(h[0, 0]) == 2.0 ** -20 and float(l[0, 1]) == 2.0 ** -20
