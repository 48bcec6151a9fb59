"""numpy restatement of the split-f16 ("hl8") format of spml_amd/csrc/conv.hip, written from the format's description
(include/spml_hip.h, the header comment of conv.hip) and independent of the library: the converters are compared with
it bit for bit in tests/test_conv_gpu.py, and tests/test_conv_ref.py holds it to fp64 on its own.

  S = pow2_scale(bound) = 2^(14 - e), e the smallest integer with bound < 2^e, the exponent clamped to [-100, 100];
      1 for a bound that is not a positive finite number <= 1e38 (and where there is no bound)
  h = f16(x * S),  l = f16(x * S - h)          (fp32 arithmetic, round to nearest even, subnormal halves kept)
  [rows][C] -> 16-byte units ((row * C/8 + c/8) * 2 + part) of 8 consecutive channels, part 0 = h, 1 = l
"""
import numpy as np


def pow2_scale(bound):
  if bound is None:
    return np.float32(1.0)
  b = np.float32(bound)
  if not (b > 0) or b > np.float32(1e38):
    return np.float32(1.0)
  _, e = np.frexp(b)                     # b = m * 2^e, m in [0.5, 1): the smallest e with b < 2^e
  e = min(max(14 - int(e), -100), 100)
  return np.float32(np.ldexp(np.float32(1.0), e))


def hl8_parts(x, bound):
  """x fp32 [rows, C] -> (h, l) float16 [rows, C]."""
  x = np.asarray(x, dtype=np.float32)
  with np.errstate(over='ignore', invalid='ignore', under='ignore'):
    xs = x * pow2_scale(bound)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
  return h, l


def hl8_encode(x, bound):
  """x fp32 [rows, C] (C % 8 == 0) -> the hl8 bytes, uint8 [rows * C * 4]."""
  h, l = hl8_parts(x, bound)
  rows, c = h.shape
  units = np.stack([h.reshape(rows, c // 8, 8), l.reshape(rows, c // 8, 8)], axis=2)      # [rows][C/8][part][8]
  return np.ascontiguousarray(units).view(np.uint8).reshape(-1)


def hl8_decode(data, rows, c, bound):
  """hl8 bytes -> fp64 [rows, C] = (h + l) / S."""
  units = np.asarray(data, dtype=np.uint8).reshape(-1).view(np.float16).reshape(rows, c // 8, 2, 8).astype(np.float64)
  return (units[:, :, 0] + units[:, :, 1]).reshape(rows, c) / float(pow2_scale(bound))


def weight_forward(w):
  """conv weight [Cout, Cin, kh, kw] -> the forward operand's matrix [Cout][taps * Cin] (channels-last storage)."""
  w = np.asarray(w, dtype=np.float32)
  cout, cin, kh, kw = w.shape
  return np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(cout, kh * kw * cin)


def weight_transposed(w):
  """conv weight [Cout, Cin, kh, kw] -> the data-gradient operand's matrix [Cin][taps * Cout], element
  (ci, taps - 1 - tap, co) = w[co, ci, tap]: transposed, taps mirrored."""
  w = np.asarray(w, dtype=np.float32)
  cout, cin, kh, kw = w.shape
  t = w.reshape(cout, cin, kh * kw)[:, :, ::-1]                    # mirrored taps
  return np.ascontiguousarray(t.transpose(1, 2, 0)).reshape(cin, kh * kw * cout)
