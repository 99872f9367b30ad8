"""Inputs for the bit-exact quantize / dequantize tests (test infrastructure only)."""
import numpy as np


def rounding_boundary_input(shape, bits, extract, seed=None):
  """A float32 [rows, cols] matrix aimed at the steps where a quantizer can go wrong: elements AT and one ulp
  either side of (k + 1/2) * bucket (round half to even decides), columns scaled by 2^-80 ... 2^80, denormals,
  exact zeros, a zero column, every column's maximum present; with `extract` symmetric, the diagonal above every
  column maximum.  The default seed is a function of (shape, bits)."""
  if seed is None:
    seed = hash((shape, bits, 6)) % (2 ** 31)
  rng = np.random.default_rng(seed)
  rows, cols = shape
  nb = np.float32(127.0 if bits == 8 else 32767.0)
  colmax = (rng.uniform(1.0, 2.0, size=cols) * np.exp2(rng.integers(-6, 7, size=cols))).astype(np.float32)
  wild = rng.uniform(size=cols) < 0.15
  colmax[wild] = (colmax[wild] * np.exp2(rng.choice([-80.0, -61.0, -59.0, 59.0, 61.0, 80.0], size=int(wild.sum())))
                  ).astype(np.float32)
  bucket = (colmax / nb).astype(np.float32)
  k = rng.integers(-int(nb) + 1, int(nb) - 1, size=shape).astype(np.float64)
  x = ((k + 0.5) * bucket.astype(np.float64)[None, :]).astype(np.float32)       # on a rounding boundary (or next to it)
  bump = rng.integers(-1, 2, size=shape)
  x = np.where(bump > 0, np.nextafter(x, np.float32(np.inf)), np.where(bump < 0, np.nextafter(x, np.float32(-np.inf)), x))
  x = x.astype(np.float32)
  x[rng.uniform(size=shape) < 0.05] = 0.0
  x[rng.uniform(size=shape) < 0.02] = np.float32(1e-41)                            # denormal
  x[rng.integers(0, rows, size=cols), np.arange(cols)] = colmax                     # the column maximum itself
  if cols > 2:
    x[:, 1] = 0.0
  if extract:
    x = np.triu(x) + np.triu(x, 1).T
    x[np.arange(rows), np.arange(rows)] = (colmax * 7).astype(np.float32)           # diagonal above every column maximum
  return np.ascontiguousarray(x, np.float32)
