"""Host half of the seeded draw (gill_opt_sample_token): Philox4x32-10 against known answers, gill_decode_uniforms (the kernel's
own Philox and word -> uniform code, compiled for the host) against the numpy restatement, and the restatement's keys against
the softmax they are meant to sample."""
import ctypes as C
import math

import numpy as np

import decode_sample_util as U


def _words(counter, key):
  return [int(w) for w in U.philox4x32_10(counter, key)]


def test_philox_known_answers():
  f = 0xFFFFFFFF
  assert _words((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
  assert _words((f, f, f, f), (f, f)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
  assert _words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
      [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
  # vectorised over the counter: the same words as one block at a time
  c0 = np.arange(5)
  w = U.philox4x32_10((c0, 7, 9, 0), (123, 456))
  for j in range(5):
    assert [int(v[j]) for v in w] == _words((j, 7, 9, 0), (123, 456))


def test_uniform_mapping_is_exact_and_open():
  w = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
  u = U.word_to_uniform(w)
  assert u.dtype == np.float32
  assert u[0] == np.float32(2.0 ** -24) and u[2] == u[0] and u[3] == np.float32(3 * 2.0 ** -24)
  assert u[-1] == np.float32(1 - 2.0 ** -24) and u[4] + u[5] == 1.0          # symmetric about 1/2
  exact = (2 * (w.astype(np.int64) >> 9) + 1) * 2.0 ** -24
  assert np.array_equal(u.astype(np.float64), exact)                          # no rounding in fp32
  assert (u > 0).all() and (u < 1).all()


def _lib_uniforms(seed, row, draw, first, count):
  from gill_amd import _native as N
  out = (C.c_float * max(count, 1))()
  N.check(N.lib().gill_decode_uniforms(seed, row, draw, first, count, out))
  return np.frombuffer(out, dtype=np.float32, count=count).copy()


def test_decode_uniforms_match_restatement_bit_for_bit():
  V = 50274
  cases = [(0, 0, 0, 0, 9), (99, 3, 2, 50271, 3), (2 ** 64 - 1, 5, 63, 1, 2), (0x123456789ABCDEF, 11, 7, 1022, 1031),
           (7, 0, 1, 50273, 1), (7, 2 ** 31 - 1, 2 ** 31 - 1, 65533, 3), (12345, 1, 1, 0, V)]
  for seed, row, draw, first, count in cases:
    got = _lib_uniforms(seed, row, draw, first, count)
    want = U.uniforms(seed, row, draw, first, count)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, row, draw, first, count)
    assert (got > 0).all() and (got < 1).all()
  # a window is a slice of the row: the value of a column does not depend on where the window starts
  full = _lib_uniforms(99, 3, 2, 0, V)
  assert np.array_equal(full[50271:], _lib_uniforms(99, 3, 2, 50271, 3))
  # seed halves, row and draw all reach the stream
  base = _lib_uniforms(5, 1, 1, 0, 64)
  for other in [(6, 1, 1), (5 + 2 ** 32, 1, 1), (5, 2, 1), (5, 1, 2)]:
    assert not np.array_equal(base, _lib_uniforms(*other, 0, 64)), other


def test_decode_uniforms_bad_arguments():
  from gill_amd import _native as N
  lib = N.lib()
  out = (C.c_float * 4)()
  assert lib.gill_decode_uniforms(1, 0, 0, 0, 4, None) != 0
  assert lib.gill_last_error()
  assert lib.gill_decode_uniforms(1, -1, 0, 0, 4, out) != 0
  assert lib.gill_decode_uniforms(1, 0, -1, 0, 4, out) != 0
  assert lib.gill_decode_uniforms(1, 0, 0, -1, 4, out) != 0
  assert lib.gill_decode_uniforms(1, 0, 0, 65534, 4, out) != 0
  assert lib.gill_decode_uniforms(1, 0, 0, 0, 0, out) == 0


def _chi2_sf(x, k):
  """upper tail of chi-square with k = 7 degrees of freedom in closed form (odd k):
  Q = erfc(sqrt(x / 2)) + sqrt(2 x / pi) exp(-x / 2) (1 + x / 3 + x^2 / 15)."""
  assert k == 7
  return math.erfc(math.sqrt(x / 2)) + math.sqrt(2 * x / math.pi) * math.exp(-x / 2) * (1 + x / 3 + x * x / 15)


def _chi2_quantile(p_upper, k):
  lo, hi = 0.0, 200.0
  for _ in range(200):
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if _chi2_sf(mid, k) > p_upper else (lo, mid)
  return hi


def test_restatement_samples_the_softmax():
  p = np.array([.4, .25, .15, .1, .05, .03, .015, .005])
  y = np.log(p).astype(np.float32)
  counts = np.zeros(8)
  for row in range(64):
    for draw in range(64):
      tok, keys = U.draws(y, 99, row, draw)
      assert keys is not None
      counts[tok] += 1
  n = counts.sum()
  assert n == 4096
  stat = float(((counts - n * p) ** 2 / (n * p)).sum())
  bar = _chi2_quantile(1e-6, 7)
  assert abs(_chi2_sf(14.0671, 7) - 0.05) < 1e-4          # the closed form against the textbook 95 % point
  print(f"chi-square {stat:.2f}, bar {bar:.2f}")
  assert 40 < bar < 45                                     # 1 - 1e-6 quantile, 7 degrees of freedom
  assert stat < bar, (stat, bar, counts)


def test_restatement_rows_that_do_not_draw():
  y = np.array([1.0, np.nan, 5.0, np.nan], dtype=np.float32)
  assert U.draws(y, 1, 0, 0) == (1, None)
  y = np.array([1.0, np.inf, 5.0, np.inf], dtype=np.float32)
  assert U.draws(y, 1, 0, 0) == (1, None)
  y = np.full(5, -np.inf, dtype=np.float32)
  assert U.draws(y, 1, 0, 0) == (0, None)
  # a kept mask of one column decides the draw
  y = np.array([0.0, 1.0, 2.0], dtype=np.float32)
  assert U.draws(y, 1, 0, 0, keep=np.array([False, True, False]))[0] == 1
