"""The seeded draw of gill_opt_sample_token / gill_opt_draw_token restated in numpy (the contract is in include/gill_amd.h):
Philox4x32-10, the word -> uniform mapping, the exponential-race keys in fp64 and the rule for rows that cannot draw."""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
  """counter: 4 integers or arrays (broadcast together), key: 2 integers -> 4 uint32 arrays, the output words."""
  c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
  k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
  for _ in range(10):
    p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
  return [v.astype(np.uint32) for v in c]


def word_to_uniform(w):
  """(2 * (w >> 9) + 1) * 2^-24 as fp32: an odd multiple of 2^-24 below 2^24 of them, so exact."""
  w = np.asarray(w, dtype=np.uint32)
  return ((2 * (w >> np.uint32(9)).astype(np.int64) + 1).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def uniforms(seed, row, draw, first, count):
  """u_c for c in [first, first + count): counter (c >> 2, row, draw, 0), key (seed low, seed high), output word c & 3."""
  c = np.arange(first, first + count, dtype=np.int64)
  words = philox4x32_10((c >> 2, row, draw, 0), (seed & 0xFFFFFFFF, seed >> 32))
  w = np.choose(c & 3, words)
  return word_to_uniform(w)


def divide(x, t):
  """step 1: correctly rounded fp32 division"""
  with np.errstate(over="ignore", invalid="ignore"):
    return (np.asarray(x, dtype=np.float32) / np.float32(t)).astype(np.float32)


def argmax_rule(y):
  """torch.argmax's pick: the first NaN, else the larger value, else the lower index."""
  nan = np.isnan(y)
  return int(np.argmax(nan)) if nan.any() else int(np.argmax(y))


def race_keys(y, u, keep=None):
  """fp64 keys exp(y - max) / -log(u) of one row with a finite maximum; -1 on the columns outside `keep`."""
  y64 = np.asarray(y, dtype=np.float64)
  with np.errstate(under="ignore"):
    keys = np.exp(y64 - y64.max()) / -np.log(np.asarray(u, dtype=np.float64))
  if keep is not None:
    keys = np.where(keep, keys, -1.0)
  return keys


def draws(y, seed, row, draw, keep=None):
  """(token, keys) of one row of divided logits y; keys is None where the row does not draw (no finite maximum)."""
  y = np.asarray(y, dtype=np.float32)
  if np.isnan(y).any() or not np.isfinite(y.max()):
    return argmax_rule(y), None
  keys = race_keys(y, uniforms(seed, row, draw, 0, y.shape[0]), keep)
  return int(np.argmax(keys)), keys          # np.argmax: the lower index on ties


def uniforms_rows(seed, rows, draw, count):
  """(len(rows), count): uniforms() of every row in one vectorised Philox call"""
  return _uniforms_rows(int(seed), tuple(int(r) for r in rows), int(draw), int(count))


@functools.lru_cache(maxsize=4)
def _uniforms_rows(seed, rows, draw, count):
  blocks = np.arange((count + 3) // 4, dtype=np.int64)[None, :]          # one Philox call per block of four columns
  words = philox4x32_10((blocks, np.asarray(rows, dtype=np.int64)[:, None], draw, 0), (seed & 0xFFFFFFFF, seed >> 32))
  return word_to_uniform(np.stack(words, axis=-1).reshape(len(rows), -1)[:, :count])


def judge_rows(tokens, y, seed, row0, draw, keep, tol):
  """judge() of every row b of y (B, V) as row row0 + b, vectorised over the rows that draw; keep: (B, V) bool or None."""
  y = np.asarray(y, dtype=np.float32)
  B, V = y.shape
  with np.errstate(invalid="ignore"):
    mx = np.nanmax(np.where(np.isnan(y), -np.inf, y), axis=1)
  draws_ = ~np.isnan(y).any(axis=1) & np.isfinite(mx)
  verdicts = [None] * B
  for b in np.nonzero(~draws_)[0]:
    verdicts[b] = "exact" if int(tokens[b]) == argmax_rule(y[b]) else "wrong"
  rows = np.nonzero(draws_)[0]
  if rows.size:
    u = uniforms_rows(seed, row0 + rows, draw, V)
    y64 = y[rows].astype(np.float64)
    with np.errstate(under="ignore"):
      keys = np.exp(y64 - mx[rows, None]) / -np.log(u.astype(np.float64))
    if keep is not None:
      keys = np.where(np.asarray(keep)[rows], keys, -1.0)
    want = np.argmax(keys, axis=1)
    for j, b in enumerate(rows):
      t = int(tokens[b])
      if t == want[j]:
        verdicts[b] = "exact"
      elif 0 <= t < V and keys[j, want[j]] - keys[j, t] <= tol * keys[j, want[j]]:
        verdicts[b] = "near"
      else:
        verdicts[b] = "wrong"
  return verdicts


def race_keys_fp32(y, u):
  """The kernel's arithmetic emulated in fp32: e = __expf(y - mx) = exp2(fp32(log2(e)) * fp32(y - mx)) with the product and the
  result rounded to fp32 and results below the normal range flushed to 0 (the hardware exp2 is good to 1 ulp; the emulation rounds
  the exact power correctly), E = fp32(-log(u)) (logf is good to 1 ulp likewise), key = fp32(e / E)."""
  y = np.asarray(y, dtype=np.float32)
  d = (y - y.max()).astype(np.float32)
  a = (np.float32(1.4426950408889634) * d).astype(np.float32)
  with np.errstate(under="ignore"):
    e = np.exp2(a.astype(np.float64)).astype(np.float32)
  e = np.where(e < np.float32(2.0 ** -126), np.float32(0), e)
  big_e = (-np.log(np.asarray(u, dtype=np.float64))).astype(np.float32)
  return (e / big_e).astype(np.float32), e


# the operator test's inputs (tests/test_decode_sample_gpu.py), shared with tools/decode_sample_tolerance.py
OP_V = 50274
OP_SEED = 0x5EEDC0FFEE123457
OP_TEMPERATURES = (0.7, 1.3)
OP_TOP_PS = (1.0, 0.9, 0.5)
OP_DRAWS = (0, 1, 2, 3)
TOLERANCE_FILE = "decode_sample_tolerance.json"       # under tests/golden


def operator_logits():
  import torch
  g = torch.Generator().manual_seed(4)
  return torch.randn((64, OP_V), generator=g) * torch.linspace(2.0, 8.0, 64)[:, None]


def load_tolerance():
  import json
  import os
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)) as f:
    return float(json.load(f)["tol"])


def runner_up_gap(keys):
  """relative distance of the second-largest key from the largest"""
  top2 = np.partition(keys, -2)[-2:]
  return float((top2[1] - top2[0]) / top2[1])


def judge(token, y, seed, row, draw, keep, tol):
  """'exact' when token is the fp64 argmax, 'near' when it is not but its own fp64 key is within tol (relative) of the winner's (so
  the runner-up's is too), else 'wrong'."""
  want, keys = draws(y, seed, row, draw, keep)
  if token == want:
    return "exact"
  if keys is None or not 0 <= token < keys.shape[0]:
    return "wrong"
  return "near" if keys[want] - keys[token] <= tol * keys[want] else "wrong"
