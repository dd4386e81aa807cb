#!/usr/bin/env python3
"""The near-tie bar of the seeded draw's operator test (tests/test_decode_sample_gpu.py), measured on the CPU: the largest
relative distance between the race keys in an fp32 emulation of decode_sample_kernel's arithmetic and the fp64 keys of the
restatement (tests/decode_sample_util.py), over the operator test's own inputs; tol = 10 x that.
  python tools/decode_sample_tolerance.py [--write]
--write stores tol in tests/golden/decode_sample_tolerance.json, which the test reads.
Columns whose fp32 numerator exp(y - max) is below the normal range are left out: the kernel's exp2 flushes them to 0, their
relative error is unbounded, and their keys are at most 2^-126 / 6e-8 ~ 2e-31 against a winner's >= 1 / 16.7 (the maximum's own
key: e = 1, -log(u) <= 24 log 2), so none of them is ever a winner or a runner-up."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decode_sample_util as U   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--write", action="store_true")
a = ap.parse_args()

x = U.operator_logits().numpy()
worst, worst_at, n_keys, mismatch, closest = 0.0, None, 0, 0, 1.0
for t in U.OP_TEMPERATURES:
  for row in range(x.shape[0]):
    y = U.divide(x[row], t)
    for draw in U.OP_DRAWS:
      u = U.uniforms(U.OP_SEED, row, draw, 0, U.OP_V)
      k64 = U.race_keys(y, u)
      k32, e32 = U.race_keys_fp32(y, u)
      ok = e32 > 0
      rel = np.abs(k32[ok].astype(np.float64) - k64[ok]) / k64[ok]
      n_keys += int(ok.sum())
      if rel.max() > worst:
        worst, worst_at = float(rel.max()), (t, row, draw)
      mismatch += int(np.argmax(k32) != np.argmax(k64))
      closest = min(closest, U.runner_up_gap(k64))
tol = 10 * worst
print(f"{n_keys} keys over {len(U.OP_TEMPERATURES) * x.shape[0] * len(U.OP_DRAWS)} draws: largest relative distance fp32 emulation vs "
      f"fp64 {worst:.3e} at (T, row, draw) = {worst_at}; tol = 10 x = {tol:.3e}")
print(f"fp32 emulation picks another token than fp64 in {mismatch} draws; closest fp64 runner-up at {closest:.3e} of the winner")
if a.write:
  path = os.path.join(ROOT, "tests", "golden", U.TOLERANCE_FILE)
  with open(path, "w") as f:
    json.dump({"tol": tol, "largest_relative_key_distance": worst, "at_temperature_row_draw": list(worst_at), "keys": n_keys}, f,
              indent=1)
    f.write("\n")
  print("wrote", path)
