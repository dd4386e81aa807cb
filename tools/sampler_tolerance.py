"""How far fp32 rounding alone moves a sampler trajectory: tests/sampler_util's restatements run once in float32 and once in float64 numpy
on the inputs of tests/test_samplers_gpu.py::test_sampler_kernels_vs_float64_restatement, largest per-call rel-L2 per sampler.  CPU only.
The GPU test's bar is 10 x the largest figure printed here (its F32_DISTANCE)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sampler_util as U  # noqa: E402
import test_samplers_gpu as T  # noqa: E402


def main():
  worst = {}
  for (B, n, N, g) in T.kernel_cases():
    for kind, eta in T.SAMPLERS:
      for pred in ("epsilon", "v_prediction"):
        lat0, mo, z = U.teacher_inputs(T._seed(B, n, N), N, B, 2 * B if g > 1 else B, n)
        z = z if U.needs_noise(kind, eta) else None
        l64, i64 = U.run_ref(kind, pred, N, g, lat0, mo, z, eta, np.float64)
        l32, i32 = U.run_ref(kind, pred, N, g, lat0, mo, z, eta, np.float32)
        assert l32.dtype == np.float32 and i32.dtype == np.float32
        w = max(max(U.rel_l2(l32[i], l64[i]), U.rel_l2(i32[i], i64[i])) for i in range(N))
        if w > worst.get((kind, eta, pred), (0.0,))[0]:
          worst[(kind, eta, pred)] = (w, (B, n, N, g))
  for k, (w, c) in worst.items():
    print(f"{k[0]:16s} eta={k[1]:<4} {k[2]:13s} {w:.3e}  at (B, n, calls, guidance) = {c}")
  print(f"largest: {max(w for w, _ in worst.values()):.3e}   (test bar: {T.BAR:.3e})")


if __name__ == "__main__":
  main()
