"""The denoise loop's kernels started part-way (gill_op_sd_sampler_run_from) under a teacher: B = 2, n = 256, every sampler, start 0 and 3 of
6 steps, against sampler_util.apply_rows on the host table in float64 — the bar of tests/test_samplers_gpu.py (10 x the measured distance
between an fp32 and an fp64 run of the restatement)."""
import numpy as np
import pytest
import torch

import sampler_util as U
import vae_encoder_util as V
from test_samplers_gpu import BAR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("kind,eta", [("pndm", 0.0), ("ddim", 0.0), ("ddim", 0.7), ("dpmsolver++", 0.0), ("euler", 0.0), ("euler_ancestral", 0.0)])
def test_loop_from_a_start(cuda, kind, eta, start):
  from gill_amd import ops
  B, n, N, g = 2, 256, 6, 7.5
  k, ts, sig, rows, (a, b) = V.native_schedule_from(kind, 0, N, start, eta)
  x0, mo, z = U.teacher_inputs(50 + start, k, B, 2 * B, n)
  z0 = np.random.default_rng(60 + start).standard_normal((B, n)).astype(np.float32)
  noisy = bool((rows[:, 11] != 0).any())
  t = lambda v: torch.from_numpy(v).to(cuda)  # noqa: E731
  got_l, got_i = ops.sd_sampler_run_from(kind, False, N, start, g, t(x0), t(z0), t(mo), t(z) if noisy else None, eta=eta)
  xs = a * x0.astype(np.float64) + b * z0.astype(np.float64)
  want_l, want_i = U.apply_rows(rows, 1.0, g, xs, mo, z)
  gl, gi = got_l.cpu().numpy(), got_i.cpu().numpy()
  first = U.rel_l2(gi[0], rows[0, 5] * xs)      # the first UNet input is in_scale * (a x0 + b noise)
  worst = max(max(U.rel_l2(gl[i], want_l[i]), U.rel_l2(gi[i], want_i[i])) for i in range(k))
  print(f"[sampler from {kind} eta={eta} start={start}] first input rel_l2={first:.3e} worst per-call rel_l2={worst:.3e} (bar {BAR:.3e})")
  assert first <= BAR and worst <= BAR
