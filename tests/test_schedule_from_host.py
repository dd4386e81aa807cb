"""Host checks of the image-to-image tables (gill_sd_schedule_from: csrc/sd_schedule.hip); no GPU.

start = 0 is gill_sd_schedule bit for bit; DDIM / Euler / Euler ancestral are the full table's tail; DPM-Solver++ and PNDM are compared, through
sampler_util.apply_rows in float64, with the float64 steppers of vae_encoder_util started fresh at the tail — the same bar as
tests/test_samplers_host.py (one rounding of the folded coefficients to fp32: rel-L2 <= 1e-5 after every call)."""
import numpy as np
import pytest

import sampler_util as U
import vae_encoder_util as V

NS = (4, 10, 50)


def _starts(N):
  return sorted({0, 1, 2, N // 2, N - 2, N - 1})


@pytest.mark.parametrize("kind", U.KINDS)
def test_start_zero_is_the_text_to_image_table(kind):
  for N in NS:
    n0, ts0, sig0, rows0 = U.native_schedule(kind, 0, N, 0.5 if kind == "ddim" else 0.0)
    n1, ts1, sig1, rows1, _ = V.native_schedule_from(kind, 0, N, 0, 0.5 if kind == "ddim" else 0.0)
    assert n0 == n1 and np.array_equal(ts0, ts1) and sig0 == sig1 and np.array_equal(rows0, rows1)


@pytest.mark.parametrize("kind,eta", [("ddim", 0.0), ("ddim", 0.5), ("euler", 0.0), ("euler_ancestral", 0.0)])
def test_tail_of_the_full_table(kind, eta):
  for N in NS:
    _, ts0, sig0, rows0 = U.native_schedule(kind, 0, N, eta)
    for s in _starts(N):
      n, ts, sig, rows, _ = V.native_schedule_from(kind, 0, N, s, eta)
      assert n == N - s and np.array_equal(ts, ts0[s:]) and np.array_equal(rows, rows0[s:]) and sig == sig0, (kind, N, s)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("kind", ["dpmsolver++", "pndm"])
def test_rebuilt_heads_match_a_fresh_stepper(kind, pred):
  B, n = 2, 96
  for N in NS:
    for s in _starts(N):
      k, ts, sig, rows, ab = V.native_schedule_from(kind, pred == "v_prediction", N, s)
      assert k == (N - s + 1 if kind == "pndm" else N - s), (kind, N, s, k)
      sch = V._Started(kind, N, s, pred)
      assert np.array_equal(ts.astype(np.float64), np.array(sch.timesteps, dtype=np.float64)), (kind, N, s, ts, sch.timesteps)
      x0, mo, _ = U.teacher_inputs(3000 + 7 * N + s, k, B, B, n)
      z0 = np.random.default_rng(N + s).standard_normal((B, n)).astype(np.float32)
      want_l, want_i = V.run_from_ref(kind, pred, N, s, 1.0, x0, z0, mo, None)
      xs = ab[0] * x0.astype(np.float64) + ab[1] * z0.astype(np.float64)
      got_l, got_i = U.apply_rows(rows, 1.0, 1.0, xs, mo, None)
      worst = max(max(U.rel_l2(got_l[i], want_l[i]), U.rel_l2(got_i[i], want_i[i])) for i in range(k))
      assert worst <= 1e-5, (kind, pred, N, s, worst)
      if kind == "dpmsolver++" and k > 1:      # ring slots: every later row reads the slot the row before it wrote
        assert rows[0, 10] == 0.0 and all(int(rows[i, 2]) == int(rows[i - 1, 1]) for i in range(1, k))


@pytest.mark.parametrize("kind", U.KINDS)
def test_add_noise_pair(kind):
  """(a, b) against alphas_cumprod().  The library builds abar with its own fp32 product; tests/test_native_abi.py holds it to 5e-6 relative
  of the torch one, so the bars are that bound pushed through each formula: |da| <= 2.5e-6 a for a = sqrt(abar),
  |db| <= 2.5e-6 abar / b for b = sqrt(1 - abar), |dsigma| <= 2.5e-6 / (abar sigma) for sigma = sqrt(1 / abar - 1)."""
  ac = U.alphas_cumprod()
  for N in NS:
    for s in _starts(N):
      _, ts, _, _, (a, b) = V.native_schedule_from(kind, 0, N, s)
      if kind in ("euler", "euler_ancestral"):
        ref = U.make_ref(kind)
        ref.set_timesteps(N)
        sg = ref.sigmas[s]
        abar = ac[min(int(np.floor(ts[0])) + 1, 999)]      # the smaller abar of the two grid points the sigma is interpolated between
        assert a == 1.0 and abs(b - sg) <= 2.5e-6 / (abar * sg), (kind, N, s, a, b, sg)
      else:
        t = int(ts[0])
        ra, rb = np.sqrt(ac[t]), np.sqrt(1 - ac[t])
        assert abs(a - ra) <= 2.5e-6 * ra and abs(b - rb) <= 2.5e-6 * ac[t] / rb, (kind, N, s, a, b)
        assert abs(a * a + b * b - 1.0) <= 1e-12


def test_bad_start_is_an_error():
  from gill_amd import _native as N
  for kind in U.KINDS:
    for s in (-1, 10, 11):
      rc, *_ = V.native_schedule_from(kind, 0, 10, s)
      assert rc < 0 and b"start" in N.lib().gill_last_error(), (kind, s, rc)


def test_sampler_config_schedule_takes_a_start():
  from gill_amd.sd import SamplerConfig
  ts, sig, rows = SamplerConfig("ddim").schedule(10, start=4)
  n, ts2, sig2, rows2, ab = V.native_schedule_from("ddim", 0, 10, 4)
  assert n == 6 and np.array_equal(ts.numpy(), ts2) and np.array_equal(rows.numpy(), rows2)
  assert SamplerConfig("ddim").add_noise_pair(10, 4) == ab
