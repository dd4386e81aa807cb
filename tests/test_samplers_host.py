"""Host checks of the sampler tables (gill_sd_schedule: csrc/sd_schedule.hip) and of the scheduler_config.json parsing; no GPU.

sampler_util restates DDIM, DPM-Solver++(2M), Euler and Euler ancestral step by step in float64 numpy; the engine's rows are folded
coefficients rounded to fp32 once.  Applied in float64 to the same seeded model outputs and noise, the two trajectories may differ by that one
rounding and nothing else: rel-L2 <= 1e-5 after every call.
"""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

import sampler_util as U

NS = (1, 2, 3, 14, 15, 20, 50)
CASES = [(k, 0.0) for k in ("dpmsolver++", "euler", "euler_ancestral")] + [("ddim", e) for e in (0.0, 0.5, 1.0)]


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("kind,eta", CASES)
def test_schedule_matches_restatement(kind, eta, pred):
  B, n = 2, 96
  for N in NS:
    ref = U.make_ref(kind, pred, np.float64, eta)
    ts_ref = np.array(ref.set_timesteps(N))
    ncalls, ts, sig0, rows = U.native_schedule(kind, pred == "v_prediction", N, eta)
    assert ncalls == N == len(ts_ref), (kind, N, ncalls)
    if kind in ("ddim", "dpmsolver++"):
      assert np.array_equal(ts.astype(np.float64), ts_ref), (kind, N, ts, ts_ref)
    assert np.all(np.abs(ts - ts_ref) <= 1e-6 * np.maximum(np.abs(ts_ref), 1e-30)), (kind, N, ts, ts_ref)
    assert abs(sig0 - ref.init_noise_sigma) <= 1e-6 * ref.init_noise_sigma, (kind, N, sig0, ref.init_noise_sigma)
    if kind in ("euler", "euler_ancestral") and N > 1:      # (a single call runs at t = 0, whose sigma is small)
      assert sig0 > 14.0
    lat0, mo, z = U.teacher_inputs(1000 + N, N, B, B, n)
    noisy = U.needs_noise(kind, eta)
    # (Euler ancestral's last call targets sigma 0 and adds no noise: a single call reads none)
    assert bool((rows[:, 11] != 0).any()) == ((kind == "ddim" and eta > 0) or (kind == "euler_ancestral" and N > 1)), (kind, N, rows[:, 11])
    want_l, want_i = U.run_ref(kind, pred, N, 1.0, lat0, mo, z if noisy else None, eta)
    got_l, got_i = U.apply_rows(rows, sig0, 1.0, lat0, mo, z)
    worst = max(max(U.rel_l2(got_l[i], want_l[i]), U.rel_l2(got_i[i], want_i[i])) for i in range(N))
    assert worst <= 1e-5, (kind, eta, pred, N, worst)


def test_lower_order_final_switches_at_15():
  """DPM-Solver++: the last call is first order (no history term) below 15 calls, second order from 15 on."""
  _, _, _, r14 = U.native_schedule("dpmsolver++", 0, 14)
  _, _, _, r15 = U.native_schedule("dpmsolver++", 0, 15)
  assert r14[-1, 10] == 0.0 and r15[-1, 10] != 0.0
  assert r14[0, 10] == 0.0 and r15[0, 10] == 0.0 and np.all(r14[1:-1, 10] != 0.0)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_pndm_through_sd_schedule_matches_oracle(pred):
  import torch
  from oracle.scheduler_ref import PNDMSchedulerRef
  B, n = 2, 96
  for N in (2, 3, 14, 15, 20, 50):
    ref = PNDMSchedulerRef(prediction_type=pred)
    ts_ref = ref.set_timesteps(N)
    ncalls, ts, sig0, rows = U.native_schedule("pndm", pred == "v_prediction", N)
    assert ncalls == N + 1 and [int(t) for t in ts] == ts_ref and sig0 == 1.0
    lat0, mo, _ = U.teacher_inputs(2000 + N, ncalls, B, B, n)
    got_l, got_i = U.apply_rows(rows, sig0, 1.0, lat0, mo, None)
    lat = torch.from_numpy(lat0).double()
    for i, t in enumerate(ts_ref):
      assert U.rel_l2(got_i[i], lat.numpy()) <= 1e-5
      lat = ref.step(torch.from_numpy(mo[i]).double(), t, lat)
      assert U.rel_l2(got_l[i], lat.numpy()) <= 1e-5, (pred, N, i)


def test_bad_arguments_report_errors_not_crashes():
  from gill_amd import _native as N
  lib = N.lib()
  for kind, steps, eta, word in ((7, 10, 0.0, b"kind"), (-1, 10, 0.0, b"kind"), ("ddim", 0, 0.0, b"num_steps"), ("euler", 0, 0.0, b"num_steps"),
                                 ("pndm", 1, 0.0, b"num_steps"), ("ddim", 10, -0.5, b"eta")):
    rc, *_ = U.native_schedule(kind, 0, steps, eta)
    assert rc < 0, (kind, steps, eta, rc)
    assert word in lib.gill_last_error(), (kind, steps, eta, lib.gill_last_error())
  assert lib.gill_sd_schedule(None, 0, 10, None, None, None) < 0 and lib.gill_last_error()
  sp = N.gill_sd_sampler(kind=1, steps_offset=1, set_alpha_to_one=0, eta=0.0)
  assert lib.gill_sd_schedule(C.byref(sp), 0, 10, None, None, None) == 10       # every output is optional


# ------------------------------------------------------------------------------------------------ scheduler_config.json
def _dir(tmp_path, cfg):
  d = tmp_path / "sd"
  os.makedirs(d / "scheduler")
  if cfg is not None:
    with open(d / "scheduler" / "scheduler_config.json", "w") as f:
      json.dump(cfg, f)
  return str(d)


@pytest.mark.parametrize("name,kind", [(None, "pndm"), ("PNDMScheduler", "pndm"), ("DDIMScheduler", "ddim"),
                                       ("DPMSolverMultistepScheduler", "dpmsolver++"), ("EulerDiscreteScheduler", "euler"),
                                       ("EulerAncestralDiscreteScheduler", "euler_ancestral")])
def test_scheduler_class_names(tmp_path, name, kind):
  from gill_amd.sd import parse_scheduler_config
  cfg = dict(prediction_type="v_prediction", beta_schedule="scaled_linear", steps_offset=1, set_alpha_to_one=False)
  if name:
    cfg["_class_name"] = name
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    s, pred = parse_scheduler_config(_dir(tmp_path, cfg))
  assert (s.kind, s.steps_offset, s.set_alpha_to_one, pred) == (kind, 1, False, "v_prediction")


def test_scheduler_config_absent_or_minimal_is_todays_pndm(tmp_path):
  from gill_amd.sd import parse_scheduler_config
  s, pred = parse_scheduler_config(_dir(tmp_path, None))
  assert (s.kind, s.steps_offset, s.set_alpha_to_one, pred) == ("pndm", 1, False, "epsilon")
  s, pred = parse_scheduler_config(_dir(tmp_path / "b", dict(prediction_type="epsilon")))
  assert (s.kind, s.steps_offset, s.set_alpha_to_one, pred) == ("pndm", 1, False, "epsilon")


def test_scheduler_fields_are_read(tmp_path):
  from gill_amd.sd import parse_scheduler_config
  s, _ = parse_scheduler_config(_dir(tmp_path, dict(_class_name="DDIMScheduler", steps_offset=0, set_alpha_to_one=True)))
  assert (s.kind, s.steps_offset, s.set_alpha_to_one) == ("ddim", 0, True)


def test_unknown_scheduler_class_warns_and_runs_pndm(tmp_path):
  from gill_amd.sd import parse_scheduler_config
  with pytest.warns(UserWarning, match="LMSDiscreteScheduler"):
    s, _ = parse_scheduler_config(_dir(tmp_path, dict(_class_name="LMSDiscreteScheduler")))
  assert s.kind == "pndm"


def test_unbuilt_configurations_raise(tmp_path):
  from gill_amd.sd import SamplerConfig, parse_scheduler_config
  with pytest.raises(ValueError, match="beta_schedule"):
    parse_scheduler_config(_dir(tmp_path / "a", dict(_class_name="DDIMScheduler", beta_schedule="linear")))
  with pytest.raises(ValueError, match="algorithm_type"):
    parse_scheduler_config(_dir(tmp_path / "b", dict(_class_name="DPMSolverMultistepScheduler", algorithm_type="dpmsolver")))
  with pytest.raises(ValueError, match="solver_order"):
    parse_scheduler_config(_dir(tmp_path / "c", dict(_class_name="DPMSolverMultistepScheduler", solver_order=3)))
  with pytest.raises(ValueError, match="unknown scheduler"):
    SamplerConfig(kind="heun")


def test_scheduler_argument_overrides_the_file(tmp_path):
  from gill_amd.sd import SamplerConfig, parse_scheduler_config
  d = _dir(tmp_path, dict(_class_name="PNDMScheduler", prediction_type="v_prediction"))
  s, pred = parse_scheduler_config(d, "ddim")
  assert (s.kind, pred) == ("ddim", "v_prediction")
  s, _ = parse_scheduler_config(d, "EulerDiscreteScheduler")
  assert s.kind == "euler"
  s, _ = parse_scheduler_config(d, SamplerConfig("ddim", steps_offset=0, set_alpha_to_one=True))
  assert (s.kind, s.steps_offset, s.set_alpha_to_one) == ("ddim", 0, True)
  with warnings.catch_warnings():           # the override also silences the unknown-class warning: the file's class is not used
    warnings.simplefilter("error")
    s, _ = parse_scheduler_config(_dir(tmp_path / "x", dict(_class_name="LMSDiscreteScheduler")), "dpmsolver++")
  assert s.kind == "dpmsolver++"


def test_sampler_config_schedule_is_the_native_table():
  from gill_amd.sd import SamplerConfig
  ts, sig0, rows = SamplerConfig("euler").schedule(7)
  n, ts2, sig2, rows2 = U.native_schedule("euler", 0, 7)
  assert n == 7 and np.array_equal(ts.numpy(), ts2) and sig0 == sig2 and np.array_equal(rows.numpy(), rows2)
  from gill_amd import _native as N
  with pytest.raises(N.GillNativeError):
    SamplerConfig("ddim").schedule(0)
