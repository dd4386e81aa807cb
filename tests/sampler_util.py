"""Numpy restatements of the four schedulers the denoise loop can run besides PNDM — DDIM, DPM-Solver++(2M), Euler, Euler ancestral — as
diffusers 0.17.1 configures them for Stable Diffusion, for tests/test_samplers_host.py and tests/test_samplers_gpu.py.

They are written step by step (prediction -> x0 / eps -> update), NOT in the folded-coefficient form of the engine's tables (csrc/sd_schedule.hip:
sd_schedule), so that a folding mistake cannot be shared by both sides.  `dtype` is the arithmetic's precision: float64 is the reference, the
float32 run measures how far fp32 rounding alone moves a trajectory (the GPU test's tolerance).

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

KINDS = ("pndm", "ddim", "dpmsolver++", "euler", "euler_ancestral")
ROW = 12      # GILL_SD_ROW_DOUBLES


def alphas_cumprod() -> np.ndarray:
  """scaled_linear betas 0.00085..0.012 over 1000 train steps, in torch fp32 like every diffusers scheduler, widened."""
  betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
  return torch.cumprod(1.0 - betas, dim=0).double().numpy()


class _Base:
  init_noise_sigma = 1.0

  def __init__(self, prediction_type: str = "epsilon", dtype=np.float64):
    self.prediction_type = prediction_type
    self.dtype = dtype
    self.ac = alphas_cumprod()
    self.timesteps = []
    self.i = 0

  def _f(self, v):      # a table value (computed in double) as the arithmetic's dtype
    return self.dtype(v)

  def scale_model_input(self, sample, t=None):
    return sample


class DDIMRef(_Base):
  def __init__(self, prediction_type="epsilon", dtype=np.float64, steps_offset: int = 1, set_alpha_to_one: bool = False, eta: float = 0.0):
    super().__init__(prediction_type, dtype)
    self.steps_offset, self.set_alpha_to_one, self.eta = steps_offset, set_alpha_to_one, eta

  def set_timesteps(self, n: int):
    self.n, self.ratio, self.i = n, 1000 // n, 0
    self.timesteps = [float(i * self.ratio + self.steps_offset) for i in range(n - 1, -1, -1)]
    return self.timesteps

  def step(self, model_output, t, sample, noise=None):
    t = int(t)
    prev = t - self.ratio
    a_t = self.ac[t]
    a_p = self.ac[prev] if prev >= 0 else (1.0 if self.set_alpha_to_one else self.ac[0])
    f = self._f
    if self.prediction_type == "v_prediction":
      eps = f(np.sqrt(a_t)) * model_output + f(np.sqrt(1 - a_t)) * sample
      x0 = f(np.sqrt(a_t)) * sample - f(np.sqrt(1 - a_t)) * model_output
    else:
      eps = model_output
      x0 = (sample - f(np.sqrt(1 - a_t)) * eps) / f(np.sqrt(a_t))
    std = self.eta * np.sqrt((1 - a_p) / (1 - a_t)) * np.sqrt(1 - a_t / a_p)
    out = f(np.sqrt(a_p)) * x0 + f(np.sqrt(1 - a_p - std ** 2)) * eps
    if std > 0:
      out = out + f(std) * noise
    return out


class DPMSolverPP2MRef(_Base):
  def set_timesteps(self, n: int):
    self.n, self.i = n, 0
    ts = np.round(np.linspace(0, 999, n + 1))[::-1][:-1].astype(np.int64)
    self.timesteps = [float(t) for t in ts]
    self.hist = []       # (timestep, x0) of earlier calls
    return self.timesteps

  def _asl(self, t):
    a, s = np.sqrt(self.ac[t]), np.sqrt(1 - self.ac[t])
    return a, s, np.log(a) - np.log(s)

  def step(self, model_output, t, sample, noise=None):
    s0 = int(t)
    f = self._f
    a_s, sg_s, l_s = self._asl(s0)
    if self.prediction_type == "v_prediction":
      x0 = f(a_s) * sample - f(sg_s) * model_output
    else:
      x0 = (sample - f(sg_s) * model_output) / f(a_s)
    last = self.i == self.n - 1
    tgt = 0 if last else int(self.timesteps[self.i + 1])
    a_t, sg_t, l_t = self._asl(tgt)
    h = l_t - l_s
    if self.i == 0 or (last and self.n < 15):
      out = f(sg_t / sg_s) * sample - f(a_t * (np.exp(-h) - 1)) * x0
    else:
      s1, m1 = self.hist[-1]
      h0 = l_s - self._asl(s1)[2]
      r0 = h0 / h
      d1 = (x0 - m1) / f(r0)
      out = f(sg_t / sg_s) * sample - f(a_t * (np.exp(-h) - 1)) * x0 - f(0.5 * a_t * (np.exp(-h) - 1)) * d1
    self.hist.append((s0, x0))
    self.i += 1
    return out


class EulerRef(_Base):
  ancestral = False

  def set_timesteps(self, n: int):
    self.n, self.i = n, 0
    ts = np.linspace(0, 999, n)[::-1].copy()
    sig = np.sqrt((1 - self.ac) / self.ac)
    self.sigmas = np.concatenate([np.interp(ts, np.arange(1000), sig), [0.0]])
    self.timesteps = [float(t) for t in ts]
    self.init_noise_sigma = float(self.sigmas.max())
    return self.timesteps

  def scale_model_input(self, sample, t=None):
    s = self.sigmas[self.i]
    return sample / self._f(np.sqrt(s * s + 1))

  def step(self, model_output, t, sample, noise=None):
    s, to = self.sigmas[self.i], self.sigmas[self.i + 1]
    f = self._f
    if self.prediction_type == "v_prediction":
      x0 = sample / f(s * s + 1) - model_output * f(s / np.sqrt(s * s + 1))
      eps = (sample - x0) / f(s)
    else:
      eps = model_output
    if not self.ancestral:
      out = sample + f(to - s) * eps
    else:
      up = np.sqrt(to ** 2 * (s ** 2 - to ** 2) / s ** 2)
      down = np.sqrt(to ** 2 - up ** 2)
      out = sample + f(down - s) * eps
      if up > 0:
        out = out + f(up) * noise
    self.i += 1
    return out


class EulerAncestralRef(EulerRef):
  ancestral = True


def make_ref(kind: str, prediction_type: str = "epsilon", dtype=np.float64, eta: float = 0.0, steps_offset: int = 1,
             set_alpha_to_one: bool = False):
  if kind == "ddim":
    return DDIMRef(prediction_type, dtype, steps_offset, set_alpha_to_one, eta)
  return {"dpmsolver++": DPMSolverPP2MRef, "euler": EulerRef, "euler_ancestral": EulerAncestralRef}[kind](prediction_type, dtype)


def needs_noise(kind: str, eta: float = 0.0) -> bool:
  return kind == "euler_ancestral" or (kind == "ddim" and eta > 0)


def run_ref(kind, prediction_type, n_steps, guidance, lat0, model_out, noise, eta=0.0, dtype=np.float64):
  """The loop of custom_sd.py:607-646 with the UNet replaced by model_out [ncalls][Bx][...] (uncond rows then cond rows when guidance > 1).
  -> (latents after every call, UNet input of every call), each [ncalls][B][...] in `dtype`."""
  sch = make_ref(kind, prediction_type, dtype, eta)
  ts = sch.set_timesteps(n_steps)
  B = lat0.shape[0]
  lat = lat0.astype(dtype) * dtype(sch.init_noise_sigma)
  lats, ins = [], []
  for i, t in enumerate(ts):
    ins.append(sch.scale_model_input(lat, t))
    e = model_out[i].astype(dtype)
    if guidance > 1.0:
      eu, ec = e[:B], e[B:]
      e = eu + dtype(guidance) * (ec - eu)
    lat = sch.step(e, t, lat, None if noise is None else noise[i].astype(dtype))
    lats.append(lat)
  return np.stack(lats), np.stack(ins)


# ---- the engine's tables (gill_sd_schedule), and their application in numpy float64
def native_schedule(kind, v_prediction, n_steps, eta=0.0, steps_offset=1, set_alpha_to_one=0):
  """-> (status or ncalls, timesteps float32 [ncalls], init_noise_sigma, rows float64 [ncalls][ROW])"""
  from gill_amd import _native as N
  cap = max(n_steps, 0) + 2
  sp = N.gill_sd_sampler(kind=KINDS.index(kind) if isinstance(kind, str) else int(kind), steps_offset=steps_offset,
                         set_alpha_to_one=set_alpha_to_one, eta=eta)
  ts, sig, rows = (C.c_float * cap)(), C.c_double(), (C.c_double * (cap * ROW))()
  n = N.lib().gill_sd_schedule(C.byref(sp), int(v_prediction), int(n_steps), ts, C.byref(sig), rows)
  if n <= 0:
    return n, None, None, None
  return n, np.array(ts[:n], dtype=np.float32), float(sig.value), np.array(rows[:n * ROW], dtype=np.float64).reshape(n, ROW)


def apply_rows(rows, sigma0, guidance, lat0, model_out, noise):
  """The row semantics documented in include/gill_amd.h, in float64 -> (latents after every call, UNet input of every call)."""
  B = lat0.shape[0]
  x = lat0.astype(np.float64) * sigma0
  ring, saved = {}, None
  lats, ins = [], []
  for i, r in enumerate(rows):
    mode, slot_new, s1, s2, s3 = (int(v) for v in r[:5])
    in_scale, p_x, p_e, c_x, c_0, c_1, c_n = r[5:]
    ins.append(in_scale * x)
    e = model_out[i].astype(np.float64)
    if guidance > 1.0:
      e = e[:B] + guidance * (e[B:] - e[:B])
    if mode < 0:
      m = p_x * x + p_e * e
      if slot_new >= 0:
        ring[slot_new] = m
      y = c_x * x + c_0 * m
      if c_1 != 0:
        y = y + c_1 * ring[s1]
      if c_n != 0:
        y = y + c_n * noise[i].astype(np.float64)
    else:
      xs = x
      if mode == 0:
        ep, saved = e, x
        ring[slot_new] = e
      elif mode == 1:
        ep, xs = 0.5 * (e + ring[s1]), saved
      else:
        ring[slot_new] = e
        if mode == 2:
          ep = (3 * e - ring[s1]) / 2
        elif mode == 3:
          ep = (23 * e - 16 * ring[s1] + 5 * ring[s2]) / 12
        else:
          ep = (55 * e - 59 * ring[s1] + 37 * ring[s2] - 9 * ring[s3]) / 24
      y = c_x * xs + c_0 * ep
    x = y
    lats.append(x)
  return np.stack(lats), np.stack(ins)


def rel_l2(a, b) -> float:
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def teacher_inputs(seed, ncalls, B, Bx, n):
  rng = np.random.default_rng(seed)
  return (rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((ncalls, Bx, n)).astype(np.float32),
          rng.standard_normal((ncalls, B, n)).astype(np.float32))


# ---- the denoise loop of oracle/pipeline_ref.py::denoise with the scheduler as a parameter (custom_sd.py:588-651 without the VAE decode)
def denoise_ref(unet_sd, cond, uncond, latents, sched, num_inference_steps, guidance_scale, block_out_channels, heads, groups, noise=None):
  """sched: one of the restatements above (float64).  noise: [ncalls][B][4][L][L] torch tensor for the stochastic ones."""
  from oracle import unet_ref
  B = cond.shape[0]
  do_cfg = guidance_scale > 1.0
  if do_cfg and uncond.shape[0] != B:
    uncond = uncond.expand(B, -1, -1)
  ctx = torch.cat([uncond, cond], 0) if do_cfg else cond
  ts = sched.set_timesteps(num_inference_steps)
  lat = latents.double().numpy() * sched.init_noise_sigma
  for i, t in enumerate(ts):
    inp = sched.scale_model_input(lat, t)
    inp_t = torch.from_numpy(inp).float()
    inp_t = torch.cat([inp_t] * 2) if do_cfg else inp_t
    eps = unet_ref.unet_forward(unet_sd, inp_t, torch.full((inp_t.shape[0],), float(t)), ctx, block_out_channels, heads, groups)
    if do_cfg:
      eu, ec = eps.chunk(2)
      eps = eu + guidance_scale * (ec - eu)
    lat = sched.step(eps.double().numpy(), t, lat, None if noise is None else noise[i].double().numpy())
  return torch.from_numpy(lat).float()
