"""Plain-torch restatement of the AutoencoderKL encoder half (diffusers state-dict names) and of the image-to-image driver, for the
encoder / img2img tests and tools/vae_encoder_tolerance.py.  Written from the structure, not from the engine: NCHW fp32 (or fp64) torch ops.

`q` is applied to every tensor the engine STORES as bf16 (conv / GroupNorm / attention outputs); the identity gives the fp32 restatement,
`bf16_round` the restatement "with bf16 storage" whose distance from the former is the parity test's bar.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import sampler_util as U


def bf16_round(t: torch.Tensor) -> torch.Tensor:
  return t.to(torch.bfloat16).to(t.dtype)


def _ident(t):
  return t


def _gn(sd, p, x, groups, silu, q):
  y = F.group_norm(x, groups, sd[p + ".weight"].to(x.dtype), sd[p + ".bias"].to(x.dtype), 1e-6)
  return q(F.silu(y) if silu else y)


def _conv(sd, p, x, padding=1, stride=1):
  return F.conv2d(x, sd[p + ".weight"].to(x.dtype), sd[p + ".bias"].to(x.dtype), padding=padding, stride=stride)


def _resnet(sd, p, x, groups, q):
  h = q(_conv(sd, p + ".conv1", _gn(sd, p + ".norm1", x, groups, True, q)))
  h = _conv(sd, p + ".conv2", _gn(sd, p + ".norm2", h, groups, True, q))
  if (p + ".conv_shortcut.weight") in sd:
    x = _conv(sd, p + ".conv_shortcut", x, padding=0)
  return q(x + h)


def _attn(sd, p, x, groups, q):
  B, C, H, W = x.shape
  h = _gn(sd, p + ".group_norm", x, groups, False, q).permute(0, 2, 3, 1).reshape(B, H * W, C)
  lin = lambda n, t: F.linear(t, sd[f"{p}.{n}.weight"].to(t.dtype), sd[f"{p}.{n}.bias"].to(t.dtype))  # noqa: E731
  qq, k, v = q(lin("to_q", h) * C ** -0.5), q(lin("to_k", h)), q(lin("to_v", h))
  a = q(q(q(qq @ k.transpose(-1, -2)).softmax(-1)) @ v)
  o = lin("to_out.0", a).reshape(B, H, W, C).permute(0, 3, 1, 2)
  return q(x + o)


def encoder_moments(sd, image: torch.Tensor, block_out_channels, groups: int = 32, q=_ident, dtype=torch.float32) -> torch.Tensor:
  """image (B,3,H,W) in [-1,1] -> quant_conv(encoder(image)) with the logvar half clamped to [-30, 20]: (B, 2 lc, H/8, W/8)."""
  x = image.to(dtype)
  x = q(_conv(sd, "encoder.conv_in", q(x)))      # (the engine's im2col rounds the pixels to bf16)
  for i in range(4):
    for j in range(2):
      x = _resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", x, groups, q)
    if i < 3:      # Downsample2D(padding=0): pad right / bottom by one, stride-2 conv without padding
      x = q(_conv(sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", F.pad(x, (0, 1, 0, 1)), padding=0, stride=2))
  x = _resnet(sd, "encoder.mid_block.resnets.0", x, groups, q)
  x = _attn(sd, "encoder.mid_block.attentions.0", x, groups, q)
  x = _resnet(sd, "encoder.mid_block.resnets.1", x, groups, q)
  x = _gn(sd, "encoder.conv_norm_out", x, groups, True, q)
  m = _conv(sd, "quant_conv", _conv(sd, "encoder.conv_out", x), padding=0)
  mean, logvar = m.chunk(2, dim=1)
  return torch.cat([mean, logvar.clamp(-30.0, 20.0)], 1)


def sample_latents(moments: torch.Tensor, noise, scaling: float) -> torch.Tensor:
  mean, logvar = moments.chunk(2, dim=1)
  return scaling * (mean if noise is None else mean + torch.exp(0.5 * logvar) * noise.to(moments.dtype))


def test_images(B: int, side: int, seed: int = 0) -> torch.Tensor:
  """Unit-scale smooth content plus noise, (B,3,side,side) in [-1,1]."""
  g = torch.Generator().manual_seed(seed)
  yy, xx = torch.meshgrid(torch.linspace(0, 1, side), torch.linspace(0, 1, side), indexing="ij")
  out = []
  for b in range(B):
    f = torch.rand((3, 4), generator=g) * 6.0 + 1.0
    base = torch.stack([torch.sin(f[c, 0] * xx + f[c, 1]) * torch.cos(f[c, 2] * yy + f[c, 3]) for c in range(3)], 0)
    out.append((0.8 * base + 0.1 * torch.randn((3, side, side), generator=g)).clamp(-1, 1))
  return torch.stack(out, 0)


# ---- schedulers started part-way (include/gill_amd.h gill_sd_schedule_from) ----
class DPMFromRef(U.DPMSolverPP2MRef):
  """DPM-Solver++(2M) handed the tail of its timestep list with an empty history: the first call is first order; lower_order_final is
  decided on the full list's length, as diffusers' scheduler does (its `timesteps` stay the full list)."""

  def start_at(self, n: int, start: int):
    self.set_timesteps(n)
    self.i = start
    return self.timesteps[start:]

  def step(self, model_output, t, sample, noise=None):
    if self.hist:
      return super().step(model_output, t, sample, noise)
    s0 = int(t)
    f = self._f
    a_s, sg_s, l_s = self._asl(s0)
    x0 = f(a_s) * sample - f(sg_s) * model_output if self.prediction_type == "v_prediction" else (sample - f(sg_s) * model_output) / f(a_s)
    tgt = 0 if self.i == self.n - 1 else int(self.timesteps[self.i + 1])
    a_t, sg_t, l_t = self._asl(tgt)
    out = f(sg_t / sg_s) * sample - f(a_t * (np.exp(-(l_t - l_s)) - 1)) * x0
    self.hist.append((s0, x0))
    self.i += 1
    return out


def pndm_tail_timesteps(n: int, start: int, steps_offset: int = 1):
  """t_s, t_s - D, t_s - D, t_s - 2D, ... down the n-step grid: n - start + 1 entries (the second may fall below 0 when start == n - 1)."""
  ratio = 1000 // n
  grid = [(n - 1 - i) * ratio + steps_offset for i in range(n)]
  ts = [grid[start], grid[start] - ratio, grid[start] - ratio] + grid[start + 2:]
  return ts[:n - start + 1]


class _Started:
  """A restated scheduler positioned at step `start` of its n-step schedule: .timesteps (the model's), .step, .scale_model_input, .add_noise."""

  def __init__(self, kind, n, start, pred="epsilon", eta=0.0):
    self.kind, self.n, self.start = kind, n, start
    ac = U.alphas_cumprod()
    if kind == "pndm":
      from oracle.scheduler_ref import PNDMSchedulerRef
      self.s = PNDMSchedulerRef(prediction_type=pred)
      self.s.set_timesteps(n)
      self.raw = pndm_tail_timesteps(n, start) if start > 0 else list(self.s.timesteps)
      self.timesteps = [float(max(t, 0)) for t in self.raw]
      self.ab = (np.sqrt(ac[self.raw[0]]), np.sqrt(1 - ac[self.raw[0]]))
    else:
      self.s = DPMFromRef(pred, np.float64) if kind == "dpmsolver++" else U.make_ref(kind, pred, np.float64, eta)
      full = self.s.set_timesteps(n)
      self.s.i = start
      self.raw = self.timesteps = full[start:]
      if kind in ("euler", "euler_ancestral"):
        self.ab = (1.0, float(self.s.sigmas[start]))
      else:
        t0 = int(full[start])
        self.ab = (np.sqrt(ac[t0]), np.sqrt(1 - ac[t0]))

  def add_noise(self, x0, noise):
    return self.ab[0] * np.asarray(x0, dtype=np.float64) + self.ab[1] * np.asarray(noise, dtype=np.float64)

  def scale_model_input(self, x, t=None):
    return self.s.scale_model_input(x, t)

  def step(self, i, e, x, noise=None):
    if self.kind == "pndm":
      return self.s.step(torch.from_numpy(np.asarray(e, dtype=np.float64)), self.raw[i], torch.from_numpy(np.asarray(x, dtype=np.float64))).numpy()
    return self.s.step(e, self.raw[i], x, noise)


def run_from_ref(kind, pred, n, start, guidance, x0, init_noise, model_out, noise, eta=0.0):
  """sampler_util.run_ref from step `start`: -> (latents after every call, UNet input of every call) in float64."""
  sch = _Started(kind, n, start, pred, eta)
  B = x0.shape[0]
  lat = sch.add_noise(x0, init_noise)
  lats, ins = [], []
  for i in range(len(sch.timesteps)):
    ins.append(np.asarray(sch.scale_model_input(lat), dtype=np.float64))
    e = model_out[i].astype(np.float64)
    if guidance > 1.0:
      e = e[:B] + guidance * (e[B:] - e[:B])
    lat = sch.step(i, e, lat, None if noise is None else noise[i].astype(np.float64))
    lats.append(lat)
  return np.stack(lats), np.stack(ins)


def native_schedule_from(kind, v_prediction, n, start, eta=0.0):
  """-> (status or ncalls, timesteps, init_noise_sigma, rows, (a, b))"""
  import ctypes as C
  from gill_amd import _native as N
  cap = max(n, 0) + 2
  sp = N.gill_sd_sampler(kind=U.KINDS.index(kind), steps_offset=1, set_alpha_to_one=0, eta=eta)
  ts, sig, rows, ab = (C.c_float * cap)(), C.c_double(), (C.c_double * (cap * U.ROW))(), (C.c_double * 2)()
  k = N.lib().gill_sd_schedule_from(C.byref(sp), int(v_prediction), int(n), int(start), ts, C.byref(sig), rows, ab)
  if k <= 0:
    return k, None, None, None, None
  return k, np.array(ts[:k], dtype=np.float32), float(sig.value), np.array(rows[:k * U.ROW], dtype=np.float64).reshape(k, U.ROW), (ab[0], ab[1])


def img2img_ref(unet_sd, ucfg, vae_sd, vcfg, cond, uncond, image, kind, n, strength, guidance, seed):
  """The image-to-image pipeline on the CPU: fp32 encoder restatement, posterior sample, float64 add-noise, the fp32 oracle UNet under the
  float64 scheduler from the start index.  Draws from torch.Generator(seed) in the pipeline's order: posterior, add-noise, step noise."""
  from oracle import unet_ref
  g = torch.Generator().manual_seed(seed)
  B = cond.shape[0]
  if image.shape[0] != B:
    image = image.repeat(B // image.shape[0], 1, 1, 1)
  L = vcfg.latent_size
  mom = encoder_moments(vae_sd, image, vcfg.block_out_channels, vcfg.norm_num_groups)
  x0 = sample_latents(mom, torch.randn((B, vcfg.latent_channels, L, L), generator=g), vcfg.scaling_factor)
  z0 = torch.randn((B, vcfg.latent_channels, L, L), generator=g)
  start = n - min(int(n * strength), n)
  sch = _Started(kind, n, start)
  lat = sch.add_noise(x0.double().numpy(), z0.double().numpy())
  do_cfg = guidance > 1.0
  ctx = torch.cat([uncond.expand(B, -1, -1), cond], 0) if do_cfg else cond
  for i, t in enumerate(sch.timesteps):
    inp = torch.from_numpy(np.asarray(sch.scale_model_input(lat))).float()
    inp = torch.cat([inp] * 2) if do_cfg else inp
    eps = unet_ref.unet_forward(unet_sd, inp, torch.full((inp.shape[0],), float(t)), ctx, ucfg.block_out_channels, ucfg.num_heads,
                                ucfg.norm_num_groups)
    if do_cfg:
      eu, ec = eps.chunk(2)
      eps = eu + guidance * (ec - eu)
    lat = sch.step(i, eps.double().numpy(), lat)
  return torch.from_numpy(np.asarray(lat)).float(), start
