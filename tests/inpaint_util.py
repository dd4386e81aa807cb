"""CPU restatement of inpainting (include/gill_amd.h gill_sd_inpaint*): mask preprocessing, the keep table in float64, the row semantics of
sampler_util.apply_rows with the blend after every call, and the pipeline driver built from the pieces of vae_encoder_util / sampler_util.

Mask convention: values in [0,1], 1 = repaint from 0.5 up, 0 = keep.  diffusers is not installed: this file is the yardstick.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np
import torch

import sampler_util as U
import vae_encoder_util as V


# ---- mask preprocessing
def prepare_ref(image: torch.Tensor, mask: torch.Tensor):
  """image (B,3,H,W) in [-1,1], mask (B|1,1,H,W) in [0,1] -> (masked image (B,3,H,W), latent mask (B,1,H/8,W/8) in {0,1})."""
  B = image.shape[0]
  mb = (mask >= 0.5).to(torch.float32).expand(B, -1, -1, -1)
  return image * (1 - mb), mb[:, :, ::8, ::8].contiguous()     # F.interpolate(mask, size=(H/8, W/8)), nearest, for a factor of exactly 8


# ---- the keep table
def keep_ref(kind: str, n: int, start: int, pred: str = "epsilon", eta: float = 0.0) -> np.ndarray:
  """(ncalls,2) float64: the add_noise pair at the noise level the latents have AFTER call i of the table that starts at `start`."""
  ac = U.alphas_cumprod()
  if kind == "pndm":
    ts = V.pndm_tail_timesteps(n, start) if start > 0 else [int(t) for t in V._Started("pndm", n, 0, pred).raw]
    rows = [(np.sqrt(ac[max(int(t), 0)]), np.sqrt(1 - ac[max(int(t), 0)])) for t in ts[1:]]
  else:
    rows = [V._Started(kind, n, s, pred, eta).ab for s in range(start + 1, n)]
  return np.array([(float(a), float(b)) for a, b in rows] + [(1.0, 0.0)], dtype=np.float64)


def native_keep(kind, v_prediction, n, start, eta=0.0):
  """-> (status or ncalls, keep float64 (ncalls,2): the fp32 values the device reads, widened)"""
  import ctypes as C
  from gill_amd import _native as N
  cap = max(n, 0) + 2
  sp = N.gill_sd_sampler(kind=U.KINDS.index(kind), steps_offset=1, set_alpha_to_one=0, eta=eta)
  buf = (C.c_double * (2 * cap))()
  k = N.lib().gill_sd_inpaint_keep(C.byref(sp), int(v_prediction), int(n), int(start), buf)
  if k <= 0:
    return k, None
  return k, np.array(buf[:2 * k], dtype=np.float64).reshape(k, 2)


# ---- sampler_util.apply_rows with an operation on the latents after every call (the documented row semantics, float64)
def apply_rows_after(rows, guidance, x_start, model_out, noise, after=None):
  """-> (latents after every call [and after `after(i, x)`], UNet input of every call); x_start is the loop's first latents."""
  B = x_start.shape[0]
  x = x_start.astype(np.float64)
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
        ep = {2: lambda: (3 * e - ring[s1]) / 2, 3: lambda: (23 * e - 16 * ring[s1] + 5 * ring[s2]) / 12,
              4: lambda: (55 * e - 59 * ring[s1] + 37 * ring[s2] - 9 * ring[s3]) / 24}[mode]()
      y = c_x * xs + c_0 * ep
    x = y if after is None else after(i, y)
    lats.append(x)
  return np.stack(lats), np.stack(ins)


def blend(keep, x0, z0, m):
  """The blend of call i as a function for apply_rows_after: m broadcastable to x0 (1 = repaint)."""
  x0, z0, m = (np.asarray(v, dtype=np.float64) for v in (x0, z0, m))
  return lambda i, y: m * y + (1 - m) * (keep[i, 0] * x0 + keep[i, 1] * z0)


# ---- the pipeline on the CPU
def inpaint_ref(unet_sd, ucfg, vae_sd, vcfg, cond, uncond, image, mask, kind, n, strength, guidance, seed):
  """vae_encoder_util.img2img_ref with a mask.  ucfg.in_channels == out_channels: blend after every step; 2 * out_channels + 1: the UNet input is
  [scaled latents | latent mask | masked-image latents].  Draws from torch.Generator(seed) in the pipeline's order: the image's posterior
  noise, the masked image's (concat only), add-noise, step noise.  -> (latents, start)"""
  from oracle import unet_ref
  g = torch.Generator().manual_seed(seed)
  B = cond.shape[0]
  if image.shape[0] != B:
    image = image.repeat(B // image.shape[0], 1, 1, 1)
  concat = ucfg.in_channels != ucfg.out_channels
  L = vcfg.latent_size
  masked, lm = prepare_ref(image, mask)
  enc = lambda im: V.sample_latents(V.encoder_moments(vae_sd, im, vcfg.block_out_channels, vcfg.norm_num_groups),  # noqa: E731
                                    torch.randn((B, vcfg.latent_channels, L, L), generator=g), vcfg.scaling_factor)
  x0 = enc(image)
  xm = enc(masked) if concat else None
  z0 = torch.randn((B, vcfg.latent_channels, L, L), generator=g)
  start = n - min(int(n * strength), n)
  sch = V._Started(kind, n, start)
  keep = keep_ref(kind, n, start)
  assert len(keep) == len(sch.timesteps)
  lat = sch.add_noise(x0.double().numpy(), z0.double().numpy())
  after = blend(keep, x0.numpy(), z0.numpy(), lm.numpy())
  do_cfg = guidance > 1.0
  ctx = torch.cat([uncond.expand(B, -1, -1), cond], 0) if do_cfg else cond
  for i, t in enumerate(sch.timesteps):
    inp = torch.from_numpy(np.asarray(sch.scale_model_input(lat))).float()
    if concat:
      inp = torch.cat([inp, lm, xm], 1)
    inp = torch.cat([inp] * 2) if do_cfg else inp
    eps = unet_ref.unet_forward(unet_sd, inp, torch.full((inp.shape[0],), float(t)), ctx, ucfg.block_out_channels, ucfg.num_heads,
                                ucfg.norm_num_groups)
    if do_cfg:
      eu, ec = eps.chunk(2)
      eps = eu + guidance * (ec - eu)
    lat = sch.step(i, eps.double().numpy(), lat)
    if not concat:
      lat = after(i, lat)
  return torch.from_numpy(np.asarray(lat)).float(), start
