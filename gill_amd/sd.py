"""Stable Diffusion side of the hot path: the object GILL holds as `self.sd_pipe`.

The reference builds `StableDiffusionPipeline.from_pretrained("runwayml/stable-diffusion-v1-5", fp16).to("cuda")`
(gill/models.py:550-551) and calls it as
    self.sd_pipe(prompt_embeds=gen_emb[i:i+8], generator=generator, guidance_scale=..., num_inference_steps=...).images
(gill/models.py:730-731); the loop it runs is restated in-tree at gill/custom_sd.py:567-651.
`GillSDPipeline` keeps that call signature (prompt / negative_prompt / prompt_embeds / negative_prompt_embeds / latents /
generator / guidance_scale / num_inference_steps / num_images_per_prompt / output_type / return_prompts_only) and runs the UNet +
denoise loop in libgill_amd (gill_sd_denoise_ex: csrc/unet.hip) under the pipeline's `scheduler`: PNDM (the default, and what
SD-1.5's scheduler_config.json names), DDIM, DPM-Solver++(2M), Euler or Euler ancestral.

Text prompts (`prompt=`, `negative_prompt=`: _encode_prompt, gill/custom_sd.py:224-373) run through the CLIP text tower in libgill_amd
(gill_clip_text_forward: csrc/cliptext.hip) when the pipeline was built with text-encoder weights (`text_state=` / a model directory
with `text_encoder/`) and a tokenizer; tokenisation itself stays with the CPU tokenizer object.  `truncate_side` and
`return_prompts_only` are the reference's two additions to the stock pipeline (custom_sd.py:90, :268-298, :496, :589-604).  A pipeline
built without text-encoder weights is driven by `prompt_embeds` alone, as `GILL.generate_images` drives it.

`output_type` defaults to "pil" like the reference's (gill/custom_sd.py:491) when the handle holds VAE weights (a UNet-only
handle defaults to "latent"); "latent" (what `GILL.generate_images` passes: the hot path hands latents to the all-gather) returns
the final latents (B,4,64,64) fp32 in `.images`; "pil" / "np" / "pt" run the VAE decoder (gill_vae_decode: csrc/vae.hip, custom_sd.py:385-392, :654-661) and
need the handle to have been built with VAE weights.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import warnings
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Union

import torch

from . import _native as N
from .synth import ClipTextConfig, UNetConfig, VAEConfig


@dataclass
class PipelineOutput:
  images: object                      # latents tensor (B,4,L,L) when output_type == "latent"
  nsfw_content_detected: Optional[List[bool]] = None
  images_u8: Optional[torch.Tensor] = None      # output_type "pil" / "np": the (B,8L,8L,3) uint8 device tensor the images were built from
                                                # (None when a safety checker rewrote them on the host); not a reference field


SAMPLER_KINDS = ("pndm", "ddim", "dpmsolver++", "euler", "euler_ancestral")      # gill_sd_sampler.kind, in order
_SCHEDULER_CLASSES = {"PNDMScheduler": "pndm", "DDIMScheduler": "ddim", "DPMSolverMultistepScheduler": "dpmsolver++",
                      "EulerDiscreteScheduler": "euler", "EulerAncestralDiscreteScheduler": "euler_ancestral"}


@dataclass
class SamplerConfig:
  """Which scheduler the denoise loop runs (the tables are built in libgill_amd: gill_sd_schedule).  steps_offset / set_alpha_to_one are
  PNDM's and DDIM's; `eta` is not here: it is the pipeline call's argument and reaches DDIM only (custom_sd.py:395-403)."""
  kind: str = "pndm"
  steps_offset: int = 1
  set_alpha_to_one: bool = False

  def __post_init__(self):
    if self.kind not in SAMPLER_KINDS:
      raise ValueError(f"unknown scheduler {self.kind!r}: one of {', '.join(SAMPLER_KINDS)}")

  def native(self, eta: float = 0.0) -> "N.gill_sd_sampler":
    return N.gill_sd_sampler(kind=SAMPLER_KINDS.index(self.kind), steps_offset=int(self.steps_offset),
                             set_alpha_to_one=int(bool(self.set_alpha_to_one)), eta=float(eta) if self.kind == "ddim" else 0.0)

  def schedule(self, num_steps: int, v_prediction: bool = False, eta: float = 0.0, start: int = 0):
    """(timesteps [ncalls] float32, init_noise_sigma, rows [ncalls][12] float64 in the layout of include/gill_amd.h) — host only.
    start > 0: the table of an image-to-image loop that begins at sampler step `start` (gill_sd_schedule_from)."""
    ts, sig, rows, _ = self._schedule_from(num_steps, v_prediction, eta, start)
    return ts, sig, rows

  def add_noise_pair(self, num_steps: int, start: int, v_prediction: bool = False, eta: float = 0.0):
    """(a, b) of x_start = a * init_latents + b * noise at the first timestep of the loop that begins at step `start`."""
    return self._schedule_from(num_steps, v_prediction, eta, start)[3]

  def _schedule_from(self, num_steps, v_prediction, eta, start):
    cap = int(num_steps) + 1 if num_steps >= 1 else 1
    ts, sig, rows = (C.c_float * cap)(), C.c_double(), (C.c_double * (cap * N.SD_ROW_DOUBLES))()
    ab = (C.c_double * 2)()
    sp = self.native(eta)
    n = N.lib().gill_sd_schedule_from(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), ts, C.byref(sig), rows, ab)
    if n < 0:
      N.check(n)
    return (torch.tensor(list(ts)[:n], dtype=torch.float32), float(sig.value),
            torch.tensor(list(rows)[:n * N.SD_ROW_DOUBLES], dtype=torch.float64).reshape(n, N.SD_ROW_DOUBLES), (float(ab[0]), float(ab[1])))


def as_sampler_config(scheduler: Union[None, str, SamplerConfig]) -> SamplerConfig:
  if scheduler is None:
    return SamplerConfig()
  if isinstance(scheduler, SamplerConfig):
    return replace(scheduler)
  if isinstance(scheduler, str):
    return SamplerConfig(kind=_SCHEDULER_CLASSES.get(scheduler, scheduler))
  raise TypeError(f"scheduler must be a kind string or a SamplerConfig, got {type(scheduler)}")


def parse_scheduler_config(model_dir: str, scheduler: Union[None, str, SamplerConfig] = None):
  """`scheduler/scheduler_config.json` of a diffusers directory -> (SamplerConfig, prediction_type); needs no weights.  An absent file or
  class name means PNDM; a scheduler class this build does not have warns and runs PNDM; `scheduler=` overrides the file's class (and, given
  as a SamplerConfig, its fields).  A configuration the tables are not built for raises instead of running something else."""
  c = {}
  spath = os.path.join(model_dir, "scheduler", "scheduler_config.json")
  if os.path.exists(spath):
    with open(spath) as f:
      c = json.load(f)
  pred = c.get("prediction_type", "epsilon")
  if c.get("beta_schedule", "scaled_linear") != "scaled_linear":
    raise ValueError(f"{spath}: beta_schedule {c['beta_schedule']!r} is not built (only 'scaled_linear')")
  if isinstance(scheduler, SamplerConfig):
    return replace(scheduler), pred
  name = c.get("_class_name", "PNDMScheduler")
  if scheduler is not None:
    kind = as_sampler_config(scheduler).kind
  elif name in _SCHEDULER_CLASSES:
    kind = _SCHEDULER_CLASSES[name]
  else:
    warnings.warn(f"{spath}: scheduler class {name} is not built into this pipeline; running PNDMScheduler instead "
                  f"(available: {', '.join(_SCHEDULER_CLASSES)})")
    kind = "pndm"
  if kind == "dpmsolver++" and name == "DPMSolverMultistepScheduler":
    if c.get("algorithm_type", "dpmsolver++") != "dpmsolver++" or c.get("solver_order", 2) != 2:
      raise ValueError(f"{spath}: only algorithm_type 'dpmsolver++' with solver_order 2 is built, got "
                       f"{c.get('algorithm_type')!r} / {c.get('solver_order')!r}")
  # (a file that leaves these two out gets SD's values, as every directory did before the file was read for them)
  return SamplerConfig(kind=kind, steps_offset=int(c.get("steps_offset", 1)), set_alpha_to_one=bool(c.get("set_alpha_to_one", False))), pred


class GillSDPipeline:
  def __init__(self, unet_state: Dict[str, torch.Tensor], cfg: UNetConfig, uncond_embeds: Optional[torch.Tensor],
               device: Union[str, torch.device] = "cuda", max_batch: int = 16,
               vae_state: Optional[Dict[str, torch.Tensor]] = None, vae_cfg: Optional[VAEConfig] = None,
               text_state: Optional[Dict[str, torch.Tensor]] = None, text_cfg: Optional[ClipTextConfig] = None, tokenizer=None,
               text_max_batch: Optional[int] = None, scheduler: Union[None, str, SamplerConfig] = None):
    """scheduler: a kind string ("pndm", "ddim", "dpmsolver++", "euler", "euler_ancestral", or the diffusers class name) or a SamplerConfig;
    None is PNDM.  text_state / text_cfg: the CLIP text tower (state-dict names of the published text_encoder files, `text_model.` prefix);
    tokenizer: a Hugging Face style tokenizer object (CLIPTokenizer).  Without text_state nothing is allocated for text and
    `prompt=` raises.  uncond_embeds may be None only when text_state and tokenizer are given: it is then the native encoding of ""."""
    self.cfg = cfg
    self.scheduler = as_sampler_config(scheduler)
    self.truncate_side = "right"        # custom_sd.py:90, :169 ('left': keep the tail of an over-long prompt)
    self.tokenizer = tokenizer
    self.text_encoder = None
    self.device = torch.device(device if str(device) != "cuda" else "cuda:0")
    if self.device.type != "cuda":
      raise N.GillNativeError("GillSDPipeline runs only on an MI355X through libgill_amd")
    self.max_batch = max_batch
    #  the captured denoise loop wants DEBUG_CLR_GRAPH_PACKET_CAPTURE=0, which ROCm reads when HIP initialises: entry points call
    # gill_amd.configure_hip_runtime() first; a caller that did not gets ONE RuntimeWarning here instead of a silent 1.2 % (README "Runtime setting")
    from . import configure_hip_runtime
    configure_hip_runtime(warn=True)
    if text_state is not None:
      from .clip_text import GillClipTextEncoder
      tc = text_cfg or ClipTextConfig.sd15()
      if tc.hidden_size != cfg.cross_attention_dim or tc.max_positions < cfg.ctx_len:
        raise ValueError(f"text encoder (width {tc.hidden_size}, {tc.max_positions} positions) does not fit the UNet's context "
                         f"({cfg.ctx_len} x {cfg.cross_attention_dim})")
      self.text_encoder = GillClipTextEncoder(text_state, tc, self.device, max_batch=text_max_batch or max_batch)
    if uncond_embeds is None:
      if self.text_encoder is None or self.tokenizer is None:
        raise ValueError("uncond_embeds=None needs text-encoder weights and a tokenizer to encode the empty prompt")
      uncond_embeds = self.encode_prompt_ids(self._tokenize([""]), dtype=torch.bfloat16)
    self.uncond_embeds = uncond_embeds.to(self.device, torch.bfloat16).reshape(1, cfg.ctx_len, cfg.cross_attention_dim).contiguous()
    ccfg = N.gill_unet_config(in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                              layers_per_block=cfg.layers_per_block, cross_attention_dim=cfg.cross_attention_dim,
                              num_heads=cfg.num_heads, norm_num_groups=cfg.norm_num_groups,
                              v_prediction=int(cfg.prediction_type == "v_prediction"), fp8_convs=int(cfg.fp8_convs),
                              sample_size=cfg.sample_size, ctx_len=cfg.ctx_len, max_batch=max_batch)
    for i in range(4):
      ccfg.block_out_channels[i] = cfg.block_out_channels[i]
      ccfg.heads_per_level[i] = cfg.heads_per_level[i] if cfg.heads_per_level else 0
    arr, keep = N.make_tensor_table(unet_state, self.device)
    h = C.c_void_p()
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_unet_create(C.byref(h), C.byref(ccfg), arr, len(unet_state)))
    del keep
    self._h = h
    self._vae = None
    self.vae_cfg = None
    self.safety_checker = None          # GillSafetyChecker (custom_sd.py:375-383), loaded by from_pretrained when its files exist
    if vae_state is not None:
      self.load_vae(vae_state, vae_cfg or VAEConfig(latent_size=cfg.sample_size))

  def set_scheduler(self, scheduler: Union[None, str, SamplerConfig]) -> "GillSDPipeline":
    """Swap the sampler of later calls (the handle keeps one captured step per step kernel: nothing is rebuilt)."""
    self.scheduler = as_sampler_config(scheduler)
    return self

  def load_vae(self, vae_state: Dict[str, torch.Tensor], vae_cfg: VAEConfig) -> None:
    """AutoencoderKL (state-dict keys post_quant_conv.* / decoder.*, and encoder.* / quant_conv.* when present: the encoder half
    is built only then — image-to-image needs it) -> gill_vae handle."""
    v = N.gill_vae_config(latent_channels=vae_cfg.latent_channels, out_channels=vae_cfg.out_channels,
                          layers_per_block=vae_cfg.layers_per_block, norm_num_groups=vae_cfg.norm_num_groups,
                          latent_size=vae_cfg.latent_size, scaling_factor=vae_cfg.scaling_factor,
                          max_batch=max(1, self.max_batch // 2))
    for i in range(4):
      v.block_out_channels[i] = vae_cfg.block_out_channels[i]
    dec = {k: t for k, t in vae_state.items() if k.startswith(("decoder.", "post_quant_conv.", "encoder.", "quant_conv."))}
    self._vae_has_encoder = "encoder.conv_in.weight" in dec
    arr, keep = N.make_tensor_table(dec, self.device)
    h = C.c_void_p()
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_vae_create(C.byref(h), C.byref(v), arr, len(dec)))
    del keep
    self._vae, self.vae_cfg = h, vae_cfg

  def decode_latents(self, latents: torch.Tensor, as_uint8: bool = True, both: bool = False):
    """custom_sd.py:385-392 (+ numpy_to_pil's uint8 step): latents (B,4,L,L) -> (B,8L,8L,3) uint8, or with
    as_uint8=False the raw decoder output vae.decode(latents / 0.18215).sample (B,3,8L,8L) fp32; both=True returns
    (fp32, uint8) of the same decode."""
    if self._vae is None:
      raise N.GillNativeError("this pipeline was built without VAE weights (pass vae_state= / use from_pretrained)")
    lat = latents.to(self.device, torch.float32).contiguous()
    B, side = lat.shape[0], 8 * self.vae_cfg.latent_size
    ch = self.vae_cfg.out_channels
    f32 = torch.empty((B, ch, side, side), device=self.device, dtype=torch.float32) if (both or not as_uint8) else None
    u8 = torch.empty((B, side, side, ch), device=self.device, dtype=torch.uint8) if (both or as_uint8) else None
    cap = max(1, self.max_batch // 2)
    with torch.cuda.device(self.device):
      for i in range(0, B, cap):
        b = min(cap, B - i)
        N.check(N.lib().gill_vae_decode(self._vae, N.ptr(lat[i:i + b]), b, None if f32 is None else N.ptr(f32[i:i + b]),
                                        None if u8 is None else N.ptr(u8[i:i + b]), N.current_stream()))
    return (f32, u8) if both else (u8 if as_uint8 else f32)

  def encode_image(self, image, generator=None, sample: bool = True) -> torch.Tensor:
    """vae.encode(image).latent_dist.sample(generator) * scaling_factor (sample=False: the posterior mode) on the device
    (gill_vae_encode: csrc/vae.hip): image in any form `preprocess_image` takes -> latents (B,4,L,L) fp32.  The posterior noise is drawn on
    the CPU generator(s) like every other draw of this pipeline."""
    if self._vae is None or not getattr(self, "_vae_has_encoder", False):
      raise N.GillNativeError("this pipeline was built without VAE encoder weights (encoder.* / quant_conv.* in vae_state= / from_pretrained)")
    return self._encode_preprocessed(self.preprocess_image(image).to(self.device).contiguous(), generator, sample)

  def _encode_preprocessed(self, img: torch.Tensor, generator=None, sample: bool = True) -> torch.Tensor:
    """encode_image behind its host plumbing: img (B,3,8L,8L) fp32 in [-1,1], contiguous, on the device."""
    B, L, lc = img.shape[0], self.vae_cfg.latent_size, self.vae_cfg.latent_channels
    noise = self._randn((B, lc, L, L), generator).to(self.device).contiguous() if sample else None
    out = torch.empty((B, lc, L, L), device=self.device, dtype=torch.float32)
    cap = max(1, self.max_batch // 2)
    with torch.cuda.device(self.device):
      for i in range(0, B, cap):
        b = min(cap, B - i)
        N.check(N.lib().gill_vae_encode(self._vae, N.ptr(img[i:i + b]), b, None if noise is None else N.ptr(noise[i:i + b]),
                                        N.ptr(out[i:i + b]), None, N.current_stream()))
    return out

  def preprocess_image(self, image) -> torch.Tensor:
    """A PIL image, a list of them, a (B,H,W,3) array in [0,1] or a (B,3,H,W) tensor in [-1,1] -> (B,3,8L,8L) fp32 in [-1,1] on the
    host (plumbing).  The handle is built for one size: anything else raises, as `height=` does."""
    import numpy as np
    side = 8 * self.cfg.sample_size
    if isinstance(image, torch.Tensor):
      t = image.detach().to("cpu", torch.float32)
      if t.dim() == 3:
        t = t[None]
    else:
      if not isinstance(image, (list, tuple, np.ndarray)):
        image = [image]
      if not isinstance(image, np.ndarray):
        image = np.stack([np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0 if hasattr(im, "convert") else np.asarray(im, dtype=np.float32)
                          for im in image], 0)
      if image.ndim == 3:
        image = image[None]
      t = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).permute(0, 3, 1, 2) * 2.0 - 1.0
    if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != side or t.shape[3] != side:
      raise ValueError(f"this handle was built for {side}x{side} images, got an image batch of shape {tuple(t.shape)}")
    return t.contiguous()

  def preprocess_mask(self, mask_image) -> torch.Tensor:
    """A PIL image (converted to "L", / 255), a list of them, a (B|1,H,W) or (B|1,H,W,1) array in [0,1] or a (B|1,1,H,W) tensor in [0,1]
    -> (Bm,1,8L,8L) fp32 on the host (plumbing), 1 = repaint.  Binarising (>= 0.5) is the device's work (`prepare_mask`)."""
    import numpy as np
    side = 8 * self.cfg.sample_size
    if isinstance(mask_image, torch.Tensor):
      t = mask_image.detach().to("cpu", torch.float32)
      if t.dim() == 3:
        t = t[:, None]
    else:
      if not isinstance(mask_image, (list, tuple, np.ndarray)):
        mask_image = [mask_image]
      if not isinstance(mask_image, np.ndarray):
        mask_image = np.stack([np.asarray(im.convert("L"), dtype=np.float32) / 255.0 if hasattr(im, "convert") else np.asarray(im, dtype=np.float32)
                               for im in mask_image], 0)
      if mask_image.ndim == 4 and mask_image.shape[-1] == 1:
        mask_image = mask_image[..., 0]
      t = torch.from_numpy(np.ascontiguousarray(mask_image, dtype=np.float32))
      if t.dim() == 3:
        t = t[:, None]
    if t.dim() != 4 or t.shape[1] != 1 or t.shape[2] != side or t.shape[3] != side:
      raise ValueError(f"this handle was built for {side}x{side} images: `mask_image` must be (B|1,1,{side},{side}), got a mask batch of shape "
                       f"{tuple(t.shape)}")
    return t.contiguous()

  def prepare_mask(self, image: torch.Tensor, mask: torch.Tensor):
    """gill_sd_inpaint_prepare on the device: image (B,3,8L,8L) in [-1,1] and mask (B|1,1,8L,8L) in [0,1] (the outputs of `preprocess_image` /
    `preprocess_mask`) -> (masked image (B,3,8L,8L) = image where mask < 0.5 else 0, latent mask (B,1,L,L) in {0,1} = mask[8y,8x] >= 0.5)."""
    from . import ops
    with torch.cuda.device(self.device):
      return ops.sd_inpaint_prepare(image.to(self.device, torch.float32), mask.to(self.device, torch.float32))

  @staticmethod
  def _randn(shape, generator=None) -> torch.Tensor:
    """One unit-variance draw of `shape` (batch first) from the CPU generator, or one sample from each generator of a list."""
    if isinstance(generator, list):
      if len(generator) != shape[0]:
        raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                         f" size of {shape[0]}. Make sure the batch size matches the length of the generators.")
      return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=g.device if g is not None else "cpu", dtype=torch.float32).cpu()
                        for g in generator], 0)
    gdev = generator.device if generator is not None else torch.device("cpu")
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=torch.float32).cpu()

  # ---- construction from a local diffusers directory (no diffusers import: safetensors + json only)
  @classmethod
  def from_pretrained(cls, model_dir: str, uncond_embeds: Optional[torch.Tensor] = None, device="cuda", max_batch: int = 16,
                      tokenizer=None, text_max_batch: Optional[int] = None, scheduler: Union[None, str, SamplerConfig] = None, **_ignored):
    """The sampler comes from `scheduler/scheduler_config.json` (parse_scheduler_config) unless `scheduler=` names one.
    When `text_encoder/model.safetensors` and its `config.json` exist they are loaded into the native text tower, with the
    tokenizer from `tokenizer=` or `tokenizer/` (transformers.CLIPTokenizer: plumbing).  The default negative embedding comes from,
    in this order: `uncond_embeds=`; `uncond_embeds.safetensors`; the native tower on ""; the transformers host forward, only when
    there are no text-encoder weights the native tower can load.  The third arm replaces what used to be that host computation
    (fp32 torch on the CPU): its values agree with it to the rounding of the tower's bf16 GEMM operands, not bit for bit."""
    from safetensors.torch import load_file
    with open(os.path.join(model_dir, "unet", "config.json")) as f:
      c = json.load(f)
    ahd = c["attention_head_dim"]     # diffusers quirk: this field holds the head COUNT(s)
    heads = ahd if isinstance(ahd, int) else ahd[0]
    sampler, pred = parse_scheduler_config(model_dir, scheduler)
    cfg = UNetConfig(in_channels=c["in_channels"], out_channels=c["out_channels"],
                     block_out_channels=tuple(c["block_out_channels"]), layers_per_block=c["layers_per_block"],
                     cross_attention_dim=c["cross_attention_dim"], num_heads=heads,
                     norm_num_groups=c["norm_num_groups"], sample_size=c["sample_size"],
                     heads_per_level=None if isinstance(ahd, int) else tuple(ahd), prediction_type=pred)
    wpath = os.path.join(model_dir, "unet", "diffusion_pytorch_model.safetensors")
    sd = load_file(wpath)
    upath = os.path.join(model_dir, "uncond_embeds.safetensors")
    if uncond_embeds is None and os.path.exists(upath):
      # offline cache of CLIP-text("") (1,77,ctx_dim): what _encode_prompt computes for the empty negative prompt
      # (custom_sd.py:319-357), for machines without the text encoder / tokenizer files
      uncond_embeds = load_file(upath)["uncond_embeds"]
    text_sd, text_cfg = None, None
    tdir = os.path.join(model_dir, "text_encoder")
    if os.path.exists(os.path.join(tdir, "model.safetensors")) and os.path.exists(os.path.join(tdir, "config.json")):
      with open(os.path.join(tdir, "config.json")) as f:
        tc = json.load(f)
      text_cfg = ClipTextConfig(vocab_size=tc["vocab_size"], hidden_size=tc["hidden_size"], num_layers=tc["num_hidden_layers"],
                                num_heads=tc["num_attention_heads"], intermediate_size=tc["intermediate_size"],
                                max_positions=tc.get("max_position_embeddings", 77), hidden_act=tc.get("hidden_act", "quick_gelu"),
                                use_attention_mask=bool(tc.get("use_attention_mask", False)))
      text_sd = load_file(os.path.join(tdir, "model.safetensors"))
      if tokenizer is None and os.path.isdir(os.path.join(model_dir, "tokenizer")):
        from transformers import CLIPTokenizer
        tokenizer = CLIPTokenizer.from_pretrained(os.path.join(model_dir, "tokenizer"))
    if uncond_embeds is None and text_sd is not None and tokenizer is None:
      raise ValueError(f"{model_dir} has text-encoder weights but neither tokenizer= nor a tokenizer/ directory to encode the empty "
                       "negative prompt with; pass one of them, uncond_embeds=, or add uncond_embeds.safetensors")
    if uncond_embeds is None and text_sd is None:
      # CLIP-text("") on the host — only for directories whose text encoder the native tower cannot load (no safetensors file)
      from transformers import CLIPTextModel, CLIPTokenizer
      tok = CLIPTokenizer.from_pretrained(os.path.join(model_dir, "tokenizer"))
      enc = CLIPTextModel.from_pretrained(os.path.join(model_dir, "text_encoder"))
      with torch.no_grad():
        ids = tok([""], padding="max_length", max_length=tok.model_max_length, return_tensors="pt").input_ids
        uncond_embeds = enc(ids)[0]
    vae_sd, vae_cfg = None, None
    vdir = os.path.join(model_dir, "vae")
    if os.path.exists(os.path.join(vdir, "diffusion_pytorch_model.safetensors")):
      with open(os.path.join(vdir, "config.json")) as f:
        vc = json.load(f)
      vae_cfg = VAEConfig(latent_channels=vc["latent_channels"], out_channels=vc["out_channels"],
                          block_out_channels=tuple(vc["block_out_channels"]), layers_per_block=vc["layers_per_block"],
                          norm_num_groups=vc["norm_num_groups"], latent_size=cfg.sample_size)   # scaling 0.18215: custom_sd.py:387
      vae_sd = load_file(os.path.join(vdir, "diffusion_pytorch_model.safetensors"))
    pipe = cls(sd, cfg, uncond_embeds, device, max_batch, vae_state=vae_sd, vae_cfg=vae_cfg, text_state=text_sd, text_cfg=text_cfg,
               tokenizer=tokenizer, text_max_batch=text_max_batch, scheduler=sampler)    # uncond_embeds None here: the native tower encodes ""
    sdir = os.path.join(model_dir, "safety_checker")
    if os.path.exists(os.path.join(sdir, "model.safetensors")):     # the reference's from_pretrained loads it by default
      from .safety import GillSafetyChecker
      from .synth import ClipConfig
      with open(os.path.join(sdir, "config.json")) as f:
        vc = json.load(f).get("vision_config", {})
      ccfg = ClipConfig(image_size=vc.get("image_size", 224), patch_size=vc.get("patch_size", 14), hidden_size=vc.get("hidden_size", 1024),
                        num_layers=vc.get("num_hidden_layers", 24), num_heads=vc.get("num_attention_heads", 16),
                        intermediate_size=vc.get("intermediate_size", 4096))
      pipe.safety_checker = GillSafetyChecker(load_file(os.path.join(sdir, "model.safetensors")), ccfg, pipe.device, max_batch=max(1, max_batch // 2))
    return pipe

  def to(self, device):   # the reference chains .to("cuda")
    assert torch.device(device).type == "cuda"
    return self

  def __del__(self):
    try:
      if getattr(self, "_h", None):
        N.lib().gill_unet_destroy(self._h)
        self._h = None
      if getattr(self, "_vae", None):
        N.lib().gill_vae_destroy(self._vae)
        self._vae = None
      self.text_encoder = None
    except Exception:
      pass

  # ---- low level: one UNet forward (used by parity tests)
  def unet(self, sample: torch.Tensor, timesteps: torch.Tensor, encoder_hidden_states: torch.Tensor) -> torch.Tensor:
    Bx = sample.shape[0]
    sample = sample.to(self.device, torch.float32).contiguous()
    ctx = encoder_hidden_states.to(self.device, torch.bfloat16).contiguous()
    ts = timesteps.detach().float().cpu().reshape(-1)
    if ts.numel() == 1:
      ts = ts.expand(Bx).contiguous()
    tarr = (C.c_float * Bx)(*[float(v) for v in ts])
    if sample.dim() != 4 or sample.shape[1] != self.cfg.in_channels:
      raise ValueError(f"this UNet takes {self.cfg.in_channels} input channels, got a sample of shape {tuple(sample.shape)}")
    out = torch.empty((Bx, self.cfg.out_channels) + tuple(sample.shape[2:]), device=self.device, dtype=torch.float32)
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_unet_forward(self._h, N.ptr(sample), tarr, N.ptr(ctx), Bx, N.ptr(out), N.current_stream()))
    return out

  def prepare_latents(self, batch_size: int, generator=None, latents: Optional[torch.Tensor] = None) -> torch.Tensor:
    """custom_sd.py:458-472.  Latents are drawn on the CPU generator (cuRAND Philox streams of the reference
    notebooks are not reproducible off-NVIDIA); the multiplication by init_noise_sigma (:472) is gill_sd_denoise_ex's first kernel."""
    L = self.cfg.sample_size
    shape = (batch_size, self.cfg.out_channels, L, L)      # the latents (an inpainting UNet's input has more channels)
    if isinstance(generator, list) and len(generator) != batch_size:
      raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                       f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
    if latents is None:
      if isinstance(generator, list):
        latents = torch.cat([torch.randn((1,) + shape[1:], generator=g, device=g.device if g is not None else "cpu",
                                         dtype=torch.float32) for g in generator], 0)
      else:
        gdev = generator.device if generator is not None else torch.device("cpu")
        latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32)
    return latents.to(self.device, torch.float32).contiguous()

  def _step_noise(self, ncalls: int, batch_size: int, generator=None) -> torch.Tensor:
    """The variance noise of a stochastic sampler: one randn per UNet call, in call order, from the generator(s) the latents came from
    (so: after them), as the schedulers' step() draws it; uploaded once."""
    L = self.cfg.sample_size
    one = (self.cfg.out_channels, L, L)
    calls = []
    for _ in range(ncalls):
      if isinstance(generator, list):
        calls.append(torch.cat([torch.randn((1,) + one, generator=g, device=g.device if g is not None else "cpu", dtype=torch.float32).cpu()
                                for g in generator], 0))
      else:
        gdev = generator.device if generator is not None else torch.device("cpu")
        calls.append(torch.randn((batch_size,) + one, generator=generator, device=gdev, dtype=torch.float32).cpu())
    return torch.stack(calls, 0).to(self.device).contiguous()

  # ---- text prompts (custom_sd.py:224-373)
  def encode_prompt_ids(self, ids: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """text_encoder(input_ids)[0] (custom_sd.py:305-309): ids (B,77) from the tokenizer -> (B,77,D) on the device, float32 or
    bfloat16 (the rounding of the former, from the same pass).  Any B: rows go through the tower in chunks of its max_batch."""
    if self.text_encoder is None:
      raise N.GillNativeError("this pipeline was built without text-encoder weights (pass text_state= / use from_pretrained)")
    return self.text_encoder(ids, dtype=dtype)

  def _tokenize(self, texts) -> torch.Tensor:
    return self.tokenizer(texts, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                          return_tensors="pt").input_ids

  def _prompt_ids(self, prompt) -> torch.Tensor:
    """custom_sd.py:266-284: the ids the text encoder sees for `prompt` (str | list[str])."""
    if self.truncate_side not in ("left", "right"):
      raise ValueError(f"truncate_side must be 'left' or 'right', got {self.truncate_side!r}")
    if self.truncate_side == "left":
      # keep the tail: decode the last model_max_length ids in front of the closing token and tokenise those again (:268-275)
      untruncated = self.tokenizer(prompt, padding="longest", return_tensors="pt").input_ids
      mml = self.tokenizer.model_max_length
      if untruncated.shape[-1] > mml:
        prompt = self.tokenizer.batch_decode(untruncated[:, -1 - mml:-1])
    return self._tokenize(prompt)

  def _negative_texts(self, prompt, negative_prompt, batch_size: int) -> List[str]:
    """custom_sd.py:320-337 (the type check compares with the prompt as the caller passed it)."""
    if negative_prompt is None:
      return [""] * batch_size
    if type(prompt) is not type(negative_prompt):
      raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != {type(prompt)}.")
    if isinstance(negative_prompt, str):
      return [negative_prompt]
    if batch_size != len(negative_prompt):
      raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} has batch "
                       f"size {batch_size}. Please make sure that passed `negative_prompt` matches the batch size of `prompt`.")
    return negative_prompt

  @torch.no_grad()
  def __call__(self, prompt=None, height=None, width=None, num_inference_steps: int = 50, guidance_scale: float = 7.5,
               negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0, generator=None,
               latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
               negative_prompt_embeds: Optional[torch.Tensor] = None, output_type: Optional[str] = None, return_dict: bool = True,
               return_prompts_only: bool = False, scheduler: Union[None, str, SamplerConfig] = None, image=None, strength: float = 0.8,
               mask_image=None, **_ignored):
    """scheduler: this call's sampler instead of `self.scheduler`.  eta reaches DDIM only (custom_sd.py:395-403).
    image= / strength=: image-to-image (diffusers' StableDiffusionImg2ImgPipeline): the image is encoded by the VAE encoder, noised to the
    timestep of step `num_inference_steps - min(int(num_inference_steps * strength), num_inference_steps)` and denoised from there
    (gill_sd_denoise_from).  Draw order on the generator(s): posterior noise, add-noise noise, step noise.
    mask_image= (needs image=; any form `preprocess_mask` takes; 1 = repaint, 0 = keep; batch 1 serves every prompt): inpainting
    (gill_sd_inpaint) on the image-to-image loop.  A handle whose UNet takes the latents alone blends the kept region back after every step; a
    handle with a 9-channel inpainting UNet feeds [latents | mask | masked-image latents] instead and cannot be called without a mask.  Draw
    order: the image's posterior noise, the masked image's posterior noise (9-channel handle only), add-noise noise, step noise."""
    if mask_image is not None and image is None:
      raise ValueError("`mask_image` needs `image`: inpainting repaints a region of an image.")
    if image is not None:
      if latents is not None:
        raise ValueError("Cannot forward both `image` and `latents`: image-to-image starts from the encoded image.")
      if not (0.0 <= float(strength) <= 1.0):
        raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
      init_timestep = min(int(num_inference_steps * strength), int(num_inference_steps))
      if init_timestep < 1:
        raise ValueError(f"strength {strength} with {num_inference_steps} steps leaves no step to run")
      if self._vae is None or not getattr(self, "_vae_has_encoder", False):
        raise N.GillNativeError("image= needs the VAE encoder weights (encoder.* / quant_conv.* in vae_state= / from_pretrained)")
    text = getattr(self, "text_encoder", None) is not None
    if prompt is not None and not text:
      raise ValueError("GillSDPipeline is driven by prompt_embeds (gill/models.py:730); text prompts need the CLIP text "
                       "encoder, which is outside this path")
    # diffusers' check_inputs (custom_sd.py:572-574)
    if prompt is not None and prompt_embeds is not None:
      raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to only forward "
                       "one of the two.")
    if prompt is None and prompt_embeds is None:
      raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
    if prompt is not None and not isinstance(prompt, (str, list)):
      raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
    if text and negative_prompt is not None and negative_prompt_embeds is not None:
      raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`: "
                       f"{negative_prompt_embeds}. Please make sure to only forward one of the two.")
    if prompt is not None and self.tokenizer is None:
      raise ValueError("text prompts need a tokenizer (tokenizer= / a `tokenizer/` directory next to the weights)")
    # custom_sd.py:588-591
    do_cfg = guidance_scale > 1.0 and not return_prompts_only
    neg_texts = None
    if text and do_cfg and negative_prompt_embeds is None and (prompt is not None or negative_prompt is not None):
      neg_texts = self._negative_texts(prompt, negative_prompt, 1 if isinstance(prompt, str) else len(prompt or ()))
    if return_prompts_only:      # :589-604: the prompt embeddings alone, no negative half, float32 for the caller's .cpu().numpy()
      emb = self.encode_prompt_ids(self._prompt_ids(prompt)) if prompt is not None else prompt_embeds.to(torch.float32)
      return emb.repeat_interleave(num_images_per_prompt, dim=0) if num_images_per_prompt != 1 else emb
    if prompt is not None:
      # the tower writes the bf16 context gill_sd_denoise reads: nothing visits the host between the two
      prompt_embeds = self.encode_prompt_ids(self._prompt_ids(prompt), dtype=torch.bfloat16)
      if neg_texts is not None:
        # negative_prompt=None: "" for every prompt (:321-322) — identical rows, so one is encoded and shared by the batch
        negative_prompt_embeds = self.encode_prompt_ids(self._tokenize([""] if negative_prompt is None else neg_texts),
                                                        dtype=torch.bfloat16)
    if output_type is None:
      # the reference's default is "pil" (gill/custom_sd.py:491: `.images` is a list of PIL images); a handle built WITHOUT VAE
      # weights (UNet-only parity rigs) can only return latents
      output_type = "pil" if self._vae is not None else "latent"
    concat = self.cfg.in_channels != self.cfg.out_channels
    if concat and self.cfg.in_channels != 2 * self.cfg.out_channels + 1:
      raise ValueError(f"a UNet with {self.cfg.in_channels} input and {self.cfg.out_channels} output channels is neither a text-to-image "
                       "nor an inpainting UNet")
    if concat and mask_image is None:
      raise ValueError(f"this handle's UNet takes {self.cfg.in_channels} channels ([latents | mask | masked-image latents]): pass `image` and "
                       "`mask_image`")
    L = self.cfg.sample_size
    if (height is not None and height != L * 8) or (width is not None and width != L * 8):
      raise ValueError(f"this handle was built for {L * 8}x{L * 8} images")
    if output_type not in ("latent", "pil", "np", "pt"):
      raise ValueError(f"unknown output_type {output_type!r}")
    if output_type != "latent" and self._vae is None:
      raise N.GillNativeError("output_type != 'latent' needs the VAE decoder weights (vae_state= / from_pretrained)")
    cond = prompt_embeds.to(self.device, torch.bfloat16)
    if num_images_per_prompt != 1:
      cond = cond.repeat_interleave(num_images_per_prompt, dim=0)
    cond = cond.contiguous()
    B = cond.shape[0]
    if negative_prompt_embeds is None:
      uncond = self.uncond_embeds
    else:      # custom_sd.py:359-369: one negative embedding per prompt (or one for all), repeated per image
      uncond = negative_prompt_embeds.to(self.device, torch.bfloat16)
      if uncond.shape[0] != 1 and num_images_per_prompt != 1:
        uncond = uncond.repeat_interleave(num_images_per_prompt, dim=0)
      uncond = uncond.contiguous()
      if uncond.shape[0] not in (1, B) or tuple(uncond.shape[1:]) != tuple(cond.shape[1:]):
        raise ValueError(f"`negative_prompt_embeds` must have the shape of `prompt_embeds` (or batch 1): got "
                         f"{tuple(negative_prompt_embeds.shape)} for prompt_embeds {tuple(prompt_embeds.shape)}")
    sampler = self.scheduler if scheduler is None else as_sampler_config(scheduler)
    _, _, rows = sampler.schedule(int(num_inference_steps), self.cfg.prediction_type == "v_prediction", eta)   # (raises on bad arguments)
    sp = sampler.native(eta)
    if image is not None:
      start = int(num_inference_steps) - init_timestep
      _, _, rows = sampler.schedule(int(num_inference_steps), self.cfg.prediction_type == "v_prediction", eta, start=start)
      img = self.preprocess_image(image)
      if img.shape[0] != B:
        if B % img.shape[0] != 0:
          raise ValueError(f"Cannot duplicate `image` of batch size {img.shape[0]} to {B} text prompts.")
        img = img.repeat(B // img.shape[0], 1, 1, 1)
      lmask = xm = None
      if mask_image is not None:
        side = 8 * self.cfg.sample_size
        mk = self.preprocess_mask(mask_image)
        if mk.shape[0] not in (1, B):
          raise ValueError(f"`mask_image` must be (B|1,1,{side},{side}) with B = {B} prompts, got a mask batch of shape {tuple(mk.shape)}")
        masked, lmask = self.prepare_mask(img, mk)
      x0 = self.encode_image(img, generator)                     # draw 1: the posterior's noise
      if concat:
        xm = self._encode_preprocessed(masked.contiguous(), generator)      # (9-channel handle) the masked image's posterior noise
      L = self.cfg.sample_size
      z0 = self._randn((B, self.cfg.out_channels, L, L), generator).to(self.device).contiguous()      # draw 2: add_noise
      noise = self._step_noise(rows.shape[0], B, generator) if bool((rows[:, 11] != 0).any()) else None    # draw 3
      out = torch.empty_like(x0)
      with torch.cuda.device(self.device):
        if lmask is not None:
          from . import ops
          out = ops.sd_inpaint(self._h, sp, cond, uncond, start, x0, z0, lmask, xm, int(num_inference_steps), float(guidance_scale), noise)
        else:
          N.check(N.lib().gill_sd_denoise_from(self._h, C.byref(sp), N.ptr(cond), N.ptr(uncond), int(uncond.shape[0]), start, N.ptr(x0),
                                             N.ptr(z0), B, int(num_inference_steps), float(guidance_scale), N.ptr(out),
                                             None if noise is None else N.ptr(noise), N.current_stream()))
    else:
      lat0 = self.prepare_latents(B, generator, latents)
      noise = self._step_noise(rows.shape[0], B, generator) if bool((rows[:, 11] != 0).any()) else None
      out = torch.empty_like(lat0)
      with torch.cuda.device(self.device):
        N.check(N.lib().gill_sd_denoise_ex(self._h, C.byref(sp), N.ptr(cond), N.ptr(uncond), int(uncond.shape[0]), N.ptr(lat0), B,
                                           int(num_inference_steps), float(guidance_scale), N.ptr(out),
                                           None if noise is None else N.ptr(noise), N.current_stream()))
    has_nsfw, dev_u8 = None, None
    if output_type in ("pil", "np"):      # custom_sd.py:654-661: decode_latents -> run_safety_checker -> numpy_to_pil
      from PIL import Image
      dev_u8 = self.decode_latents(out, as_uint8=True)
      u8 = dev_u8.cpu().numpy()
      n = N.lib().gill_coop_timeouts()      # (the copy above synchronised: the loop's give-up count is final — include/gill_amd.h "Exclusive-device contract")
      if n != 0:
        raise N.GillNativeError(f"{n} in-kernel GroupNorm finish(es) of the denoise loop timed out and NaN-poisoned the latents: the GPU is shared with "
                                "another stream or process that also runs waiting workgroups; give this pipeline the device, or set GILL_GEMM_COOP=0")
      if self.safety_checker is not None:
        img01, has_nsfw = self.safety_checker(u8.astype("float32") / 255.0, [Image.fromarray(im) for im in u8])
        u8 = (img01 * 255).round().astype("uint8")
        dev_u8 = None
      out = [Image.fromarray(im) for im in u8] if output_type == "pil" else u8.astype("float32") / 255.0
    elif output_type == "pt":
      out = self.decode_latents(out, as_uint8=False)
    if not return_dict:
      return (out, has_nsfw)
    return PipelineOutput(images=out, nsfw_content_detected=has_nsfw, images_u8=dev_u8)
