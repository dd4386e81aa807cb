"""Inpainting through the pipeline (image= / mask_image=) on the rig of tests/test_img2img_gpu.py: tiny UNet + tiny VAE against the CPU driver
of tests/inpaint_util.py (fp32 encoder restatement, float64 add-noise, the fp32 oracle UNet under the float64 scheduler, the blend in float64),
same generator seeds; the bar of the tiny loop tests (rel-L2 < 8e-2).  Blend mode on the 4-channel handle, concat mode on a 9-channel one."""
import ctypes as C
import dataclasses

import pytest
import torch

import inpaint_util as I
import vae_encoder_util as V
from gill_amd import synth

pytestmark = pytest.mark.gpu


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def _mask(B, side=128, seed=41):
  """Per-sample random rectangles of ones on zeros, on the host: (B,1,side,side) in {0,1}, about half repainted."""
  g = torch.Generator().manual_seed(seed)
  m = torch.zeros(B, 1, side, side)
  for b in range(B):
    y0, x0 = (int(v) for v in torch.randint(0, side // 4, (2,), generator=g))
    m[b, 0, y0:y0 + 3 * side // 4, x0:x0 + 5 * side // 8 + 3] = 1.0      # edges off the 8-pixel grid
  return m


def _vae(vcfg):
  return _bfw({**synth.vae_decoder_state_dict(vcfg, seed=5), **synth.vae_encoder_state_dict(vcfg, seed=5)})


@pytest.fixture(scope="module")
def rig(cuda):
  from gill_amd.sd import GillSDPipeline
  cfg = synth.UNetConfig.tiny(16)
  usd = _bfw(synth.unet_state_dict(cfg, seed=3))
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=3).bfloat16().float()
  vcfg = synth.VAEConfig.tiny(16)
  vsd = _vae(vcfg)
  pipe = GillSDPipeline(usd, cfg, uncond, cuda, max_batch=8, vae_state=vsd, vae_cfg=vcfg)
  cond = synth.normal("i2i_cond", (2, 77, cfg.cross_attention_dim), 4).bfloat16().float()
  img = V.test_images(2, 128, seed=21)
  return cfg, usd, uncond, vcfg, vsd, pipe, cond, img


@pytest.fixture(scope="module")
def rig9(cuda):
  from gill_amd.sd import GillSDPipeline
  cfg = dataclasses.replace(synth.UNetConfig.tiny(16), in_channels=9)
  usd = _bfw(synth.unet_state_dict(cfg, seed=6))
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=3).bfloat16().float()
  vcfg = synth.VAEConfig.tiny(16)
  vsd = _vae(vcfg)
  pipe = GillSDPipeline(usd, cfg, uncond, cuda, max_batch=8, vae_state=vsd, vae_cfg=vcfg)
  cond = synth.normal("i2i_cond", (2, 77, cfg.cross_attention_dim), 4).bfloat16().float()
  img = V.test_images(2, 128, seed=21)
  return cfg, usd, uncond, vcfg, vsd, pipe, cond, img


KW = dict(strength=0.5, num_inference_steps=6, guidance_scale=7.5, output_type="latent")


@pytest.mark.parametrize("kind", ["ddim", "pndm"])
def test_blend_tiny_vs_cpu_driver(rig, kind):
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  mask = _mask(2)
  got = pipe(prompt_embeds=cond, image=img, mask_image=mask, scheduler=kind, generator=torch.Generator().manual_seed(77), **KW).images.float().cpu()
  with torch.no_grad():
    ref, start = I.inpaint_ref(usd, cfg, vsd, vcfg, cond, uncond, img, mask, kind, 6, 0.5, 7.5, 77)
  rel = ((got - ref).norm() / ref.norm()).item()
  lm = I.prepare_ref(img, mask)[1].expand(-1, 4, -1, -1) > 0
  rel_in = ((got - ref)[lm].norm() / ref[lm].norm()).item()
  print(f"[inpaint blend tiny {kind}] start={start} rel_l2={rel:.3e} (repainted region alone {rel_in:.3e})")
  assert start == 3 and got.shape == ref.shape and rel < 8e-2


def test_blend_mask_extremes(rig):
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  run = lambda **kw: pipe(prompt_embeds=cond, image=img, scheduler="ddim", generator=torch.Generator().manual_seed(11), **KW, **kw).images  # noqa: E731
  plain = run()
  assert torch.equal(run(mask_image=torch.ones(2, 1, 128, 128)), plain)           # repaint everything: image-to-image, bit for bit
  assert torch.equal(run(mask_image=torch.ones(1, 1, 128, 128)), plain)           # one mask for every prompt
  x0 = pipe.encode_image(img, torch.Generator().manual_seed(11))
  assert torch.equal(run(mask_image=torch.zeros(2, 1, 128, 128)), x0)             # keep everything: the encoded image, bit for bit
  assert not torch.equal(plain, x0)


def test_unet_forward_9_channels_vs_oracle(rig9):
  from oracle import unet_ref
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig9
  x = synth.normal("unet9_x", (3, 9, 16, 16), 9)
  ctx = synth.normal("unet_ctx", (3, 77, cfg.cross_attention_dim), 9).bfloat16().float()
  t = torch.tensor([981.0, 501.0, 1.0])
  ref = unet_ref.unet_forward(usd, x, t, ctx, cfg.block_out_channels, cfg.num_heads, cfg.norm_num_groups)
  got = pipe.unet(x, t, ctx).float().cpu()
  rel = ((got - ref).norm() / ref.norm()).item()
  cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
  print(f"[unet tiny 9-channel forward] rel_l2={rel:.3e} cos={cos:.6f}")
  assert tuple(got.shape) == (3, 4, 16, 16) and got.shape == ref.shape
  assert rel < 5e-2 and cos > 0.998      # the bar of test_unet_forward_tiny_vs_oracle: only the first layer's K changes


def test_concat_tiny_vs_cpu_driver(rig9):
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig9
  mask = _mask(2, seed=43)
  got = pipe(prompt_embeds=cond, image=img, mask_image=mask, scheduler="ddim", generator=torch.Generator().manual_seed(78), **KW).images.float().cpu()
  with torch.no_grad():
    ref, start = I.inpaint_ref(usd, cfg, vsd, vcfg, cond, uncond, img, mask, "ddim", 6, 0.5, 7.5, 78)
  rel = ((got - ref).norm() / ref.norm()).item()
  print(f"[inpaint concat tiny ddim] start={start} rel_l2={rel:.3e}")
  assert start == 3 and tuple(got.shape) == (2, 4, 16, 16) and got.shape == ref.shape and rel < 8e-2


def test_concat_handle_refuses_calls_without_a_mask(rig9):
  from gill_amd import _native as N
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig9
  with pytest.raises(ValueError, match="mask_image"):
    pipe(prompt_embeds=cond, **KW)
  with pytest.raises(ValueError, match="mask_image"):
    pipe(prompt_embeds=cond, image=img, **KW)
  sp = pipe.scheduler.native(0.0)
  c = cond.to(pipe.device, torch.bfloat16).contiguous()
  lat = torch.zeros(2, 4, 16, 16, device=pipe.device)
  out = torch.empty_like(lat)
  with pytest.raises(N.GillNativeError, match="gill_sd_inpaint"):
    N.check(N.lib().gill_sd_denoise_ex(pipe._h, C.byref(sp), N.ptr(c), N.ptr(pipe.uncond_embeds), 1, N.ptr(lat), 2, 6, 7.5, N.ptr(out), None,
                                       N.current_stream()))
  from gill_amd import ops
  lm = torch.ones(2, 1, 16, 16, device=pipe.device)
  with pytest.raises(N.GillNativeError, match="blend mode"):       # no masked_latents on the 9-channel handle
    ops.sd_inpaint(pipe._h, "ddim", c, pipe.uncond_embeds, 3, lat, lat, lm, None, 6, 7.5)


def test_argument_errors(rig):
  from gill_amd import _native as N
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  kw = dict(prompt_embeds=cond, **KW)
  with pytest.raises(ValueError, match="needs `image`"):
    pipe(mask_image=torch.ones(2, 1, 128, 128), **kw)
  with pytest.raises(ValueError, match="128x128"):
    pipe(image=img, mask_image=torch.ones(2, 1, 64, 64), **kw)
  with pytest.raises(ValueError, match="128,128"):
    pipe(image=img, mask_image=torch.ones(3, 1, 128, 128), **kw)       # neither 1 nor B
  # masked_latents on a 4-channel handle, through ops
  from gill_amd import ops
  c = cond.to(pipe.device, torch.bfloat16).contiguous()
  lat = torch.zeros(2, 4, 16, 16, device=pipe.device)
  lm = torch.ones(2, 1, 16, 16, device=pipe.device)
  with pytest.raises(N.GillNativeError, match="concat mode"):
    ops.sd_inpaint(pipe._h, "ddim", c, pipe.uncond_embeds, 3, lat, lat, lm, lat, 6, 7.5)
  with pytest.raises(ValueError, match="latent_mask"):
    ops.sd_inpaint(pipe._h, "ddim", c, pipe.uncond_embeds, 3, lat, lat, lm[:, :, :8], None, 6, 7.5)
