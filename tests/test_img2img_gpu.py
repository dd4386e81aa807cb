"""Image-to-image through the pipeline (image= / strength=): tiny UNet + tiny VAE against the CPU driver of tests/vae_encoder_util.py (fp32
encoder restatement, float64 add-noise, the fp32 oracle UNet under the float64 scheduler from the start index), same generator seeds; the
bar of the tiny text-to-image loop tests (rel-L2 < 8e-2)."""
import numpy as np
import pytest
import torch

import vae_encoder_util as V
from gill_amd import synth

pytestmark = pytest.mark.gpu


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def rig(cuda):
  from gill_amd.sd import GillSDPipeline
  cfg = synth.UNetConfig.tiny(16)
  usd = _bfw(synth.unet_state_dict(cfg, seed=3))
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=3).bfloat16().float()
  vcfg = synth.VAEConfig.tiny(16)
  vsd = _bfw({**synth.vae_decoder_state_dict(vcfg, seed=5), **synth.vae_encoder_state_dict(vcfg, seed=5)})
  pipe = GillSDPipeline(usd, cfg, uncond, cuda, max_batch=8, vae_state=vsd, vae_cfg=vcfg)
  cond = synth.normal("i2i_cond", (2, 77, cfg.cross_attention_dim), 4).bfloat16().float()
  img = V.test_images(2, 128, seed=21)
  return cfg, usd, uncond, vcfg, vsd, pipe, cond, img


@pytest.mark.parametrize("kind", ["ddim", "pndm"])
def test_img2img_tiny_vs_cpu_driver(rig, kind):
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  got = pipe(prompt_embeds=cond, image=img, strength=0.5, num_inference_steps=6, guidance_scale=7.5, output_type="latent", scheduler=kind,
             generator=torch.Generator().manual_seed(77)).images.float().cpu()
  with torch.no_grad():
    ref, start = V.img2img_ref(usd, cfg, vsd, vcfg, cond, uncond, img, kind, 6, 0.5, 7.5, 77)
  rel = ((got - ref).norm() / ref.norm()).item()
  print(f"[img2img tiny {kind}] start={start} rel_l2={rel:.3e}")
  assert start == 3 and got.shape == ref.shape and rel < 8e-2


def test_one_image_is_repeated_over_the_prompts(rig):
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  run = lambda im: pipe(prompt_embeds=cond, image=im, strength=0.5, num_inference_steps=4, output_type="latent", scheduler="ddim",  # noqa: E731
                        generator=torch.Generator().manual_seed(5)).images
  assert torch.equal(run(img[:1]), run(img[:1].repeat(2, 1, 1, 1)))
  arr = ((img[:1] + 1) / 2).permute(0, 2, 3, 1).numpy()       # (B,H,W,3) in [0,1]: the same image in the array form (host plumbing)
  assert torch.allclose(pipe.preprocess_image(arr), img[:1], atol=1e-6) and torch.isfinite(run(arr)).all()


def test_full_strength_starts_from_the_noised_image_not_from_noise(rig):
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  kw = dict(prompt_embeds=cond, num_inference_steps=4, output_type="latent", scheduler="ddim", guidance_scale=7.5)
  got = pipe(image=img, strength=1.0, generator=torch.Generator().manual_seed(9), **kw).images.float().cpu()
  with torch.no_grad():
    ref, start = V.img2img_ref(usd, cfg, vsd, vcfg, cond, uncond, img, "ddim", 4, 1.0, 7.5, 9)
  assert start == 0 and ((got - ref).norm() / ref.norm()).item() < 8e-2
  # text-to-image from the add-noise draw alone differs: the image's share a * x0 is in the start
  g = torch.Generator().manual_seed(9)
  torch.randn((2, 4, 16, 16), generator=g)
  z0 = torch.randn((2, 4, 16, 16), generator=g)
  t2i = pipe(latents=z0, **kw).images.float().cpu()
  assert ((got - t2i).norm() / t2i.norm()).item() > 1e-3


def test_argument_errors(rig, cuda):
  from gill_amd import _native as N
  from gill_amd.sd import GillSDPipeline
  cfg, usd, uncond, vcfg, vsd, pipe, cond, img = rig
  kw = dict(prompt_embeds=cond, num_inference_steps=6, output_type="latent")
  for s in (-0.1, 1.5):
    with pytest.raises(ValueError, match="strength"):
      pipe(image=img, strength=s, **kw)
  with pytest.raises(ValueError, match="no step"):
    pipe(image=img, strength=0.1, **kw)
  with pytest.raises(ValueError, match="latents"):
    pipe(image=img, latents=torch.zeros(2, 4, 16, 16), **kw)
  with pytest.raises(ValueError, match="128x128"):
    pipe(image=torch.zeros(2, 3, 64, 64), **kw)
  dec_only = GillSDPipeline(usd, cfg, uncond, cuda, max_batch=4, vae_state=_bfw(synth.vae_decoder_state_dict(vcfg, seed=5)), vae_cfg=vcfg)
  with pytest.raises(N.GillNativeError, match="encoder"):
    dec_only(image=img, **kw)
  with pytest.raises(N.GillNativeError, match="encoder"):
    dec_only.encode_image(img)
  lat = pipe.encode_image(img, sample=False)
  assert tuple(lat.shape) == (2, 4, 16, 16) and torch.isfinite(lat).all()
