"""The VAE encoder half (gill_vae_encode: csrc/vae.hip) against the fp32 restatement of tests/vae_encoder_util.py."""
import ctypes as C

import pytest
import torch

import vae_encoder_util as V
from gill_amd import synth

pytestmark = pytest.mark.gpu

# tools/vae_encoder_tolerance.py (CPU; these weights and images): the fp32 restatement against itself with bf16-rounded stored activations
#   mean: rel L2 1.176e-02, 1 - cos 6.860e-05;  logvar: rel L2 1.260e-02, 1 - cos 7.915e-05  (profiles/vae_encoder.md)
# The bars are twice those figures: the factor covers the MFMA's accumulation order and __expf.
STORAGE = {"mean": (1.176e-2, 6.860e-5), "logvar": (1.260e-2, 7.915e-5)}


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def _handle(sd, cfg, dev, max_batch=4):
  from gill_amd import _native as N
  v = N.gill_vae_config(latent_channels=cfg.latent_channels, out_channels=cfg.out_channels, layers_per_block=cfg.layers_per_block,
                        norm_num_groups=cfg.norm_num_groups, latent_size=cfg.latent_size, scaling_factor=cfg.scaling_factor, max_batch=max_batch)
  for i in range(4):
    v.block_out_channels[i] = cfg.block_out_channels[i]
  arr, keep = N.make_tensor_table(sd, dev)
  h = C.c_void_p()
  N.check(N.lib().gill_vae_create(C.byref(h), C.byref(v), arr, len(sd)))
  del keep
  return h


def _encode(h, cfg, img, noise, want_moments=True):
  from gill_amd import _native as N
  B, L, lc = img.shape[0], cfg.latent_size, cfg.latent_channels
  z = torch.empty((B, lc, L, L), device=img.device)
  mom = torch.empty((B, 2 * lc, L, L), device=img.device) if want_moments else None
  N.check(N.lib().gill_vae_encode(h, N.ptr(img), B, N.ptr(noise), N.ptr(z), N.ptr(mom), N.current_stream()))
  torch.cuda.synchronize()
  return z, mom


@pytest.fixture(scope="module")
def rig(cuda):
  from gill_amd import _native as N
  cfg = synth.VAEConfig.tiny(16)
  enc = _bfw(synth.vae_encoder_state_dict(cfg, seed=5))
  dec = _bfw(synth.vae_decoder_state_dict(cfg, seed=5))
  img = V.test_images(3, 8 * cfg.latent_size, seed=11)
  with torch.no_grad():
    ref = V.encoder_moments(enc, img, cfg.block_out_channels, cfg.norm_num_groups)
  both = _handle({**dec, **enc}, cfg, cuda)
  only = _handle(dec, cfg, cuda)
  yield cfg, enc, dec, img, ref, both, only
  N.lib().gill_vae_destroy(both)
  N.lib().gill_vae_destroy(only)


def test_moments_match_the_fp32_restatement(rig, cuda):
  """Measured bf16-storage distance (CPU): mean rel L2 1.176e-02 / 1 - cos 6.860e-05, logvar 1.260e-02 / 7.915e-05; the bars are twice that."""
  cfg, enc, dec, img, ref, both, only = rig
  _, mom = _encode(both, cfg, img.to(cuda), None)
  mom = mom.cpu()
  for name, got, want in zip(("mean", "logvar"), mom.chunk(2, 1), ref.chunk(2, 1)):
    rel = ((got - want).norm() / want.norm()).item()
    cos = torch.nn.functional.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    print(f"[vae encoder {name}] rel_l2={rel:.3e} 1-cos={1 - cos:.3e} (bars {2 * STORAGE[name][0]:.3e}, {2 * STORAGE[name][1]:.3e})")
    assert rel <= 2 * STORAGE[name][0] and 1 - cos <= 2 * STORAGE[name][1], (name, rel, 1 - cos)


def _ulp_close(got, want, ulps=8):
  """|got - want| within `ulps` fp32 ulp of the larger magnitude (a product, a sum, __expf against exp: a few roundings)."""
  tol = ulps * 2.0 ** -23 * torch.maximum(got.abs(), want.abs()).clamp_min(2.0 ** -100)
  return bool(((got - want).abs() <= tol).all())


def test_latents_follow_from_the_devices_own_moments(rig, cuda):
  cfg, enc, dec, img, ref, both, only = rig
  noise = torch.randn((3, cfg.latent_channels, cfg.latent_size, cfg.latent_size), generator=torch.Generator().manual_seed(3))
  z, mom = _encode(both, cfg, img.to(cuda), noise.to(cuda))
  mean, logvar = mom.double().cpu().chunk(2, 1)
  # __expf is not correctly rounded: allow its documented 2 ulp + the ulp of exp's argument scaled by |0.5 logvar| (< 16) on the noise term
  want = cfg.scaling_factor * (mean + torch.exp(0.5 * logvar) * noise.double())
  term = (cfg.scaling_factor * torch.exp(0.5 * logvar) * noise.double()).abs()
  tol = 8 * 2.0 ** -23 * (want.abs() + (1 + (0.5 * logvar).abs()) * term)
  assert bool(((z.double().cpu() - want).abs() <= tol).all())
  z0, mom0 = _encode(both, cfg, img.to(cuda), None)
  assert torch.equal(mom0, mom)
  assert _ulp_close(z0.cpu(), (cfg.scaling_factor * mom0.cpu().chunk(2, 1)[0].double()).float(), 2)
  z1, none = _encode(both, cfg, img.to(cuda), None, want_moments=False)      # moments_out may be NULL
  assert none is None and torch.equal(z1, z0)


def test_logvar_is_clamped(cuda):
  cfg = synth.VAEConfig.tiny(16)
  enc = _bfw(synth.vae_encoder_state_dict(cfg, seed=5))
  enc["quant_conv.bias"] = enc["quant_conv.bias"].clone()
  enc["quant_conv.bias"][cfg.latent_channels + 1] = 100.0       # pushes logvar channel 1 past 20
  enc["quant_conv.bias"][cfg.latent_channels + 2] = -100.0      # and channel 2 below -30
  from gill_amd import _native as N
  h = _handle({**_bfw(synth.vae_decoder_state_dict(cfg, seed=5)), **enc}, cfg, cuda, max_batch=1)
  try:
    _, mom = _encode(h, cfg, V.test_images(1, 128, seed=11).to(cuda), None)
  finally:
    N.lib().gill_vae_destroy(h)
  lv = mom[:, cfg.latent_channels:]
  assert bool((lv[:, 1] == 20.0).all()) and bool((lv[:, 2] == -30.0).all()) and bool((lv[:, 0].abs() < 20.0).all())


def test_decoder_only_handle_refuses_encode_and_decodes_the_same_bits(rig, cuda):
  from gill_amd import _native as N
  cfg, enc, dec, img, ref, both, only = rig
  with pytest.raises(N.GillNativeError, match="encoder"):
    _encode(only, cfg, img.to(cuda), None)
  lat = synth.initial_latents(2, 4, cfg.latent_size, seed=9).to(cuda)
  outs = []
  for h in (only, both):
    o = torch.empty((2, 3, 8 * cfg.latent_size, 8 * cfg.latent_size), device=cuda)
    N.check(N.lib().gill_vae_decode(h, N.ptr(lat), 2, N.ptr(o), None, N.current_stream()))
    torch.cuda.synchronize()
    outs.append(o)
  assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
  with pytest.raises(N.GillNativeError, match="max_batch"):
    _encode(both, cfg, V.test_images(5, 128, seed=1).to(cuda), None)


def test_round_trip_plumbing(rig, cuda):
  """decode(encode(x, sample=False)): shapes and finite values only — synthetic weights make no autoencoder."""
  from gill_amd import _native as N
  cfg, enc, dec, img, ref, both, only = rig
  z, _ = _encode(both, cfg, img.to(cuda), None)
  out = torch.empty((3, 3, 8 * cfg.latent_size, 8 * cfg.latent_size), device=cuda)
  N.check(N.lib().gill_vae_decode(both, N.ptr(z), 3, N.ptr(out), None, N.current_stream()))
  torch.cuda.synchronize()
  assert tuple(z.shape) == (3, 4, 16, 16) and torch.isfinite(z).all() and torch.isfinite(out).all()
