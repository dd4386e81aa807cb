"""The bar of tests/test_vae_encoder_gpu.py, measured on the CPU: how far bf16 STORAGE alone moves the encoder's moments.

Compares the fp32 restatement of the encoder (tests/vae_encoder_util.py) with the same restatement after rounding every tensor the engine
stores as bf16 (conv, GroupNorm and attention outputs, the im2col pixels) to bf16 — same bf16-rounded synthetic weights, same images as the
test.  Prints relative L2 and 1 - cosine for the mean and the logvar halves; the test's bar is twice these figures (the factor covers the
MFMA's accumulation order and __expf).  `--write` records them in profiles/vae_encoder.md.

    python tools/vae_encoder_tolerance.py [--write]
"""
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vae_encoder_util as V  # noqa: E402
from gill_amd import synth  # noqa: E402


def case():
  """(cfg, bf16-rounded weights, images) of the parity test."""
  cfg = synth.VAEConfig.tiny(16)
  sd = {k: v.bfloat16().float() for k, v in synth.vae_encoder_state_dict(cfg, seed=5).items()}
  return cfg, sd, V.test_images(3, 8 * cfg.latent_size, seed=11)


def measure():
  cfg, sd, img = case()
  with torch.no_grad():
    ref = V.encoder_moments(sd, img, cfg.block_out_channels, cfg.norm_num_groups)
    low = V.encoder_moments(sd, img, cfg.block_out_channels, cfg.norm_num_groups, q=V.bf16_round)
  out = {}
  for name, a, b in zip(("mean", "logvar"), low.chunk(2, 1), ref.chunk(2, 1)):
    rel = ((a - b).norm() / b.norm()).item()
    cos = torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()
    out[name] = (rel, 1.0 - cos)
  return out


if __name__ == "__main__":
  torch.set_num_threads(synth.host_cores())
  m = measure()
  lines = [f"| {k} | {v[0]:.3e} | {v[1]:.3e} |" for k, v in m.items()]
  print("\n".join(lines))
  if "--write" in sys.argv:
    path = os.path.join(ROOT, "profiles", "vae_encoder.md")
    text = open(path).read() if os.path.exists(path) else "# VAE encoder\n"
    block = ("<!-- tolerance -->\n## bf16 storage distance (tools/vae_encoder_tolerance.py, CPU)\n\n"
             "fp32 restatement against the restatement with bf16-rounded stored activations; VAEConfig.tiny(16), 128x128, B = 3.\n\n"
             "| half | rel L2 | 1 - cos |\n|---|---|---|\n" + "\n".join(lines) + "\n<!-- /tolerance -->\n")
    if "<!-- tolerance -->" in text:
      text = re.sub(r"<!-- tolerance -->.*?<!-- /tolerance -->\n", lambda _: block, text, flags=re.S)
    else:
      text = text.rstrip("\n") + "\n\n" + block
    open(path, "w").write(text)
