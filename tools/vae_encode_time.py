"""HIP-event time of gill_vae_encode at SD-1.5 size (512x512 pixels -> 64x64 latents), B = 1 and 4, beside gill_vae_decode from the same run.
Synthetic weights (timing does not depend on the values).  `--write` records the numbers in profiles/vae_encoder.md; there is no bar.

    python tools/vae_encode_time.py [--write] [--iters 10]
"""
import argparse
import ctypes as C
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gill_amd  # noqa: E402
from gill_amd import _native as N, synth  # noqa: E402


def _time(fn, iters):
  for _ in range(2):
    fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--iters", type=int, default=10)
  args = ap.parse_args()
  gill_amd.configure_hip_runtime()
  dev = torch.device("cuda:0")
  cfg = synth.VAEConfig.sd15()
  sd = {**synth.vae_decoder_state_dict(cfg, seed=0), **synth.vae_encoder_state_dict(cfg, seed=0)}
  v = N.gill_vae_config(latent_channels=4, out_channels=3, layers_per_block=2, norm_num_groups=32, latent_size=64,
                        scaling_factor=cfg.scaling_factor, max_batch=4)
  for i in range(4):
    v.block_out_channels[i] = cfg.block_out_channels[i]
  arr, keep = N.make_tensor_table({k: t.bfloat16() for k, t in sd.items()}, dev)
  h = C.c_void_p()
  N.check(N.lib().gill_vae_create(C.byref(h), C.byref(v), arr, len(sd)))
  del keep
  rows = []
  for B in (1, 4):
    img = (torch.rand((B, 3, 512, 512), device=dev) * 2 - 1).contiguous()
    noise = torch.randn((B, 4, 64, 64), device=dev)
    lat = torch.empty((B, 4, 64, 64), device=dev)
    out = torch.empty((B, 3, 512, 512), device=dev)
    s = N.current_stream()
    enc = _time(lambda: N.check(N.lib().gill_vae_encode(h, N.ptr(img), B, N.ptr(noise), N.ptr(lat), None, s)), args.iters)
    dec = _time(lambda: N.check(N.lib().gill_vae_decode(h, N.ptr(lat), B, N.ptr(out), None, s)), args.iters)
    rows.append(f"| {B} | {enc:.2f} | {dec:.2f} |")
    print(rows[-1])
  N.lib().gill_vae_destroy(h)
  if args.write:
    path = os.path.join(ROOT, "profiles", "vae_encoder.md")
    text = open(path).read() if os.path.exists(path) else "# VAE encoder\n"
    block = ("<!-- time -->\n## Time at SD-1.5 size (tools/vae_encode_time.py)\n\nHIP events around " + str(args.iters) +
             " back-to-back calls after 2 warm-up calls, one MI355X, synthetic bf16 weights, 512x512 pixels; the decoder's time is from the same "
             "run and handle.  No bar: first measurement.\n\n| B | gill_vae_encode ms | gill_vae_decode ms |\n|---|---|---|\n" +
             "\n".join(rows) + "\n<!-- /time -->\n")
    if "<!-- time -->" in text:
      text = re.sub(r"<!-- time -->.*?<!-- /time -->\n", lambda _: block, text, flags=re.S)
    else:
      text = text.rstrip("\n") + "\n\n" + block
    open(path, "w").write(text)


if __name__ == "__main__":
  main()
