"""HIP-event time of inpainting at SD-1.5 size (64x64 latents), synthetic weights (timing does not depend on the values):

  1. gill_sd_inpaint in blend mode beside gill_sd_denoise_from at the same start: 4 prompts, guidance 7.5, DDIM, 50 steps at strength 0.8 (40 UNet
     calls of batch 8), alternating runs on one handle — what the extra launch per step costs inside the replayed graph;
  2. gill_unet_forward of the 9-channel inpainting UNet beside the 4-channel one, batch 8 — what conv_in's second K step costs.

`--write` records the numbers in profiles/inpaint.md; there is no bar.

    python tools/inpaint_time.py [--write] [--runs 5] [--forward-iters 20]
"""
import argparse
import ctypes as C
import dataclasses
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gill_amd  # noqa: E402
from bench import gpu_state_dict, shapes_of  # noqa: E402
from gill_amd import _native as N, synth  # noqa: E402
from gill_amd.sd import GillSDPipeline, as_sampler_config  # noqa: E402

B, STEPS, STRENGTH, GUIDANCE = 4, 50, 0.8, 7.5


def _events(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b)


def _pipe(cfg, dev, seed):
  sd = gpu_state_dict(lambda c, meta: shapes_of("unet_state_dict", c), cfg, dev, seed)
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, 0)
  return GillSDPipeline(sd, cfg, uncond, dev, max_batch=2 * B)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--forward-iters", type=int, default=20)
  args = ap.parse_args()
  gill_amd.configure_hip_runtime()
  dev = torch.device("cuda:0")
  cfg = synth.UNetConfig.sd15()
  L = cfg.sample_size
  g = torch.Generator(device=dev).manual_seed(5)
  rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)  # noqa: E731
  lib, s = N.lib(), N.current_stream()

  # ---- 1. the loop: blend mode beside image-to-image
  pipe = _pipe(cfg, dev, 1)
  sp = as_sampler_config("ddim").native(0.0)
  start = STEPS - min(int(STEPS * STRENGTH), STEPS)
  cond = rnd(B, cfg.ctx_len, cfg.cross_attention_dim).bfloat16().contiguous()
  x0, z0, out = rnd(B, 4, L, L), rnd(B, 4, L, L), torch.empty((B, 4, L, L), device=dev)
  lm = (torch.rand((B, 1, L, L), device=dev, generator=g) < 0.5).float().contiguous()
  un = pipe.uncond_embeds
  plain = lambda: N.check(lib.gill_sd_denoise_from(pipe._h, C.byref(sp), N.ptr(cond), N.ptr(un), 1, start, N.ptr(x0), N.ptr(z0), B, STEPS, GUIDANCE,  # noqa: E731
                                                   N.ptr(out), None, s))
  blend = lambda: N.check(lib.gill_sd_inpaint(pipe._h, C.byref(sp), N.ptr(cond), N.ptr(un), 1, start, N.ptr(x0), N.ptr(z0), N.ptr(lm), None, B, STEPS,  # noqa: E731
                                              GUIDANCE, N.ptr(out), None, s))
  for fn in (plain, blend, plain, blend):      # warm-up: the eager first step and the capture of both graphs, then one replayed loop each
    fn()
  torch.cuda.synchronize()
  t_plain, t_blend = [], []
  for _ in range(args.runs):
    t_plain.append(_events(plain))
    t_blend.append(_events(blend))
  ncalls = STEPS - start
  mp, mb = statistics.median(t_plain), statistics.median(t_blend)
  loop_rows = [f"| gill_sd_denoise_from | {mp:.2f} | {min(t_plain):.2f} | {max(t_plain):.2f} | {mp / ncalls:.3f} |",
               f"| gill_sd_inpaint (blend) | {mb:.2f} | {min(t_blend):.2f} | {max(t_blend):.2f} | {mb / ncalls:.3f} |"]
  delta = f"median difference {mb - mp:+.2f} ms per loop = {(mb - mp) / ncalls * 1000:+.1f} us per step ({(mb / mp - 1) * 100:+.2f} %)"
  print("\n".join(loop_rows + [delta]))

  # ---- 2. one UNet forward: 9 input channels beside 4
  pipe9 = _pipe(dataclasses.replace(cfg, in_channels=9), dev, 1)
  Bx = 2 * B
  ts = (C.c_float * Bx)(*([501.0] * Bx))
  ctx = rnd(Bx, cfg.ctx_len, cfg.cross_attention_dim).bfloat16().contiguous()
  x4, x9, eps = rnd(Bx, 4, L, L), rnd(Bx, 9, L, L), torch.empty((Bx, 4, L, L), device=dev)
  f4 = lambda: N.check(lib.gill_unet_forward(pipe._h, N.ptr(x4), ts, N.ptr(ctx), Bx, N.ptr(eps), s))  # noqa: E731
  f9 = lambda: N.check(lib.gill_unet_forward(pipe9._h, N.ptr(x9), ts, N.ptr(ctx), Bx, N.ptr(eps), s))  # noqa: E731
  many = lambda fn: lambda: [fn() for _ in range(args.forward_iters)]  # noqa: E731
  for fn in (f4, f9, f4, f9):
    fn()
  torch.cuda.synchronize()
  t4, t9 = [], []
  for _ in range(args.runs):
    t4.append(_events(many(f4)) / args.forward_iters)
    t9.append(_events(many(f9)) / args.forward_iters)
  m4, m9 = statistics.median(t4), statistics.median(t9)
  fwd_rows = [f"| 4 | {m4:.3f} | {min(t4):.3f} | {max(t4):.3f} |", f"| 9 | {m9:.3f} | {min(t9):.3f} | {max(t9):.3f} |"]
  fdelta = f"median difference {(m9 - m4) * 1000:+.1f} us per forward ({(m9 / m4 - 1) * 100:+.2f} %)"
  print("\n".join(fwd_rows + [fdelta]))

  if args.write:
    path = os.path.join(ROOT, "profiles", "inpaint.md")
    open(path, "w").write(
      "# Inpainting: measured times (tools/inpaint_time.py)\n\n"
      "One MI355X, SD-1.5 shapes (64x64 latents), synthetic bf16 weights, HIP events around whole calls.  No bar: first measurement.\n\n"
      f"## The loop: blend mode beside image-to-image\n\n{B} prompts, guidance {GUIDANCE}, DDIM, {STEPS} steps at strength {STRENGTH}: start {start}, "
      f"{ncalls} UNet calls of batch {2 * B} per loop.  One handle, both graphs captured and replayed once before timing, then {args.runs} "
      "alternating pairs of loops.  The blend adds one launch over "
      f"{B} x {4 * L * L} floats to every replayed step.\n\n| entry | median ms | min | max | ms per step |\n|---|---|---|---|---|\n" +
      "\n".join(loop_rows) + f"\n\n{delta}; the spread between runs of the same entry is in the min / max columns.\n\n"
      f"## One UNet forward: 9 input channels beside 4\n\ngill_unet_forward, batch {Bx}, timestep 501, eager launches (no graph), "
      f"{args.forward_iters} back-to-back forwards per sample, {args.runs} alternating samples.  conv_in runs on K = 128 for 9 channels and K = 64 for 4; "
      "everything after it is the same.\n\n| in_channels | median ms | min | max |\n|---|---|---|---|\n" + "\n".join(fwd_rows) + f"\n\n{fdelta}.\n\n"
      "A difference smaller than the min - max spread of its two rows is not resolved by this measurement.\n")


if __name__ == "__main__":
  main()
