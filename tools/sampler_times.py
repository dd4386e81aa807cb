"""HIP-event time of gill_sd_denoise_ex per sampler on the full-size SD-1.5 UNet (synthetic weights, 64x64 latents) at 4 prompts with
classifier-free guidance: PNDM 50 steps (51 UNet calls), DDIM 50, Euler 30, DPM-Solver++(2M) 20.  Per case: warm-up runs (the first
captures the step graph), then the median of three timed runs, with the mean shader clock over the timed runs.  The expectation is time
proportional to the number of UNet calls: the last column is each case's ms per call over PNDM's.

  python tools/sampler_times.py [--prompts 4] [--repeat 3] [--warmup 2] [--md profiles/samplers_table.md]

Prints a markdown table and one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("pndm", 50), ("ddim", 50), ("euler", 30), ("dpmsolver++", 20))


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--prompts", type=int, default=4)
  ap.add_argument("--repeat", type=int, default=3)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--md", default=None, help="also write the table to this file")
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("sampler_times.py times the native denoise loop: it needs the MI355X")
  import gill_amd
  gill_amd.configure_hip_runtime()
  import bench
  from gill_amd import _native as N, synth
  from gill_amd.sd import GillSDPipeline, SamplerConfig
  dev = torch.device("cuda:0")
  cfg = synth.UNetConfig.sd15()
  sd = bench.gpu_state_dict(lambda c, meta: bench.shapes_of("unet_state_dict", c), cfg, dev, 1)     # the bench workload's UNet weights
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=2)
  pipe = GillSDPipeline(sd, cfg, uncond, dev, max_batch=2 * a.prompts)
  del sd
  B = a.prompts
  cond = synth.normal("st_cond", (B, cfg.ctx_len, cfg.cross_attention_dim), 3).to(dev, torch.bfloat16).contiguous()
  lat0 = synth.initial_latents(B, cfg.in_channels, cfg.sample_size, seed=1337).to(dev).contiguous()
  out = torch.empty_like(lat0)
  stream = N.current_stream()

  def run(sp, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    N.check(N.lib().gill_sd_denoise_ex(pipe._h, C.byref(sp), N.ptr(cond), N.ptr(pipe.uncond_embeds), 1, N.ptr(lat0), B, steps, 7.5,
                                       N.ptr(out), None, stream))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)

  recs = []
  for kind, steps in CASES:
    s = SamplerConfig(kind)
    ncalls = int(s.schedule(steps)[2].shape[0])
    sp = s.native()
    for _ in range(max(2, a.warmup)):       # eager first step + capture, then one replayed run
      run(sp, steps)
    clocks = bench.ClockSampler(dev)
    clocks.start()
    runs = [run(sp, steps) for _ in range(a.repeat)]
    ck = clocks.stop()
    ms = statistics.median(runs)
    recs.append({"sampler": kind, "steps": steps, "unet_calls": ncalls, "ms": ms, "ms_runs": runs, "ms_per_call": ms / ncalls,
                 "finite": bool(torch.isfinite(out).all().item()), "sclk_mhz_mean": ck["sclk_mhz_mean"]})
  base = recs[0]["ms_per_call"]
  lines = ["| sampler | steps | UNet calls | ms (median of %d) | runs (ms) | ms / call | ms / call over PNDM's | sclk_mhz_mean |" % a.repeat,
           "|---|---|---|---|---|---|---|---|"]
  for r in recs:
    r["per_call_over_pndm"] = r["ms_per_call"] / base
    clk = "n/a" if r["sclk_mhz_mean"] is None else f"{r['sclk_mhz_mean']:.0f}"
    lines.append(f"| {r['sampler']} | {r['steps']} | {r['unet_calls']} | {r['ms']:.2f} | {', '.join(f'{v:.2f}' for v in r['ms_runs'])} | "
                 f"{r['ms_per_call']:.3f} | {r['per_call_over_pndm']:.4f} | {clk} |")
  table = "\n".join(lines)
  print(table)
  if a.md:
    with open(a.md, "w") as f:
      f.write(table + "\n")
  print(json.dumps({"prompts": B, "guidance": 7.5, "cases": recs}))


if __name__ == "__main__":
  main()
