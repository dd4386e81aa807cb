#!/usr/bin/env python3
"""Per-launch time of the seeded draw (gill_opt_draw_token: decode_sample_kernel) beside the greedy pick (gill_opt_pick_token:
decode_rule_pick_kernel<true>) on (B, 50274) fp32 logits: device events around R back-to-back launches of each, alternating.
  python tools/decode_sample_time.py [--batch 1,16] [--reps 200] [--top-p 0.95,1.0]
Under `rocprofv3 --kernel-trace --stats -- python tools/decode_sample_time.py --batch B --reps 50` the trace gives each kernel's
own duration (one batch size per run: the statistics are per kernel name)."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gill_amd
gill_amd.configure_hip_runtime()
from gill_amd import _native as N
from gill_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="1,16")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--top-p", default="0.95,1.0")
ap.add_argument("--temperature", type=float, default=0.7)
a = ap.parse_args()
dev = torch.device("cuda:0")
V, D = 50274, 768
ocfg = synth.OptConfig(vocab_size=V, hidden_size=D, num_layers=1, num_heads=12, ffn_dim=3072)
cfg = N.gill_opt_config(vocab_size=V, hidden_size=D, num_layers=1, num_heads=12, ffn_dim=3072, max_positions=ocfg.max_positions,
                        max_batch=8, max_seq=64)
arr, keep = N.make_tensor_table({k: v.bfloat16().float() for k, v in synth.opt_state_dict(ocfg, seed=5).items()}, dev)
h = C.c_void_p()
N.check(N.lib().gill_opt_create(C.byref(h), C.byref(cfg), arr, len(keep)))
del keep
rule = N.gill_decode_rule()
ids = synth.IMG_TOKEN_IDS
rule.n_ret = rule.n_gen = len(ids)
for j, v in enumerate(ids):
  rule.ret_ids[j] = rule.gen_ids[j] = v
rule.step, rule.min_word_tokens, rule.ret_eq_gen = 0, 1, 1            # [IMG] suppressed: a pick never forces
rule.ret_scale = rule.gen_scale = 1.0
rule.filter_value = float("-inf")
s = N.current_stream()


def timed(fn, reps):
  for _ in range(10):
    fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / reps * 1e3


for B in [int(b) for b in a.batch.split(",")]:
  g = torch.Generator().manual_seed(B)
  x = (torch.randn((B, V), generator=g) * 5).to(dev)
  tokens = torch.zeros((B, 16), device=dev, dtype=torch.int64)
  n_out = torch.zeros(1, device=dev, dtype=torch.int32)
  nxt = torch.zeros((B, 8, D), device=dev, dtype=torch.bfloat16)

  def pick():
    N.check(N.lib().gill_opt_pick_token(h, N.ptr(x), B, C.byref(rule), N.ptr(tokens), 16, 0, N.ptr(n_out), N.ptr(nxt), s))

  def draw_with(p):
    sm = N.gill_decode_sampler()
    sm.seed, sm.draw, sm.row0, sm.temperature, sm.top_p = 1234, 0, 0, a.temperature, p

    def draw():
      N.check(N.lib().gill_opt_draw_token(h, N.ptr(x), B, C.byref(rule), C.byref(sm), N.ptr(tokens), 16, 0, N.ptr(n_out), N.ptr(nxt), s))
    return draw

  for rnd in range(3):
    line = [f"B {B:2d} round {rnd}: pick {timed(pick, a.reps):7.1f} us"]
    for p in [float(v) for v in a.top_p.split(",")]:
      line.append(f"draw top_p {p}: {timed(draw_with(p), a.reps):7.1f} us")
    print(" | ".join(line), flush=True)
torch.cuda.synchronize()
N.lib().gill_opt_destroy(h)
