#!/usr/bin/env python3
"""KV-cached decoding on the OPT-6.7b shapes (GILLModel.generate, 8-token prompt, N new tokens): ms per decoded token.
  python tools/opt_decode.py [new_tokens] [--batch B[,B2..]] [--host] [--alternate R] [--sample T,P [--seed S]] [--weights bf16,fp8]
--host runs the host decision (GILLModel.decode_on_device = False: logits copied to the host, rule + argmax there);
--alternate R times the device and the host decision R times each, alternating, with the mean sclk of each run;
--sample T,P decodes at temperature T and top_p P instead of greedily: the seeded draw on the device (generate(seed=S)) beside
the torch.multinomial draw (seed=None), alternating under --alternate; each line prints the host waits of its loop;
--weights bf16,fp8 times the device decision on the bf16 decoder and on the weight-only fp8 decoder (quantize_lm('fp8'), called once: both
native handles are kept and swapped), R alternating rounds each under --alternate, then the 8-token [IMG] block step alone
(gill_opt_forward_cached, T_new = 8 at past_len = 8, batch 1, device events) the same way, and the mean and the spread (max - min) of
each arm's rounds."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gill_amd
gill_amd.configure_hip_runtime()
import bench
from types import SimpleNamespace
from gill_amd import synth
from gill_amd.models import GILL

ap = argparse.ArgumentParser()
ap.add_argument("new_tokens", nargs="?", type=int, default=24)
ap.add_argument("--batch", default="1", help="batch size, or a comma list (one model build for all)")
ap.add_argument("--host", action="store_true", help="host decision (decode_on_device = False)")
ap.add_argument("--alternate", type=int, default=0, help="R rounds of device / host, alternating")
ap.add_argument("--sample", default=None, help="T,P: temperature and top_p of the sampled path (seeded draw beside the torch draw)")
ap.add_argument("--seed", type=int, default=1234, help="seed of the seeded draw")
ap.add_argument("--weights", default=None, help="bf16,fp8: the device decision on both decoders, alternating under --alternate")
a = ap.parse_args()
n = a.new_tokens
dev = torch.device("cuda:0")
ocfg = synth.OptConfig.opt_6_7b()
osd = bench.gpu_state_dict(lambda c, meta: bench.shapes_of("opt_state_dict", c), ocfg, dev, 0)
args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-6.7b", visual_encoder="openai/clip-vit-large-patch14",
                       n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                       ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                       gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=osd)
g = GILL(synth.HashTokenizer(), args, load_sd=False).eval().bfloat16().cuda()
del osd
kw = dict(min_word_tokens=n, temperature=0.0)          # [IMG] suppressed: n ordinary greedy steps
if a.sample:
  t_, p_ = (float(v) for v in a.sample.split(","))
  kw = dict(min_word_tokens=n, temperature=t_, top_p=p_)


peak = 0.0      # largest logit / temperature the last run saw (sampled runs only)


handles = {}     # --weights: opt_weights -> (native handle, its capacity), both alive


def use_weights(mode):
  """Make `mode` the model's decoder: its handle is built at the first use (quantize_lm sees no handle to destroy) and swapped in afterwards."""
  m = g.model
  if m.opt_weights == mode:
    return
  handles[m.opt_weights] = (m._opt_handle, m._opt_cap)
  m._opt_handle, m._opt_cap = None, (0, 0)
  m.quantize_lm(mode)
  if mode in handles:
    m._opt_handle, m._opt_cap = handles.pop(mode)


def run(emb, on_device, seed=None, weights=None):
  global peak
  B = emb.shape[0]
  if weights:
    use_weights(weights)
  g.model.decode_on_device = on_device
  kw_run = dict(kw, seed=seed) if seed is not None else kw
  what = "seeded draw" if seed is not None else "torch draw" if a.sample else "device decision" if on_device else "host decision"
  # warm-up; with --weights at the timed length, so that neither arm's handle is rebuilt for capacity inside its first timed round
  g.model.generate(emb, n if weights else 4, use_kv_cache=True, **kw_run)
  torch.cuda.synchronize()
  clk = bench.ClockSampler(dev)
  clk.start()
  t0 = time.time()
  out, _, logits = g.model.generate(emb, n, use_kv_cache=True, **kw_run)
  torch.cuda.synchronize()
  dt = time.time() - t0
  c = clk.stop()
  waits = g.model._decode_host_waits
  sclk = c["sclk_mhz_mean"]
  if weights:
    what += f", {weights} weights"
    times.setdefault((B, weights), []).append(dt / n * 1e3)
  print(f"OPT-6.7b KV-cached decode, batch {B}, {what}: {n} tokens in {dt * 1e3:.1f} ms = "
        f"{dt / n * 1e3:.2f} ms per token, {waits} host waits, sclk {'%.0f MHz' % sclk if sclk else 'n/a'}", flush=True)
  if a.sample:
    peak = max(float(l.max()) for l in logits) / kw["temperature"]
  return out


times = {}      # --weights: (batch | "block", weights) -> ms per token (per step) of every round


def run_block(weights, reps=20):
  """The 8-token block step alone at batch 1: a prefill of 8 tokens, then `reps` cached forwards of 8 tokens at past_len = 8 (each rewrites
  the same slots), between two device events."""
  use_weights(weights)
  m = g.model
  emb = m.input_embeddings(synth.synthetic_prompt_ids(1, 16, seed=2)[:, :16].to(dev))
  m._size_kv_cache(emb, 8)
  m._lm_forward_hidden_cached(emb[:, :8], 0)
  m._lm_forward_hidden_cached(emb[:, 8:], 8)
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    m._lm_forward_hidden_cached(emb[:, 8:], 8)
  e1.record()
  torch.cuda.synchronize()
  ms = e0.elapsed_time(e1) / reps
  times.setdefault(("block", weights), []).append(ms)
  print(f"OPT-6.7b cached forward, batch 1, T_new = 8 at past_len = 8, {weights} weights: {ms:.3f} ms per step ({reps} steps, events)", flush=True)


def summary():
  for (what, w), v in times.items():
    mean = sum(v) / len(v)
    name = "8-token block step" if what == "block" else f"generate() batch {what}"
    print(f"SUMMARY {name}, {w}: mean {mean:.3f} ms, min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f} over {len(v)} rounds", flush=True)


for B in [int(b) for b in a.batch.split(",")]:
  ids = synth.synthetic_prompt_ids(B, 8, seed=1)[:, :8].to(dev)
  emb = g.model.input_embeddings(ids)
  if a.sample:
    seeded = []
    for _ in range(max(1, a.alternate)):
      seeded.append(run(emb, True, seed=a.seed))
      # the torch draw takes exp(logit / T) with no maximum subtracted and refuses an inf: it is timed only where the seeded run's
      # logits stay well below fp32's exp limit (88.7)
      if peak < 80.0:
        run(emb, True)
      else:
        print(f"OPT-6.7b KV-cached decode, batch {B}, torch draw: not run, logit / T reaches {peak:.1f} and exp() would overflow", flush=True)
    assert all(torch.equal(o, seeded[0]) for o in seeded), "the seeded draw is not repeatable"
  elif a.weights:
    for _ in range(max(1, a.alternate)):
      for w in a.weights.split(","):
        run(emb, True, weights=w)
  elif a.alternate:
    outs = []
    for _ in range(a.alternate):
      outs.append(run(emb, True))
      outs.append(run(emb, False))
    assert all(torch.equal(o, outs[0]) for o in outs), "device and host decisions disagree"
  else:
    run(emb, not a.host)
if a.weights:
  for _ in range(max(1, a.alternate)):
    for w in a.weights.split(","):
      run_block(w)
  summary()
