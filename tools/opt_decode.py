#!/usr/bin/env python3
"""KV-cached greedy decoding on the OPT-6.7b shapes (GILLModel.generate, 8-token prompt, N new tokens): ms per decoded token.
  python tools/opt_decode.py [new_tokens] [--batch B[,B2..]] [--host] [--alternate R]
--host runs the host decision (GILLModel.decode_on_device = False: logits copied to the host, rule + argmax there);
--alternate R times the device and the host decision R times each, alternating, with the mean sclk of each run."""
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


def run(emb, on_device):
  B = emb.shape[0]
  g.model.decode_on_device = on_device
  g.model.generate(emb, 4, use_kv_cache=True, **kw)
  torch.cuda.synchronize()
  clk = bench.ClockSampler(dev)
  clk.start()
  t0 = time.time()
  out, _, _ = g.model.generate(emb, n, use_kv_cache=True, **kw)
  torch.cuda.synchronize()
  dt = time.time() - t0
  c = clk.stop()
  waits = g.model._decode_host_waits
  sclk = c["sclk_mhz_mean"]
  print(f"OPT-6.7b KV-cached decode, batch {B}, {'device' if on_device else 'host'} decision: {n} tokens in {dt * 1e3:.1f} ms = "
        f"{dt / n * 1e3:.2f} ms per token, {waits} host waits, sclk {'%.0f MHz' % sclk if sclk else 'n/a'}", flush=True)
  return out


for B in [int(b) for b in a.batch.split(",")]:
  ids = synth.synthetic_prompt_ids(B, 8, seed=1)[:, :8].to(dev)
  emb = g.model.input_embeddings(ids)
  if a.alternate:
    outs = []
    for _ in range(a.alternate):
      outs.append(run(emb, True))
      outs.append(run(emb, False))
    assert all(torch.equal(o, outs[0]) for o in outs), "device and host decisions disagree"
  else:
    run(emb, not a.host)
