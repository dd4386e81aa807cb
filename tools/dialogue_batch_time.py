#!/usr/bin/env python3
"""Batched dialogues with every branch (generate_for_images_and_texts_batch(all_branches=True)) timed beside the one-sequence loop.
  python tools/dialogue_batch_time.py [--rounds R] [--rows N] [--write [PATH]]      PATH: default profiles/img_heads.md
OPT-6.7b shapes with synthetic weights, a seeded N x 256 retrieval index (default 2.7 M rows, unit rows), a decision Linear(4096, 2),
load_sd=False; path_array points at eight local PNGs.  16 dialogues of 20 .. 200 tokens, 32 words each: 30 plain decisions
(min_word_tokens = 30), then gen_scale_factor = 1e5 forces an [IMG] block, so every dialogue has one block with hidden states.
1. The two arms alternate in one process: the batch entry once; generate_for_images_and_texts per dialogue one after another.  Wall
   time with a device synchronisation at both ends, mean (min .. max) of the rounds.
2. gill_op_img_block_heads alone at n = 1, 16, 64 (D = 4096, E = 256, C = 2): device events around one call that enqueues --reps + 1 launches
   (GILL_OP_REPEAT) minus one call that enqueues one, over --reps.
3. Host waits per call of both arms: the synchronising torch operations torch.cuda.set_sync_debug_mode reports (copies to the host,
   .item(), .tolist()); waits inside libgill_amd are not counted by it and there are none on these paths but those of the decode loop,
   which generate_batch counts itself (_decode_host_waits)."""
import argparse
import os
import statistics
import sys
import tempfile
import time
import warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gill_amd
gill_amd.configure_hip_runtime()

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rows", type=int, default=2_700_000)
ap.add_argument("--write", nargs="?", const="profiles/img_heads.md", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
WORDS, PLAIN = 32, 30
lines = []


def say(s=""):
  print(s, flush=True)
  lines.append(s)


def spread(v, fmt=".1f"):
  return f"{statistics.mean(v):{fmt}} ({min(v):{fmt}} .. {max(v):{fmt}})"


import bench   # noqa: E402
from types import SimpleNamespace   # noqa: E402
from PIL import Image   # noqa: E402
from gill_amd import ops, synth   # noqa: E402
from gill_amd.models import GILL   # noqa: E402
from gill_amd.retrieval import GillRetrievalIndex   # noqa: E402

ocfg = synth.OptConfig.opt_6_7b()
osd = bench.gpu_state_dict(lambda c, meta: bench.shapes_of("opt_state_dict", c), ocfg, dev, 0)
args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-6.7b", visual_encoder="openai/clip-vit-large-patch14",
                       n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                       ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                       gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=osd)
tmp = tempfile.mkdtemp(prefix="dialogue_batch_time_")
pngs = []
for k in range(8):
  p = os.path.join(tmp, f"{k}.png")
  Image.fromarray(np.full((64, 64, 3), 30 * k, dtype=np.uint8)).save(p)
  pngs.append(p)
g = GILL(synth.HashTokenizer(), args, path_array=[pngs[k % 8] for k in range(a.rows)], load_sd=False)
dec = torch.nn.Sequential(torch.nn.Dropout(0.5), torch.nn.Linear(ocfg.hidden_size, 2))
with torch.no_grad():
  dec[1].weight.copy_(synth.normal("decision.w", (2, ocfg.hidden_size), 3, 0.02))
g.decision_model = dec.eval()
g = g.eval().bfloat16().cuda()
del osd
gen = torch.Generator(device=dev).manual_seed(1234)
index = GillRetrievalIndex(256, a.rows, dev)
for lo in range(0, a.rows, 1 << 18):      # seeded rows in pieces: the fp32 draw never exists whole
  index.add(torch.randn((min(1 << 18, a.rows - lo), 256), device=dev, generator=gen), normalize=True)
g.ret_index = index
g.emb_matrix = torch.zeros((1, 256), device=dev)      # with an index attached only its dtype is read
m = g.model

lens = [20 + round(b * 180 / 15) for b in range(16)]
dialogues = [[" ".join(f"d{b}w{i}" for i in range(n - 1))] for b, n in enumerate(lens)]      # n - 1 words and <bos>: n tokens
kw = dict(num_words=WORDS, min_word_tokens=PLAIN, gen_scale_factor=1e5)
batch = lambda: g.generate_for_images_and_texts_batch(dialogues, all_branches=True, **kw)      # noqa: E731
each = lambda: [g.generate_for_images_and_texts(d, **kw) for d in dialogues]                    # noqa: E731


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  out = fn()
  torch.cuda.synchronize()
  return (time.time() - t0) * 1e3, out


def host_waits(fn):
  """Synchronising torch operations of one call (None where the debug mode is not available)."""
  try:
    torch.cuda.set_sync_debug_mode("warn")
  except Exception:
    return None
  try:
    with warnings.catch_warnings(record=True) as w:
      warnings.simplefilter("always")
      fn()
    return sum("synchroniz" in str(x.message) for x in w)
  finally:
    torch.cuda.set_sync_debug_mode("default")


m._opt_native(16, 480)      # one handle for both arms: no rebuild inside a timed run
ob, oe = batch(), each()
blocks = sum(isinstance(x, dict) for o in ob for x in o)
blocks_each = sum(isinstance(x, dict) for o in oe for x in o)
tb, te = [], []
for _ in range(a.rounds):
  tb.append(timed(batch)[0])
  te.append(timed(each)[0])
wb, we = host_waits(batch), host_waits(each)
decode_waits = m._decode_host_waits

say("# Batched dialogues with every branch: the image-block heads")
say()
say(f"`python tools/dialogue_batch_time.py --write`: OPT-6.7b shapes (synthetic weights), a {a.rows} x 256 retrieval index, a decision "
    "`Linear(4096, 2)`, `load_sd=False`, one process on one MI355X.  Figures as measured; nothing in the tests depends on them.")
say()
say("## 16 dialogues, both arms alternating")
say()
say(f"Lengths {lens}, {WORDS} words per dialogue: {PLAIN} plain decisions, then a forced [IMG] block ({blocks} blocks with hidden states in the "
    f"batch, {blocks_each} in the loop).  {a.rounds} rounds; mean (min .. max) of the wall times with a device synchronisation at both ends; both arms include their "
    "prefill, three local PNG reads per block and the mapper.")
say()
say("| arm | ms, 16 dialogues | synchronising torch operations per call |")
say("|---|---|---|")
say(f"| `generate_for_images_and_texts_batch(all_branches=True)`, one ragged batch | {spread(tb)} | {wb} (of them the decode loop's own reads: "
    f"{decode_waits}) |")
say(f"| `generate_for_images_and_texts`, 16 calls one after another (unchanged from the parent commit: the baseline) | {spread(te)} | {we} |")
say()
say(f"Ratio of the means: {statistics.mean(te) / statistics.mean(tb):.2f} x.")
say()
say("## `gill_op_img_block_heads` alone")
say()
say(f"D = 4096, E = 256, C = 2 (2.1 MB of weights per workgroup, from L2 after the first reader); device events around one call that enqueues "
    f"{a.reps} + 1 launches (`GILL_OP_REPEAT`) minus one call that enqueues one, over {a.reps}: the wrapper's host time cancels.  {a.rounds} rounds.")
say()
say("| n | us per launch |")
say("|---|---|")
hid = torch.randn((64 * 40, 4096), device=dev, generator=gen)
wr, br = torch.randn((256, 4096), device=dev, generator=gen).bfloat16() / 64, torch.zeros((256,), device=dev)
wd, bd = torch.randn((2, 4096), device=dev, generator=gen).bfloat16() / 64, torch.zeros((2,), device=dev)
for n in (1, 16, 64):
  idx = (torch.arange(n, device=dev, dtype=torch.int32) * 37) % hid.shape[0]
  out = (torch.empty((n, 256), device=dev), torch.empty((n, 2), device=dev), torch.empty((n,), device=dev, dtype=torch.int32))
  run = lambda: ops.img_block_heads(hid, idx, ret=(wr, br), decision=(wd, bd), _out=out)      # noqa: E731
  for _ in range(5):
    run()

  def one_call(repeat):
    os.environ["GILL_OP_REPEAT"] = str(repeat)      # read by the library at every call: the call enqueues `repeat` launches
    try:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      e0.record()
      run()
      e1.record()
      e1.synchronize()
      return e0.elapsed_time(e1) * 1e3
    finally:
      del os.environ["GILL_OP_REPEAT"]
  us = [(one_call(a.reps + 1) - one_call(1)) / a.reps for _ in range(a.rounds)]
  say(f"| {n} | {spread(us, '.2f')} |")
g.ret_index = None
del index
if a.write:
  with open(a.write, "w") as f:
    f.write("\n".join(lines) + "\n")
  print("wrote", a.write)
