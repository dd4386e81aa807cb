#!/usr/bin/env python3
"""Ragged batched decoding on the OPT-6.7b shapes, timed beside the uniform path, one process, both arms alternating.
  python tools/ragged_decode_time.py [--rounds R] [--write [PATH]]        the three tables below (PATH: default profiles/ragged_decode.md)
  python tools/ragged_decode_time.py --ops-only [--reps N]               only the attention launches, for a kernel trace:
      rocprofv3 --kernel-trace --stats -- python tools/ragged_decode_time.py --ops-only
1. 16 dialogues at lengths spread over 20 .. 200, 32 words each ([IMG] suppressed: 32 plain decisions per row): GILLModel.generate_batch
   once, beside the same 16 prompts through the batch-1 generate() one after another.  Both arms include their prefill.
2. Equal lengths (8-token prompts, 32 words): generate_batch beside generate() at the same B, B = 4 and 16.
3. ops.attention_decode alone at (B, n) = (1, 2048), (16, 200), (16, 2048), 32 heads of 128: device events around --reps back-to-back
   launches, as GB/s of K / V read (2 * B * H * n * d * 2 bytes).  The flash kernel at nq = 1 on the same shapes runs through
   ops.attention, which packs its operands per call: its KERNEL time comes from the kernel trace (--ops-only), not from events."""
import argparse
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gill_amd
gill_amd.configure_hip_runtime()

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--ops-only", action="store_true")
ap.add_argument("--write", nargs="?", const="profiles/ragged_decode.md", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
H, D_HEAD, WORDS = 32, 128, 32
OP_SHAPES = [(1, 2048), (16, 200), (16, 2048)]
lines = []


def say(s=""):
  print(s, flush=True)
  lines.append(s)


def spread(v):
  return f"{statistics.mean(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def op_inputs(B, n):
  from gill_amd import ops   # noqa: F401
  pitch = (n + 1 + 31) // 32 * 32
  g = torch.Generator(device="cpu").manual_seed(B * 10007 + n)
  mk = lambda *s: torch.randn(s, generator=g).to(dev, torch.bfloat16)   # noqa: E731
  return mk(B, H * D_HEAD), mk(B, H * D_HEAD), mk(B, H * D_HEAD), mk(B, H, pitch, D_HEAD), mk(B, H, D_HEAD, pitch), \
    torch.full((B,), n, dtype=torch.int32, device=dev)


def time_ops():
  from gill_amd import ops
  say("| B | n | K / V bytes read | `attention_decode` us per launch (events) | GB/s |")
  say("|---|---|---|---|---|")
  for B, n in OP_SHAPES:
    q, k, v, K, Vt, lens = op_inputs(B, n)
    for _ in range(3):
      ops.attention_decode(q, k, v, K, Vt, lens)
    us = []
    for _ in range(a.rounds):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(a.reps):
        ops.attention_decode(q, k, v, K, Vt, lens)
      e1.record()
      e1.synchronize()
      us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    nbytes = 2 * B * H * n * D_HEAD * 2
    say(f"| {B} | {n} | {nbytes / 1e6:.1f} MB | {spread(us)} | {nbytes / (statistics.mean(us) * 1e-6) / 1e9:.0f} |")
    # the flash kernel at nq = 1 on the same keys (for the kernel trace; its launch is inside an operator that packs per call)
    kk = torch.randn((B, n + 1, H * D_HEAD)).to(dev, torch.bfloat16)
    for _ in range(a.reps if a.ops_only else 2):
      ops.attention(q[:, None], kk, kk, H, causal=True)
    torch.cuda.synchronize()


if a.ops_only:
  time_ops()
  sys.exit(0)

import bench   # noqa: E402
from types import SimpleNamespace   # noqa: E402
from gill_amd import synth   # noqa: E402
from gill_amd.models import GILL   # noqa: E402

ocfg = synth.OptConfig.opt_6_7b()
osd = bench.gpu_state_dict(lambda c, meta: bench.shapes_of("opt_state_dict", c), ocfg, dev, 0)
args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-6.7b", visual_encoder="openai/clip-vit-large-patch14",
                       n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                       ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                       gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=osd)
g = GILL(synth.HashTokenizer(), args, load_sd=False).eval().bfloat16().cuda()
del osd
m = g.model
kw = dict(min_word_tokens=WORDS)          # [IMG] suppressed: WORDS ordinary greedy decisions per row


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  fn()
  torch.cuda.synchronize()
  return (time.time() - t0) * 1e3


def arms(ids, lens):
  """-> (ms of one generate_batch over all rows, ms of generate() per row one after another, ms of generate() on the whole batch or None)."""
  B = ids.shape[0]
  emb = m.input_embeddings(ids)
  batch = lambda: m.generate_batch(ids=ids, lengths=lens, max_len=WORDS, **kw)                    # noqa: E731
  each = lambda: [m.generate(emb[b:b + 1, :n], WORDS, **kw) for b, n in enumerate(lens)]          # noqa: E731
  uniform = (lambda: m.generate(emb, WORDS, **kw)) if len(set(lens)) == 1 else None               # noqa: E731
  m._opt_native(16, 480)                   # one handle for every arm: no rebuild inside a timed run
  for fn in (batch, each if uniform is None else uniform):
    fn()
  tb, te, tu = [], [], []
  for _ in range(a.rounds):
    tb.append(timed(batch))
    arms.waits = m._decode_host_waits
    if uniform is None:
      te.append(timed(each))
    else:
      tu.append(timed(uniform))
  return tb, te, tu


say("# Ragged batched decoding")
say()
say("`python tools/ragged_decode_time.py`: OPT-6.7b shapes (synthetic weights), one process on one MI355X, the arms of every table alternating, "
    f"{a.rounds} rounds; mean (min .. max) of the rounds' wall times with a device synchronisation at both ends.  Both arms include their prefill.")
say()
say("## 16 ragged dialogues")
say()
lens = [20 + round(b * 180 / 15) for b in range(16)]
ids = synth.synthetic_prompt_ids(16, 200, seed=3)[:, :200].to(dev)
tb, te, _ = arms(ids, lens)
say(f"Lengths {lens}, {WORDS} words per dialogue (`min_word_tokens = {WORDS}`: plain decisions only).")
say()
say("| arm | ms, 16 dialogues | ms per iteration | dialogues x tokens / s |")
say("|---|---|---|---|")
say(f"| `generate_batch`, one ragged batch of 16 | {spread(tb)} | {statistics.mean(tb) / WORDS:.2f} | {16 * WORDS / statistics.mean(tb) * 1e3:.0f} |")
say(f"| `generate()` at batch 1, 16 calls one after another | {spread(te)} | {statistics.mean(te) / (16 * WORDS):.2f} | "
    f"{16 * WORDS / statistics.mean(te) * 1e3:.0f} |")
say()
say(f"Ratio of the means: {statistics.mean(te) / statistics.mean(tb):.2f} x.  Host waits of the last `generate_batch`: {arms.waits}.")
say()
say("## Equal lengths")
say()
say("8-token prompts: `generate_batch` beside `generate()` at the same B.")
say()
say("| B | `generate_batch` ms | per iteration | `generate()` ms | per step |")
say("|---|---|---|---|---|")
for B in (4, 16):
  ids = synth.synthetic_prompt_ids(B, 8, seed=1)[:, :8].to(dev)
  tb, _, tu = arms(ids, [8] * B)
  say(f"| {B} | {spread(tb)} | {statistics.mean(tb) / WORDS:.2f} | {spread(tu)} | {statistics.mean(tu) / WORDS:.2f} |")
say()
say("## `attention_decode` alone")
say()
time_ops()
if a.write:
  with open(a.write, "w") as f:
    f.write("\n".join(lines) + "\n")
  print("wrote", a.write)
