#!/usr/bin/env python3
"""Dialogue sessions (GILL.open_dialogues: every row's KV cache kept across turns) timed beside the from-scratch batch entry.
  python tools/dialogue_session_time.py [--rounds R] [--reps N] [--write [PATH]]      PATH: default profiles/dialogue_session.md
OPT-6.7b shapes with synthetic weights, load_sd=False, text-only prompts, one process on one MI355X.
1. 16 dialogues, three turns each, at histories of about 100 and about 1000 tokens: turn 1 brings the history (0.8 .. 1.2 of the target, a
   different length per dialogue), turns 2 and 3 bring 12 .. 42 new tokens; every turn decodes 32 words (30 plain decisions, then
   gen_scale_factor = 1e5 forces two [IMG] blocks: 46 tokens).  The two arms alternate in one process, round by round:
     session       one GillDialogues, .say(turn) three times: turn 1 is the packed prefill, turns 2 and 3 feed [pending token | new tokens];
     from scratch  generate_for_images_and_texts_batch on the concatenated prompt lists: the whole history again at every turn.  The replies
                   are stated as filler strings of the reply's token count (the tokenizer stand-in cannot re-encode decoded words), so the two arms
                   see histories of the same lengths, not the same words.
   Wall time per turn with a device synchronisation at both ends; mean (min .. max) over the rounds.
2. gill_attention_extend alone beside ops.attention (the flash kernel, causal) at equal uniform shapes, B = 16, H = 32, d = 128: device events
   around one call that enqueues --reps + 1 launches (GILL_OP_REPEAT) minus one call that enqueues one, over --reps; the wrappers' own passes
   (ops.attention packs heads and waits) cancel.  The extend figure includes its store launch."""
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--write", nargs="?", const="profiles/dialogue_session.md", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
N, WORDS, PLAIN, REPLY = 16, 32, 30, 30 + 16
lines = []


def say(s=""):
  print(s, flush=True)
  lines.append(s)


def spread(v, fmt=".1f"):
  return f"{statistics.mean(v):{fmt}} ({min(v):{fmt}} .. {max(v):{fmt}})"


import bench   # noqa: E402
from types import SimpleNamespace   # noqa: E402
from gill_amd import ops, synth   # noqa: E402
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
kw = dict(num_words=WORDS, min_word_tokens=PLAIN, gen_scale_factor=1e5)
words = lambda tag, n: " ".join(f"{tag}w{i}" for i in range(n))      # noqa: E731  (n tokens)
gen_prefix = "".join(f"[IMG{i}]" for i in range(8))


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  out = fn()
  torch.cuda.synchronize()
  return (time.time() - t0) * 1e3, out


say("# Dialogue sessions: each row's KV cache kept across turns")
say()
say("`python tools/dialogue_session_time.py --write`: OPT-6.7b shapes (synthetic weights), `load_sd=False`, text-only prompts, one process on one "
    "MI355X.  Figures as measured; nothing in the tests depends on them.")
say()
say(f"## {N} dialogues, three turns, both arms alternating")
say()
say(f"Every turn decodes {WORDS} words per dialogue ({PLAIN} plain decisions, then two forced [IMG] blocks: {REPLY} tokens).  `session`: one "
    "`GILL.open_dialogues` object, `.say()` per turn (turn 1 is the packed prefill through `gill_opt_extend`; turns 2 and 3 feed the pending token and "
    "the new tokens at each row's cached length).  `from scratch`: `generate_for_images_and_texts_batch` on the concatenated prompt lists, the whole "
    "history again at every turn; the replies are filler strings of the reply's token count, so the arms see histories of the same lengths, not the "
    f"same words.  {a.rounds} rounds, the arms alternating; wall ms per turn with a device synchronisation at both ends, mean (min .. max).")
for target in (100, 1000):
  first = [round(target * (0.8 + 0.4 * b / (N - 1))) for b in range(N)]
  later = [[12 + 2 * ((b + 5 * t) % N) for b in range(N)] for t in range(2)]
  turns = [[[words(f"h{b}t0", first[b] - 1)] for b in range(N)]] + [[[words(f"h{b}t{t + 1}", later[t][b])] for b in range(N)] for t in range(2)]
  filler = lambda b, t: words(f"r{b}t{t}", PLAIN) + " " + gen_prefix * 2      # noqa: E731
  scratch_lists = []
  for t in range(3):
    scratch_lists.append([sum(([*turns[u][b], filler(b, u)] for u in range(t)), []) + turns[t][b] for b in range(N)])
  hist = [[first[b] + sum(REPLY + later[u][b] for u in range(t)) for b in range(N)] for t in range(3)]
  cap = max(hist[2]) + 8 * WORDS + 8
  m._opt_native(N, cap)      # one handle for both arms: no rebuild inside a timed run

  def session_arm():
    d = g.open_dialogues(N, capacity=cap)
    return [timed(lambda t=t: d.say(turns[t], **kw))[0] for t in range(3)]

  def scratch_arm():
    return [timed(lambda t=t: g.generate_for_images_and_texts_batch(scratch_lists[t], **kw))[0] for t in range(3)]

  session_arm(), scratch_arm()      # warm-up: handles, kernels, allocator
  ts, tf = [], []
  for _ in range(a.rounds):
    ts.append(session_arm())
    tf.append(scratch_arm())
  say()
  say(f"### Histories of about {target} tokens")
  say()
  say(f"Prompt lengths at turn 1: {min(first)} .. {max(first)} tokens; new tokens at turns 2 and 3: {min(min(l) for l in later)} .. "
      f"{max(max(l) for l in later)} per dialogue; history a turn decodes from: " +
      ", ".join(f"turn {t + 1}: {min(hist[t])} .. {max(hist[t])}" for t in range(3)) + ".")
  say()
  say("| turn | session, ms | from scratch, ms | from scratch / session (means) |")
  say("|---|---|---|---|")
  for t in range(3):
    s_, f_ = [r[t] for r in ts], [r[t] for r in tf]
    say(f"| {t + 1} | {spread(s_)} | {spread(f_)} | {statistics.mean(f_) / statistics.mean(s_):.2f} |")
  s_, f_ = [sum(r) for r in ts], [sum(r) for r in tf]
  say(f"| all three | {spread(s_)} | {spread(f_)} | {statistics.mean(f_) / statistics.mean(s_):.2f} |")

say()
say("## `gill_attention_extend` alone beside `ops.attention`")
say()
say(f"B = 16, H = 32, d = 128, uniform rows; device events around one call that enqueues {a.reps} + 1 launches (`GILL_OP_REPEAT`) minus one call that "
    f"enqueues one, over {a.reps}: the wrappers' own passes cancel.  The extend figure is its store launch plus its attention launch; `ops.attention` "
    f"is the flash kernel, causal, on operands its QKV epilogue would have laid out.  {a.rounds} rounds.")
say()
say("| cached length | new tokens per row | `gill_attention_extend`, us | `ops.attention(causal=True)`, us | extend / flash |")
say("|---|---|---|---|---|")
gen = torch.Generator(device=dev).manual_seed(1234)
B, H, d = 16, 32, 128


def one_call(run, repeat):
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


for past, cnt in ((0, 128), (0, 1024), (128, 32), (1024, 32), (1024, 128)):
  pitch = (past + cnt + 31) // 32 * 32
  rnd = lambda *shape: torch.randn(shape, device=dev, generator=gen).bfloat16()      # noqa: E731
  qkv = rnd(B * cnt, 3 * H * d)
  K, Vt = rnd(B, H, pitch, d), rnd(B, H, d, pitch)
  lens = torch.full((B,), past, dtype=torch.int32, device=dev)
  cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * cnt
  q, k, v = rnd(B, cnt, H * d), rnd(B, past + cnt, H * d), rnd(B, past + cnt, H * d)
  ext = lambda: ops.attention_extend(qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:], K, Vt, lens, cu, cnt)      # noqa: E731
  fla = lambda: ops.attention(q, k, v, H, causal=True)      # noqa: E731
  res = []
  for run in (ext, fla):
    for _ in range(3):
      run()
    res.append([(one_call(run, a.reps + 1) - one_call(run, 1)) / a.reps for _ in range(a.rounds)])
  say(f"| {past} | {cnt} | {spread(res[0])} | {spread(res[1])} | {statistics.mean(res[0]) / statistics.mean(res[1]):.2f} |")
if a.write:
  with open(a.write, "w") as f:
    f.write("\n".join(lines) + "\n")
  print("wrote", a.write)
