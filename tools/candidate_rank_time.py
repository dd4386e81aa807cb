#!/usr/bin/env python3
"""Candidate ranking against a cached dialogue (DialogueSession.score over gill_opt_score_candidates / csrc/attention_fork.hip) timed beside the
two routes the project had before.
  python tools/candidate_rank_time.py [--rounds R] [--reps N] [--write [PATH]]      PATH: default profiles/candidate_ranking.md (its timing section)
OPT-6.7b shapes with synthetic weights, load_sd=False, text only, one process on one MI355X.
1. One dialogue whose cache holds about 100 and about 1000 tokens; 16 and 100 candidates of 8 tokens, and one case of 32 tokens.  Three arms
   alternate in one process, round by round; wall time with a device synchronisation at both ends, mean (min .. max) over the rounds:
     (a) rank        DialogueSession.score on the session that holds the history: one packed call, the history is not re-run;
     (b) loop        GILL.get_log_likelihood_scores once per candidate on history + candidate (the whole history through all layers, the
                     logits of every position copied to the host): the oldest route, and another normalisation (it averages over the history);
     (c) batched     GILLModel.lm_forward_loss over the concatenations history + candidate in chunks of 16 sequences (what fits the handle).
   Arms (b) and (c) take the handle's cache over, so arm (a) re-opens its session and extends it (not timed) in every round.
2. gill_attention_fork alone beside ops.attention_extend at equal counts on one row whose cache holds the prefix: C candidates in ONE fork launch
   against ONE extend call of one row (the extend operator has no way to run C continuations of one row in a call: C calls would be serial);
   device events around one call that enqueues --reps + 1 launches (GILL_OP_REPEAT) minus one call that enqueues one, over --reps."""
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
ap.add_argument("--write", nargs="?", const="profiles/candidate_ranking.md", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
BEGIN, END = "<!-- timing:begin -->", "<!-- timing:end -->"
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
tok = m.tokenizer
words = lambda tag, n: " ".join(f"{tag}w{i}" for i in range(n))      # noqa: E731  (n tokens)
CHUNK = 16


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  out = fn()
  torch.cuda.synchronize()
  return (time.time() - t0) * 1e3, out


say("## Timings (`python tools/candidate_rank_time.py --write`)")
say()
say("OPT-6.7b shapes (synthetic weights), `load_sd=False`, text only, one process on one MI355X.  Figures as measured; nothing in the tests depends "
    "on them.  One candidate per 32-query wave tile is what `csrc/attention_fork.hip` builds: a candidate of 8 tokens fills a quarter of its tile.")
say()
say(f"### One dialogue, three arms alternating, {a.rounds} rounds; wall ms, mean (min .. max)")
say()
say("(a) `DialogueSession.score` on the session that holds the history; (b) `GILL.get_log_likelihood_scores` once per candidate on history + "
    "candidate (it averages over the history's positions too: another normalisation); (c) `GILLModel.lm_forward_loss` over the concatenations in "
    f"chunks of {CHUNK} sequences.")
say()
say("| cached tokens | candidates | tokens each | (a) rank, ms | (b) loop, ms | (c) batched, ms | (b) / (a) | (c) / (a) |")
say("|---|---|---|---|---|---|---|---|")
for target, n_cand, n_tok in ((100, 16, 8), (100, 100, 8), (1000, 16, 8), (1000, 100, 8), (1000, 16, 32)):
  hist = words("h", target - 1)                                      # + <bos>
  cands = [words(f"c{j}", n_tok) for j in range(n_cand)]
  hist_ids = [int(v) for v in tok(hist, add_special_tokens=True, return_tensors="pt").input_ids[0].tolist()]
  cand_ids = [[int(v) for v in tok(c, add_special_tokens=False, return_tensors="pt").input_ids[0].tolist()] for c in cands]
  T = len(hist_ids) + n_tok
  m._opt_native(CHUNK, T + 8)        # one handle for all arms: no rebuild inside a timed run

  def rank_arm():
    s = m.open_session(1, T + 8)
    s.extend([0], ids=[hist_ids])
    return timed(lambda: s.score([0], [cand_ids]))[0]

  def loop_arm():
    return timed(lambda: [g.get_log_likelihood_scores([hist + " " + c]) for c in cands])[0]

  def batched_arm():
    def run():
      out = []
      for i in range(0, n_cand, CHUNK):
        part = cand_ids[i:i + CHUNK]
        ids = torch.tensor([hist_ids + c for c in part])
        labels = torch.tensor([[-100] * len(hist_ids) + c for c in part])
        out.append(m.lm_forward_loss(ids, labels).token_loss[:, len(hist_ids) - 1:].sum(1).cpu())
      return out
    return timed(run)[0]

  rank_arm(), loop_arm(), batched_arm()      # warm-up
  ta, tb, tc = [], [], []
  for _ in range(a.rounds):
    ta.append(rank_arm())
    tb.append(loop_arm())
    tc.append(batched_arm())
  say(f"| {len(hist_ids)} | {n_cand} | {n_tok} | {spread(ta)} | {spread(tb)} | {spread(tc)} | {statistics.mean(tb) / statistics.mean(ta):.2f} | "
      f"{statistics.mean(tc) / statistics.mean(ta):.2f} |")

say()
say("### `gill_attention_fork` alone beside `ops.attention_extend`")
say()
say(f"H = 32, d = 128, one cache row that holds the prefix.  Fork: C candidates of the given count in one launch.  Extend: ONE row of that count at "
    f"the prefix length in one call (store launch + attention launch); C continuations of one row would take C serial calls.  Device events around "
    f"one call that enqueues {a.reps} + 1 launches (`GILL_OP_REPEAT`) minus one call that enqueues one, over {a.reps}; {a.rounds} rounds.")
say()
say("| prefix | count | C | fork (C candidates), us | extend (one row), us | fork / (C x extend) |")
say("|---|---|---|---|---|---|")
gen = torch.Generator(device=dev).manual_seed(1234)
H, d = 32, 128


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


for past, cnt, C in ((96, 8, 16), (96, 8, 100), (992, 8, 16), (992, 8, 100), (992, 32, 16)):
  pitch = (past + cnt + 31) // 32 * 32
  rnd = lambda *shape: torch.randn(shape, device=dev, generator=gen).bfloat16()      # noqa: E731
  qkv = rnd(C * cnt, 3 * H * d)
  K, Vt = rnd(1, H, pitch, d), rnd(1, H, d, pitch)
  parent = torch.zeros(C, dtype=torch.int32, device=dev)
  plen = torch.full((C,), past, dtype=torch.int32, device=dev)
  cu = torch.arange(C + 1, dtype=torch.int32, device=dev) * cnt
  lens1 = torch.full((1,), past, dtype=torch.int32, device=dev)
  cu1 = torch.tensor([0, cnt], dtype=torch.int32, device=dev)
  q1 = qkv[:cnt]
  Ks, Vs = K.clone(), Vt.clone()
  frk = lambda: ops.attention_fork(qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:], K, Vt, parent, plen, cu, cnt)      # noqa: E731
  ext = lambda: ops.attention_extend(q1[:, :H * d], q1[:, H * d:2 * H * d], q1[:, 2 * H * d:], Ks, Vs, lens1, cu1, cnt)      # noqa: E731
  res = []
  for run in (frk, ext):
    for _ in range(3):
      run()
    res.append([(one_call(run, a.reps + 1) - one_call(run, 1)) / a.reps for _ in range(a.rounds)])
  say(f"| {past} | {cnt} | {C} | {spread(res[0])} | {spread(res[1])} | {statistics.mean(res[0]) / (C * statistics.mean(res[1])):.2f} |")

if a.write:
  text = BEGIN + "\n" + "\n".join(lines) + "\n" + END
  old = open(a.write).read() if os.path.exists(a.write) else "# Candidate ranking: tolerances and timings\n"
  if BEGIN in old:
    i, j = old.index(BEGIN), old.index(END) + len(END)
    new = old[:i] + text + old[j:]
  else:
    new = old.rstrip("\n") + "\n\n" + text + "\n"
  with open(a.write, "w") as f:
    f.write(new)
  print("wrote", a.write)
