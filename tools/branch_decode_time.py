#!/usr/bin/env python3
"""Branch decode (DialogueSession.sample over gill_opt_decode_step_branch / csrc/attention_branch.hip) timed beside the two routes the project
had for drawing n replies from one history.
  python tools/branch_decode_time.py [--rounds R] [--reps N] [--write [PATH]]      PATH: default profiles/branch_decode.md (its timing section)
OPT-6.7b shapes with synthetic weights, load_sd=False, text only, one process on one MI355X.
1. One history of about 100 and about 1000 tokens; n = 4 and 16 replies of 32 tokens, seeded (temperature 1, top_p 1).  Three arms alternate in
   one process, round by round; wall time with a device synchronisation at both ends, mean (min .. max) over the rounds:
     (a) sample      DialogueSession.sample on ONE dialogue that holds the history: the prefix is stored once and read once per head and step;
     (b) batch       generate_batch over n copies of the history: n prefills, n stored copies, every step reads n copies;
     (c) rows        an n-row session whose rows were each extended with the history (not timed), timing only its generate: n stored copies,
                     every step reads n copies.
   Arm (b) takes the handle's cache over, so arms (a) and (c) re-open and extend their sessions (not timed) in every round.
   The cache bytes each arm holds for the history and the replies are reported beside the times.
2. gill_attention_branch alone (S = n branches in one group, m own tokens) beside gill_attention_decode at B = n rows of the same total length,
   with the key / value bytes each reads; device events around one call that enqueues --reps + 1 launches (GILL_OP_REPEAT) minus one call that
   enqueues one, over --reps."""
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
ap.add_argument("--write", nargs="?", const="profiles/branch_decode.md", default=None)
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
from gill_amd import _native as N   # noqa: E402
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
MAX_LEN, N_MAX = 32, 16
KW = dict(max_len=MAX_LEN, temperature=1.0, top_p=1.0, seed=11)


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  out = fn()
  torch.cuda.synchronize()
  return (time.time() - t0) * 1e3, out


say("## Timings (`python tools/branch_decode_time.py --write`)")
say()
say("OPT-6.7b shapes (synthetic weights), `load_sd=False`, text only, one process on one MI355X.  Figures as measured; nothing in the tests depends "
    "on them, and no dispatch between the arms is added.")
say()
say(f"### n replies of {MAX_LEN} decisions from one history, three arms alternating, {a.rounds} rounds; wall ms, mean (min .. max)")
say()
say("(a) `DialogueSession.sample` on one dialogue; (b) `generate_batch` over n copies of the history (prefill included: it is part of that route); "
    "(c) an n-row session whose rows were extended with the history (not timed), its `generate` alone.  Cache MiB: the keys and values the arm "
    "holds for the history and the replies (a: one row's prefix + the branch cache; b, c: n rows).")
say()
say("| cached tokens | n | (a) sample, ms | (b) batch, ms | (c) rows, ms | (b) / (a) | (c) / (a) | tokens a / b / c | cache MiB a | cache MiB b, c |")
say("|---|---|---|---|---|---|---|---|---|---|")
H, d, L = ocfg.num_heads, ocfg.hidden_size // ocfg.num_heads, ocfg.num_layers
slot_bytes = L * H * 2 * (d + (d + 31) // 32 * 32)         # one token's keys and values over all layers, bf16
for target in (100, 1000):
  hist_ids = [int(v) for v in tok(words("h", target - 1), add_special_tokens=True, return_tensors="pt").input_ids[0].tolist()]
  T = len(hist_ids)
  cap = T + MAX_LEN * 8 + 8
  m._opt_native(N_MAX, cap)        # one handle for all arms: no rebuild inside a timed run
  for n in (4, 16):
    ids_n = torch.tensor([hist_ids] * n, dtype=torch.int64, device=dev)

    def sample_arm():
      s = m.open_session(1, cap)
      s.extend([0], ids=[hist_ids])
      t, bs = timed(lambda: s.sample([0], n, **KW))
      return t, int(bs.n_tokens.sum()), int(N.lib().gill_opt_branch_bytes(s.handle))

    def batch_arm():
      t, out = timed(lambda: m.generate_batch(ids=ids_n, lengths=[T] * n, **KW))
      return t, int(out[1].sum())

    def rows_arm():
      s = m.open_session(n, cap)
      s.extend(list(range(n)), ids=[hist_ids] * n)
      t, out = timed(lambda: s.generate(list(range(n)), **KW))
      return t, int(out[1].sum())

    sample_arm(), batch_arm(), rows_arm()      # warm-up
    ta, tb, tc = [], [], []
    for _ in range(a.rounds):
      ra, rb, rc = sample_arm(), batch_arm(), rows_arm()
      ta.append(ra[0]); tb.append(rb[0]); tc.append(rc[0])
    mib_a = (T * slot_bytes + ra[2]) / 2 ** 20
    mib_bc = n * (T + MAX_LEN) * slot_bytes / 2 ** 20
    say(f"| {T} | {n} | {spread(ta)} | {spread(tb)} | {spread(tc)} | {statistics.mean(tb) / statistics.mean(ta):.2f} | "
        f"{statistics.mean(tc) / statistics.mean(ta):.2f} | {ra[1]} / {rb[1]} / {rc[1]} | {mib_a:.1f} | {mib_bc:.1f} |")

say()
say("### `gill_attention_branch` alone beside `gill_attention_decode`")
say()
say(f"H = 32, d = 128.  Branch: S = n siblings in one group on one main-cache row of the given prefix, m = 16 own tokens each, bpitch 64.  Decode: "
    f"B = n rows that each hold prefix + 16 tokens.  KiB read: the key and value bytes of the slots each operator selects (branch: the prefix once "
    f"per head plus n own rows; decode: n whole rows).  Device events around one call that enqueues {a.reps} + 1 launches (`GILL_OP_REPEAT`) minus "
    f"one call that enqueues one, over {a.reps}; {a.rounds} rounds.")
say()
say("| prefix | n | branch, us | decode, us | decode / branch | KiB read branch | KiB read decode |")
say("|---|---|---|---|---|---|---|")
gen = torch.Generator(device=dev).manual_seed(1234)
H, d, OWN, BP = 32, 128, 16, 64


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


for past in (96, 992):
  for n in (4, 16):
    pitch = (past + OWN + 1 + 31) // 32 * 32
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=gen).bfloat16()      # noqa: E731
    qkv = rnd(n, 3 * H * d)
    K, Vt = rnd(1, H, pitch, d), rnd(1, H, d, pitch)
    Kb, Vtb = rnd(n, H, BP, d), rnd(n, H, d, BP)
    Kn, Vn = rnd(n, H, pitch, d), rnd(n, H, d, pitch)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
    gs, gp, gl, lens = i32([0, n]), i32([0]), i32([past]), i32([past + OWN] * n)
    q, k, v = qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:]
    brn = lambda: ops.attention_branch(q, k, v, K, Vt, Kb, Vtb, gs, gp, gl, lens)      # noqa: E731
    qc, kc, vc = (t.contiguous() for t in (q, k, v))
    dcd = lambda: ops.attention_decode(qc, kc, vc, Kn, Vn, lens)      # noqa: E731
    res = []
    for run in (brn, dcd):
      for _ in range(3):
        run()
      res.append([(one_call(run, a.reps + 1) - one_call(run, 1)) / a.reps for _ in range(a.rounds)])
    kib_b = H * (past + n * OWN) * 2 * d * 2 / 1024
    kib_d = H * n * (past + OWN) * 2 * d * 2 / 1024
    say(f"| {past} | {n} | {spread(res[0])} | {spread(res[1])} | {statistics.mean(res[1]) / statistics.mean(res[0]):.2f} | {kib_b:.0f} | {kib_d:.0f} |")

say()
say("Not measured: several dialogues in one call, more than 32 branches per dialogue (several groups re-read the prefix once each), image "
    "contexts, fp8-weight handles, real checkpoints, `propose` (sample + score) end to end.")

if a.write:
  text = BEGIN + "\n" + "\n".join(lines) + "\n" + END
  old = open(a.write).read() if os.path.exists(a.write) else "# Branch decode: n replies per dialogue from one cached history\n"
  if BEGIN in old:
    i, j = old.index(BEGIN), old.index(END) + len(END)
    new = old[:i] + text + old[j:]
  else:
    new = old.rstrip("\n") + "\n\n" + text + "\n"
  with open(a.write, "w") as f:
    f.write(new)
  print("wrote", a.write)
