#!/usr/bin/env python3
"""The e4m3 KV cache timed beside the bf16 cache.
  python tools/kv8_decode_time.py [--rounds R] [--iters N] [--reps N] [--write [PATH]]      PATH: default profiles/kv8_decode.md
OPT-6.7b shapes with synthetic weights, load_sd=False, one process on one MI355X, B = 16.  Two handles per weight format live side by side, one
per cache format, and the arms alternate round by round; no dispatch between the arms exists or is added: the figures are reported whichever
way they fall.
1. The ragged decode iteration (gill_opt_decode_step + gill_opt_next_token_ragged, the loop of generate_batch with its one host read per
   iteration) at cached lengths of about 256, 1024 and 1900, on bf16 and on fp8 weights: wall ms over --iters iterations with a device
   synchronisation at both ends, divided by --iters - 1 (the first iteration is a decision without a decode step).  The cache holds zeros below each length (timing does not depend on the values); lengths grow by one per
   iteration.
2. The two attention operators alone beside their bf16 twins, H = 32, d = 128: device events around one call that enqueues --reps + 1 launches
   (GILL_OP_REPEAT) minus one call that enqueues one, over --reps.  Achieved bytes/s = the cache bytes the (b, h) pairs hold below their lengths
   (keys, values and, for e4m3, exponents) over that time: the bytes the algorithm needs, not a hardware counter.
3. One session turn at about 1000 tokens of history (tools/dialogue_session_time.py's turn 2): 16 rows extend by 12 .. 42 tokens and decode 30
   tokens; wall ms of the extend and of the decode loop."""
import argparse
import ctypes as C
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
ap.add_argument("--iters", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--write", nargs="?", const="profiles/kv8_decode.md", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
B, CAP = 16, 2048
lines = []


def say(s=""):
  print(s, flush=True)
  lines.append(s)


def spread(v, fmt=".2f"):
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
lib = N.lib()
D, vocab = m.opt_cfg.hidden_size, m.opt_cfg.vocab_size
KV = ("bf16", "fp8")


def make_handle(weights, kv):
  c = m.opt_cfg
  cfg = N.gill_opt_config(vocab_size=c.vocab_size, hidden_size=c.hidden_size, num_layers=c.num_layers, num_heads=c.num_heads, ffn_dim=c.ffn_dim,
                          max_positions=c.max_positions, max_batch=B, max_seq=CAP)
  arr, keep = N.make_tensor_table(m.lm.state_dict(), dev)
  h = C.c_void_p()
  N.check(lib.gill_opt_create_ex(C.byref(h), C.byref(cfg), arr, len(keep), 1 if weights == "fp8" else 0))
  N.check(lib.gill_opt_set_kv_format(h, 1 if kv == "fp8" else 0))
  return h


def adopt(h, weights, kv):
  """The model's entries run on this handle (the tool owns the handles: the model must neither rebuild nor destroy them)."""
  m._opt_handle, m._opt_cap, m.opt_weights, m.kv_cache = h, (B, CAP), weights, kv
  m._cache_epoch += 1


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  out = fn()
  torch.cuda.synchronize()
  return (time.time() - t0) * 1e3, out


def decode_iterations(h, n):
  """--iters iterations of the ragged loop from cached lengths of about n (0.9 .. 1.0 of it, a different length per row) -> ms per iteration."""
  L = a.iters
  lens = [round(n * (0.9 + 0.1 * b / (B - 1))) for b in range(B)]
  st = torch.zeros(6 * B + 1, dtype=torch.int32)
  st[0:B] = torch.tensor(lens, dtype=torch.int32) - 1
  st[4 * B:5 * B] = torch.arange(B, dtype=torch.int32)
  st[6 * B] = B
  st = st.to(dev)
  gen = torch.Generator(device=dev).manual_seed(7)
  hid = torch.randn((B, D), device=dev, generator=gen)
  steps = torch.zeros((L, B, D), device=dev, dtype=torch.float32)
  nxt = torch.zeros((B, D), device=dev, dtype=torch.bfloat16)
  logits = torch.empty((B, vocab), device=dev, dtype=torch.float32)
  tokens = torch.full((B, L), -1, device=dev, dtype=torch.int64)
  rule = m._decode_rule(0, L, 1.0, 1.0, -float("inf"))      # min_word_tokens = L: the [IMG] ids stay filtered, every iteration is one token
  ms, _ = timed(lambda: m._ragged_decode_loop(h, B, st, hid, steps, nxt, logits, tokens, rule, None, L, L, max(lens)))
  return ms / (L - 1)      # the first iteration is a decision without a decode step


say("# The e4m3 KV cache beside the bf16 cache: timings")
say()
say("`python tools/kv8_decode_time.py --write`: OPT-6.7b shapes (synthetic weights), `load_sd=False`, one process on one MI355X, B = 16.  Two handles")
say("per weight format, one per cache format, live side by side and the arms alternate round by round.  Figures as measured; nothing in the tests")
say("depends on them, and no dispatch between the arms exists.")
say()
say("## The ragged decode iteration")
say()
say(f"`gill_opt_decode_step` + `gill_opt_next_token_ragged` as `generate_batch` loops them (one 4-byte host read per iteration, one iteration late),")
say(f"{a.iters} iterations (wall / {a.iters - 1}: the first one has no decode step) from cached lengths of 0.9 .. 1.0 of the stated length (a different length per row); wall ms per iteration with a device")
say(f"synchronisation at both ends, mean (min .. max) of {a.rounds} rounds.  Cache bytes: what `gill_opt_kv_bytes` reports for 16 x 2048 slots.")
say()
say("| weights | cached length | bf16 cache, ms | e4m3 cache, ms | bf16 / e4m3 (means) |")
say("|---|---|---|---|---|")
session_rows = []
for weights in ("bf16", "fp8"):
  hs = {kv: make_handle(weights, kv) for kv in KV}
  for n in (256, 1024, 1900):
    for kv in KV:
      decode_iterations(hs[kv], n)      # warm-up: the cache allocation, kernels, allocator
    res = {kv: [] for kv in KV}
    for _ in range(a.rounds):
      for kv in KV:
        res[kv].append(decode_iterations(hs[kv], n))
    say(f"| {weights} | {n} | {spread(res['bf16'])} | {spread(res['fp8'])} | {statistics.mean(res['bf16']) / statistics.mean(res['fp8']):.2f} |")
  bytes_ = {kv: lib.gill_opt_kv_bytes(hs[kv]) for kv in KV}
  if weights == "bf16":
    # one session turn at about 1000 tokens of history, on the same two handles
    first = [round(1000 * (0.8 + 0.4 * b / (B - 1))) for b in range(B)]
    later = [12 + 2 * ((b + 5) % B) for b in range(B)]
    ids = lambda n, s: (3 + (torch.arange(n) * 7919 + s * 104729) % 40000).tolist()      # noqa: E731
    kw = dict(max_len=30, min_word_tokens=30)

    def turn(kv):
      adopt(hs[kv], weights, kv)
      s = m.open_session(B, CAP)
      s.extend(list(range(B)), ids=[[2] + ids(first[b] - 1, b) for b in range(B)])
      s.generate(None, **kw)
      t_ext, _ = timed(lambda: s.extend(list(range(B)), ids=[ids(later[b], 100 + b) for b in range(B)]))
      t_dec, _ = timed(lambda: s.generate(None, **kw))
      return t_ext, t_dec

    for kv in KV:
      turn(kv)
    tr = {kv: [] for kv in KV}
    for _ in range(a.rounds):
      for kv in KV:
        tr[kv].append(turn(kv))
    for i, name in enumerate(("extend (12 .. 42 new tokens per row, packed)", "decode loop (30 iterations)")):
      x, y = [t[i] for t in tr["bf16"]], [t[i] for t in tr["fp8"]]
      session_rows.append(f"| {name} | {spread(x, '.1f')} | {spread(y, '.1f')} | {statistics.mean(x) / statistics.mean(y):.2f} |")
    m._opt_handle, m._opt_cap, m.kv_cache = None, (0, 0), "bf16"
  for h in hs.values():
    lib.gill_opt_destroy(h)
  torch.cuda.empty_cache()
say()
say(f"Cache held by a handle of 16 rows x 2048 slots: bf16 {bytes_['bf16'] / 2 ** 30:.2f} GiB, e4m3 {bytes_['fp8'] / 2 ** 30:.2f} GiB.")
say()
say("## One session turn at about 1000 tokens of history (bf16 weights)")
say()
say("`GILLModel.open_session`, 16 rows: turn 1 brings 800 .. 1200 tokens and decodes 30; the timed turn 2 extends every row by 12 .. 42 tokens")
say(f"(`gill_opt_extend`, one packed call) and decodes 30 tokens.  Wall ms, device synchronisation at both ends, {a.rounds} rounds, arms alternating.")
say()
say("| part of turn 2 | bf16 cache, ms | e4m3 cache, ms | bf16 / e4m3 (means) |")
say("|---|---|---|---|")
for r in session_rows:
  say(r)

say()
say("## The attention operators alone")
say()
say(f"B = 16, H = 32, d = 128.  Device events around one call that enqueues {a.reps} + 1 launches (`GILL_OP_REPEAT`) minus one call that enqueues one,")
say(f"over {a.reps}; {a.rounds} rounds.  TB/s: the cache bytes below the lengths (keys, values, and for e4m3 the exponents) over that time: bytes")
say("the algorithm needs, not a hardware counter.  The extend figures include the store launch; a (b, h) pair's cache is read once per 32 queries.")
say()
say("| operator | cached length | new tokens per row | bf16 cache, us | TB/s | e4m3 cache, us | TB/s | bf16 / e4m3 |")
say("|---|---|---|---|---|---|---|---|")
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


for name, past, cnt in (("decode", 256, 1), ("decode", 1024, 1), ("decode", 1900, 1), ("extend", 1024, 32), ("extend", 0, 1024)):
  pitch = (past + cnt + 31) // 32 * 32
  rnd = lambda *shape: torch.randn(shape, device=dev, generator=gen).bfloat16()      # noqa: E731
  qkv = rnd(B * cnt, 3 * H * d)
  q, k, v = qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:]
  K, Vt = rnd(B, H, pitch, d), rnd(B, H, d, pitch)
  # every byte below 0x78: finite codes; exponents of -7 (the rows of a unit-variance cache)
  K8 = torch.randint(0, 0x78, (B, H, pitch, d), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
  Vt8 = torch.randint(0, 0x78, (B, H, d, pitch), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
  Ke, Ve = (torch.full((B, H, pitch), -7, dtype=torch.int8, device=dev) for _ in range(2))
  lens = torch.full((B,), past, dtype=torch.int32, device=dev)
  cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * cnt
  if name == "decode":
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    runs = (lambda: ops.attention_decode(qc, kc, vc, K, Vt, lens), lambda: ops.attention_decode_kv8(qc, kc, vc, K8, Vt8, Ke, Ve, lens))
  else:
    runs = (lambda: ops.attention_extend(q, k, v, K, Vt, lens, cu, cnt), lambda: ops.attention_extend_kv8(q, k, v, K8, Vt8, Ke, Ve, lens, cu, cnt))
  nkeys = past + (cnt if name == "extend" else 0)
  nbytes = (B * H * nkeys * 2 * d * 2, B * H * nkeys * (2 * d + 2))
  res = []
  for run in runs:
    for _ in range(3):
      run()
    res.append([(one_call(run, a.reps + 1) - one_call(run, 1)) / a.reps for _ in range(a.rounds)])
  tb = [nbytes[i] / (statistics.mean(res[i]) * 1e-6) / 1e12 for i in range(2)]
  say(f"| {name} | {past} | {cnt} | {spread(res[0], '.1f')} | {tb[0]:.2f} | {spread(res[1], '.1f')} | {tb[1]:.2f} | "
      f"{statistics.mean(res[0]) / statistics.mean(res[1]):.2f} |")
say()
say("Not measured: real OPT checkpoints (the weights are synthetic), more than one GPU, batch sizes other than 16.")
if a.write:
  with open(a.write, "w") as f:
    f.write("\n".join(lines) + "\n")
  print("wrote", a.write)
