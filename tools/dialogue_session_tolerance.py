#!/usr/bin/env python3
"""The near-tie bar m of tests/test_dialogue_session_gpu.py, measured on the CPU, on the recipe of tools/ragged_decode_tolerance.py: 10 x the
largest distance between the logits of a bf16-operand emulation of the kernels' arithmetic (kv_cache_util.cached_forward_ref with every GEMM
operand rounded) and the fp32 oracle's, over the decision rows of the oracle's own greedy run of the test's multi-turn sessions
(tests/dialogue_session_util.py: the plans' concatenated prompts).  It also chooses the prompts: per (turn, row) the first seed of the row's
new ids at which the oracle's three decisions have no top-2 margin under m (later turns decode from histories that hold the oracle's earlier
tokens, so the choice runs in plan order).
  python tools/dialogue_session_tolerance.py [--write]
--write stores m and the seeds in tests/golden/dialogue_session_tolerance.json (the tests read both)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch   # noqa: E402
from gill_amd.synth import host_cores   # noqa: E402
import dialogue_session_util as S   # noqa: E402
import ragged_decode_util as R   # noqa: E402
from gill_amd import synth   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--write", action="store_true")
ap.add_argument("--tries", type=int, default=40)
a = ap.parse_args()
torch.set_num_threads(host_cores())

cfg, sd = R.gen_model()
memo = {}


def run(hist):
  key = tuple(hist)
  if key not in memo:
    memo[key] = R.oracle_greedy(sd, cfg, hist)
  return memo[key]


def choose(m):
  """One pass over the plans with the bar m: per (turn, row) the first seed whose three decisions are all clear of max(m, 10 x their own
  distance).  The plans share their first turn, so "three" takes the seeds "two" got there.  -> (seeds, largest distance, smallest margin, n)."""
  seeds, stat = {name: {} for name in S.PLANS}, dict(dist=0.0, margin=float("inf"), n=0)
  for name, plan in S.PLANS.items():
    def ids_of(turn, row, n, hist, name=name):
      shared = seeds["two"].get((turn, row)) if name != "two" and turn == 0 else None
      for s in ([shared] if shared is not None else range(S.SEED, S.SEED + a.tries)):
        ids = S.new_ids(turn, row, n, first=not hist, seed=s)
        _, margins, _, d = run(hist + ids)
        if min(margins) >= max(m, 10 * d):
          seeds[name][(turn, row)] = s
          return ids
      sys.exit(f"no seed found for plan {name} turn {turn} row {row}")

    def decode(turn, row, hist):
      toks, margins, _, d = run(hist)
      stat.update(dist=max(stat["dist"], d), margin=min(stat["margin"], min(margins)), n=stat["n"] + len(margins))
      return toks + synth.IMG_TOKEN_IDS * 2

    S.walk(plan, {}, decode, ids_of=ids_of)
  return seeds, stat["dist"], stat["margin"], stat["n"]


# m depends on the largest distance over the chosen prompts, and the choice on m: repeat until both stand
m = 0.0
for rnd in range(6):
  seeds, dist, margin, n_dec = choose(m)
  m = 10 * dist
  print(f"pass {rnd}: largest logit distance bf16 emulation vs fp32 oracle {dist:.3e}, m = 10 x = {m:.3e}; smallest top-2 margin of the "
        f"oracle's {n_dec} decisions {margin:.3e} ({'ok' if margin >= m else 'under m: again with this m'})")
  if margin >= m:
    break
else:
  sys.exit("the choice did not settle")
table = {name: {f"{t},{r}": s for (t, r), s in sorted(tab.items())} for name, tab in seeds.items()}
print(table)
if a.write:
  path = os.path.join(ROOT, "tests", "golden", S.TOLERANCE_FILE)
  with open(path, "w") as f:
    json.dump({"m": m, "largest_logit_distance": dist, "smallest_oracle_margin": margin, "seeds": table}, f, indent=1)
    f.write("\n")
  print("wrote", path)
