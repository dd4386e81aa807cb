#!/usr/bin/env python3
"""The bars of tests/test_kv8_engine_gpu.py and the quality of the e4m3 KV cache, measured on the CPU (tests/kv8_util.py).
  python tools/kv8_tolerance.py [--write] [--no-quality]

1. The hidden-state bar and the near-tie bar.  A one-ulp bf16 difference in a K or V element can flip an e4m3 code, so the device's run of the
   quantised-cache model and the CPU's differ by more than accumulation order.  Measured: the distance between the bf16-storage fp32 emulation
   (every GEMM operand and the extend rows' P rounded to bf16, kv8_util.kv8_forward(rnd=bf)) and the fp64 run of the same quantised model, over
   the decision rows of the fp64 model's own greedy runs of the test's inputs: the ragged batch at lengths (30, 23, 9) on bf16 and on fp8
   weights, and the three-turn session plan.  hid_bar = 4 x the largest per-row rel-L2 distance of hidden rows, m_logit = 4 x the largest logit
   distance (4 x: the margin the w8 tests give an honest emulation).
2. The prompts: per row of the batch, and per (turn, row) of the session plan the first seed of the row's new ids, at which the fp64
   model's own decisions have no top-2 margin under m_logit (the choice and the bars depend on each other: repeated until both stand).
3. Quality on SYNTHETIC weights (no real OPT checkpoint is at hand): last hidden states of the quantised-cache model against the unquantised
   fp32 oracle on the opt125 and the 2-layer opt67 geometries.  Recorded, asserted nowhere.
--write stores the bars and seeds in tests/golden/kv8_tolerance.json and the report in profiles/kv8.md."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch   # noqa: E402
from gill_amd import synth   # noqa: E402
from gill_amd.synth import host_cores   # noqa: E402
import dialogue_session_util as S   # noqa: E402
import kv8_util as K   # noqa: E402
import kv_cache_util as U   # noqa: E402
from oracle import opt_ref   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--write", action="store_true")
ap.add_argument("--no-quality", action="store_true")
ap.add_argument("--tries", type=int, default=120)
a = ap.parse_args()
torch.set_num_threads(host_cores())
PLAN = "three"
memo = {}


models = {}


def run(weights, ids, n_dec, emulate=True):
  key = (weights, tuple(int(v) for v in ids), n_dec, emulate)
  if key not in memo:
    if weights not in models:
      models[weights] = K.model(weights)
    cfg, sd = models[weights]
    memo[key] = K.greedy_ref(sd, cfg, ids, n_dec=n_dec, emulate=emulate)
  return memo[key]


def choose(m):
  """One pass with the near-tie bar m -> (batch seed, session seeds, largest hidden distance, largest logit distance, smallest margin, decisions)."""
  stat = dict(hid=0.0, logit=0.0, margin=float("inf"), n=0)

  def note(r):
    stat.update(hid=max(stat["hid"], r["hid_dist"]), logit=max(stat["logit"], r["logit_dist"]), margin=min(stat["margin"], min(r["margins"])),
                n=stat["n"] + len(r["margins"]))

  # the batch: per row the first seed at which the row's decisions are clear of the bar on bf16 and on fp8 weights (screened without the
  # emulation first: most seeds fall at their first decision)
  batch = []
  for b in range(len(K.LENGTHS)):
    for s in range(K.SEED, K.SEED + a.tries):
      ids = K.prompt_row(b, s)
      if min(min(run(w, ids, K.N_DEC, False)["margins"]) for w in ("bf16", "fp8")) < m:
        continue
      runs = [run(w, ids, K.N_DEC) for w in ("bf16", "fp8")]
      if min(min(r["margins"]) for r in runs) >= max(m, K.MARGIN * max(r["logit_dist"] for r in runs)):
        batch.append(s)
        for r in runs:
          note(r)
        break
    else:
      sys.exit(f"no seed found for batch row {b}")
  seed = batch
  seeds = {}

  def ids_of(turn, row, n, hist):
    for s in range(S.SEED, S.SEED + a.tries):
      ids = S.new_ids(turn, row, n, first=not hist, seed=s)
      if min(run("bf16", hist + ids, 3, False)["margins"]) < max(m, 1.0):
        continue
      r = run("bf16", hist + ids, 3)
      if min(r["margins"]) >= max(m, K.MARGIN * r["logit_dist"]):
        seeds[(turn, row)] = s
        return ids
    sys.exit(f"no seed found for turn {turn} row {row}")

  def decode(turn, row, hist):
    r = run("bf16", hist, 3)
    note(r)
    return r["tokens"] + synth.IMG_TOKEN_IDS * 2

  S.walk(S.PLANS[PLAN], {}, decode, ids_of=ids_of)
  return seed, seeds, stat


m = 0.0
for rnd in range(6):
  seed, seeds, stat = choose(m)
  m = K.MARGIN * stat["logit"]
  ok = stat["margin"] >= m
  print(f"pass {rnd}: batch seeds {seed}; largest hidden distance {stat['hid']:.3e}, largest logit distance {stat['logit']:.3e}, m_logit = "
        f"{K.MARGIN:g} x = {m:.3e}; smallest top-2 margin of the reference's {stat['n']} decisions {stat['margin']:.3e} "
        f"({'ok' if ok else 'under m: again with this m'})")
  if ok:
    break
else:
  sys.exit("the choice did not settle")
hid_bar = K.MARGIN * stat["hid"]
table = {f"{t},{r}": s for (t, r), s in sorted(seeds.items())}
print(f"hid_bar = {K.MARGIN:g} x {stat['hid']:.3e} = {hid_bar:.3e}; session seeds {table}")

lines = ["# The e4m3 KV cache (kv8): bars and quality", "", "`python tools/kv8_tolerance.py --write` (CPU).", "",
         "## Bars of `tests/test_kv8_engine_gpu.py`", "",
         "Distance between the bf16-storage fp32 emulation (`kv8_util.kv8_forward(rnd=bf)`) and the fp64 run of the same quantised-cache model,",
         f"over the decision rows of the fp64 model's own greedy runs: the ragged batch at lengths {tuple(K.LENGTHS)} ({K.N_DEC} decisions per row, on",
         f"bf16 and on fp8 weights) and the session plan `{PLAN}` (3 free decisions per row and turn); {stat['n']} decisions in all.", "",
         "| figure | largest distance | bar = 4 x |", "|---|---|---|",
         f"| hidden rows, per-row rel-L2 | {stat['hid']:.3e} | **{hid_bar:.3e}** |",
         f"| logits, largest absolute difference | {stat['logit']:.3e} | **{m:.3e}** |", "",
         f"Batch seeds {seed} (one per row); session seeds {table}.  Smallest top-2 margin of the reference's own decisions on these prompts: {stat['margin']:.4f}",
         "(above m_logit: the reference alone needs no excusal).  `tests/test_kv8_host.py` asserts that all six defects of `kv8_util.DEFECTS` miss the operator bar by 3 x or more, and that the three",
         "which break the engine whatever the operands are (scale dropped, exponent read as unsigned, stale exponent visible) miss the hidden bar by 3 x",
         "or more (11.8 x and up).  The hidden bar does NOT separate the other three on this rig (worst row: neighbour's scale 2.0 x, V scale on K 1.5 x,",
         "own token unquantised 0.24 x of the bar): the model's neighbouring rows share their exponents within one, and the bar has to admit e4m3 code",
         "flips between honest runs.  Those three are separated by the operator tests' inputs (exponents that differ from slot to slot; `tie_operands`).", ""]

if not a.no_quality:
  lines += ["## Quality of the quantised cache (CPU, SYNTHETIC weights)", "",
            "Last hidden states of the model with e4m3-rounded keys and values (`kv8_forward`, fp32, nothing else rounded) against the fp32 oracle",
            "with the unquantised cache, 4 sequences of 48 tokens, peaked attention (`kv_cache_util.peaked_opt_state_dict`).", "",
            "| geometry | rel-L2 | cosine |", "|---|---|---|"]
  for geom in ("opt125", "opt67"):
    g = U.GEOMETRIES[geom]
    cfg = g["cfg"]
    sd = U.peaked_opt_state_dict(cfg, g["seed"])
    x = U.token_embeds(sd, cfg, 4, 48, g["seed"] + 1)
    ref = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, x)
    got = K.kv8_forward(sd, cfg, x)
    rel = ((got - ref).norm() / ref.norm()).item()
    cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
    print(f"{geom} ({cfg.num_layers} layers): rel-L2 {rel:.3e} cosine {cos:.6f}")
    lines.append(f"| {geom} ({cfg.num_layers} layers, D = {cfg.hidden_size}) | {rel:.3e} | {cos:.6f} |")
  lines += ["", "These figures come from synthetic weights (`gill_amd.synth`); real OPT checkpoints were not available.  They are asserted nowhere.", ""]

if a.write:
  path = os.path.join(ROOT, "tests", "golden", K.TOLERANCE_FILE)
  with open(path, "w") as f:
    json.dump({"hid_bar": hid_bar, "m_logit": m, "largest_hidden_distance": stat["hid"], "largest_logit_distance": stat["logit"],
               "smallest_reference_margin": stat["margin"], "seeds": seed, "plan": PLAN, "session_seeds": table}, f, indent=1)
    f.write("\n")
  print("wrote", path)
  prof = os.path.join(ROOT, "profiles", "kv8.md")
  with open(prof, "w") as f:
    f.write("\n".join(lines))
  print("wrote", prof)
