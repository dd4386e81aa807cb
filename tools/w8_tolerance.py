#!/usr/bin/env python3
"""The bar of the w8 operator test (tests/test_w8_ops_gpu.py) and the quality of the quantised model, measured on the CPU.
  python tools/w8_tolerance.py [--write] [--no-quality]

1. The accumulation distance: an fp32 emulation of linear_w8_kernel's sum (bf16 operands, fp32 accumulation, K in the kernel's permuted and
   split order; tests/w8_util.emulate_linear) against fp64 on the same operands, as the largest |difference| / sum_k |a| |w| over the
   operator test's own shapes and row counts.  tests/w8_util.W8_ACC_DIST holds it; the operator bar is 10 x that.
2. Model quality on SYNTHETIC weights (no real OPT checkpoint is at hand): the last hidden states of the quantised model against the
   unquantised one (the fp32 oracle on sd against w8_state_dict(sd)) on the opt125 and opt67 geometries, and the share of greedy decisions
   that agree over the prompts of ragged_decode_util.gen_prompt_ids.  Recorded, not asserted anywhere.
--write replaces the "tolerance" section of profiles/w8_decode.md."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kv_cache_util as U          # noqa: E402
import ragged_decode_util as R     # noqa: E402
import w8_util as W                # noqa: E402
from oracle import opt_ref         # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "w8_decode.md")


def write_section(name, lines):
  """Replace (or append) the block between <!-- name:begin --> and <!-- name:end --> of profiles/w8_decode.md."""
  begin, end = f"<!-- {name}:begin -->", f"<!-- {name}:end -->"
  text = open(PROFILE).read() if os.path.exists(PROFILE) else "# The weight-only fp8 decoder (w8): bars, timings, quality\n"
  block = "\n".join([begin] + lines + [end])
  if begin in text and end in text:
    text = text[:text.index(begin)] + block + text[text.index(end) + len(end):]
  else:
    text = text.rstrip("\n") + "\n\n" + block + "\n"
  with open(PROFILE, "w") as f:
    f.write(text)
  print("wrote", PROFILE)


def accumulation(lines):
  worst = 0.0
  lines += ["## Accumulation distance (CPU)", "", "`python tools/w8_tolerance.py --write`: fp32 emulation of the kernel's sum against fp64 on the same",
            "operands, largest |difference| / (sum_k |a||w| + |bias| + |resid|).", "", "| N | K | slices | M | distance |", "|---|---|---|---|---|"]
  for ci, (N, K, sk) in enumerate(W.OP_CASES):
    for M in sorted(set(W.OP_ROWS)):
      d = W.acc_distance(N, K, M, sk, seed=100 + ci)
      worst = max(worst, d)
      print(f"N={N} K={K} slices={sk or W.pick_splitk(N, K)} M={M}: {d:.3e}")
      lines.append(f"| {N} | {K} | {sk or W.pick_splitk(N, K)} | {M} | {d:.3e} |")
  lines += ["", f"Largest: **{worst:.3e}** (`tests/w8_util.W8_ACC_DIST = {W.W8_ACC_DIST:.3e}`); operator bar = 10 x = {10 * worst:.3e} of the magnitude,",
            "plus half a bf16 ulp of the result for bf16 outputs.", ""]
  print(f"largest distance {worst:.3e}; tests/w8_util.W8_ACC_DIST = {W.W8_ACC_DIST:.3e}; bar = 10 x")
  return worst


def quality(lines):
  lines += ["## Quality of the quantised model (CPU oracle, SYNTHETIC weights)", "",
            "Last hidden states of the fp32 oracle on `w8_state_dict(sd)` against the oracle on `sd`, 4 sequences of 48 tokens.", "",
            "| geometry | rel-L2 | cosine |", "|---|---|---|"]
  for geom in ("opt125", "opt67"):
    g = U.GEOMETRIES[geom]
    cfg = g["cfg"]
    sd = U.peaked_opt_state_dict(cfg, g["seed"])
    x = U.token_embeds(sd, cfg, 4, 48, g["seed"] + 1)
    a = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, x)
    b = opt_ref.opt_hidden_states(W.w8_state_dict(sd, cfg), cfg.num_layers, cfg.num_heads, x)
    rel = ((a - b).norm() / a.norm()).item()
    cos = torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()
    print(f"{geom} ({cfg.num_layers} layers): rel-L2 {rel:.3e} cosine {cos:.6f}")
    lines.append(f"| {geom} ({cfg.num_layers} layers, D = {cfg.hidden_size}) | {rel:.3e} | {cos:.6f} |")
  cfg, sd = R.gen_model()
  sdq = W.w8_state_dict(sd, cfg)
  ids, lens = R.gen_prompt_ids()
  agree = total = 0
  small = float("inf")
  for b, n in enumerate(lens):
    ta, _, _, _ = R.oracle_greedy(sd, cfg, ids[b, :n])
    tb, mb, _, _ = R.oracle_greedy(sdq, cfg, ids[b, :n])
    # decisions are compared while the two runs still share their prefix
    for x, y in zip(ta, tb):
      total += 1
      agree += int(x == y)
      if x != y:
        break
    small = min(small, min(mb))
  print(f"greedy decisions that agree (oracle on sd vs on w8_state_dict(sd), gen_prompt_ids): {agree} of {total}")
  lines += ["", f"Greedy decisions of the oracle that agree between the two models over the `gen_prompt_ids` runs (OPT-125m geometry, {len(lens)} rows x "
            f"{R.GEN_MWT} decisions, compared while the prefixes agree): **{agree} of {total}**.",
            f"Smallest top-2 margin of the quantised oracle's own decisions: {small:.4f} (near-tie bar m = {R.load_gen_tolerance():.4f}).", "",
            "These figures come from synthetic weights (`gill_amd.synth`); real OPT checkpoints were not available.", ""]


def generate_margin(lines, write, first_seed, tries=20):
  """tools/ragged_decode_tolerance.py's method on the dequantised weights: m = 10 x the largest logit distance between the bf16-operand
  emulation and the fp32 oracle over the oracle's own greedy decisions, and the first prompt seed whose decisions all have a top-2 margin
  of m or more -> tests/golden/w8_generate_tolerance.json (tests/test_w8_generate_gpu.py)."""
  import json
  cfg, sd = R.gen_model()
  sdq = W.w8_state_dict(sd, cfg)
  for seed in range(first_seed, first_seed + tries):
    ids, lens = R.gen_prompt_ids(seed)
    runs = [R.oracle_greedy(sdq, cfg, ids[b, :n]) for b, n in enumerate(lens)]
    dist, margin = max(r[3] for r in runs), min(min(r[1]) for r in runs)
    m = 10 * dist
    print(f"seed {seed}: logit distance {dist:.3e}, m = {m:.3e}, smallest margin {margin:.3e} ({'ok' if margin >= m else 'under m: next seed'})")
    if margin >= m:
      break
  else:
    sys.exit("no seed found")
  lines += ["## Near-tie bar of the generate test (CPU)", "",
            f"On `w8_state_dict` of the `gen_model` weights the prompts of seed {R.GEN_SEED} have an oracle decision under the standing bar, so the",
            f"bar is re-measured by `tools/ragged_decode_tolerance.py`'s method: seed {seed}, largest logit distance {dist:.4f}, m = {m:.4f},",
            f"smallest top-2 margin of the oracle's decisions {margin:.4f} (`tests/golden/w8_generate_tolerance.json`).", ""]
  if write:
    path = os.path.join(ROOT, "tests", "golden", "w8_generate_tolerance.json")
    with open(path, "w") as f:
      json.dump({"m": m, "largest_logit_distance": dist, "seed": seed, "smallest_oracle_margin": margin}, f, indent=1)
      f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--no-quality", action="store_true")
  ap.add_argument("--first-seed", type=int, default=R.GEN_SEED)
  a = ap.parse_args()
  torch.manual_seed(0)
  lines = []
  accumulation(lines)
  if not a.no_quality:
    quality(lines)
    generate_margin(lines, a.write, a.first_seed)
  if a.write:
    write_section("tolerance", lines)
