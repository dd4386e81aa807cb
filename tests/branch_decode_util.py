"""Shared by test_branch_host.py, test_branch_decode_gpu.py and tools/branch_decode_tolerance.py (not a test module): the seeded branch-decode
run those tests make, and the fp32 oracle's own run of it.

The rig is that of the session tests (ragged_decode_util.gen_model: OPT-125m geometry, synth.opt_state_dict seed 5; B = 4 rows, capacity 128).
Rows ROWS of a session hold histories of LENGTHS tokens (synthetic ids, <bos> first); session.sample draws N replies of MAX_LEN tokens per row at
TEMPERATURE with top_p = 1 and the default rule, branch j of row r keyed (sample seed, r * N + j, decision).  A seeded decision is
argmax_c (y_c - log(-log u_c)), y = logits / temperature, u the Philox uniforms of gill_decode_uniforms: two arithmetic paths can part where the
two largest of those DECISION KEYS are near each other.  (The synthetic model's logits are peaked: at temperature 1 every branch draws the same
token, and at 6 no seed keeps forty decisions clear of the bar.  Siblings part exactly where two keys are close, so at TEMPERATURE a prompt that
is clear of the bar and still gives its row more than one reply is rare: the tool records the rows that have one, at least one.)  The bar m for "near" is MARGIN x the largest distance between the decision keys of the bf16-operand emulation (kv_cache_util.cached_forward_ref, every GEMM operand rounded) and the fp32 oracle's over the oracle's own sampled run
(the uniforms are common to both, so that distance is the logits' over the temperature).  tools/branch_decode_tolerance.py measures it and
chooses the rows' prompt seeds (per row, at one sampling seed) so that no decision of the oracle's run has a top-2 key margin under m and none picks an [IMG] token; it
also checks the greedy decisions that follow the adopted replies (ADOPT) against the session test's own bar."""
import ctypes as C
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import kv_cache_util as U
import ragged_decode_util as R
from gill_amd import synth

B = 4
CAPACITY = 128
ROWS = (0, 2)
LENGTHS = (33, 70)
N = 4
MAX_LEN = 5
TEMPERATURE = 1.5
MARGIN = 10.0                        # the session test's: m = MARGIN x the emulation's distance
EXCUSED_SHARE = 0.10                 # of the branches a near tie may excuse
ADOPT = ((0, 1, None), (2, 3, 3))    # (row, branch index, keep) the GPU test adopts
TOLERANCE_FILE = "branch_decode_tolerance.json"       # under tests/golden


def golden():
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)
  with open(path) as f:
    return json.load(f)


def prompt_ids(row, n, seed):
  return synth.synthetic_prompt_ids(B, n, seed=seed)[row, :n].tolist()


def uniforms(seed, key, draw, V):
  from gill_amd import _native as Nat
  out = (C.c_float * V)()
  Nat.check(Nat.lib().gill_decode_uniforms(seed, key, draw, 0, V, out))
  return torch.from_numpy(np.frombuffer(out, dtype=np.float32, count=V).copy())


def decision_keys(logits, seed, key, draw, temperature=None):
  """(V,) fp32 logits -> the keys whose argmax the seeded draw takes (top_p = 1: every id is kept)."""
  temperature = TEMPERATURE if temperature is None else temperature
  u = uniforms(seed, key, draw, logits.numel()).double()
  return logits.double() / temperature - torch.log(-torch.log(u))


def oracle_sampled(sd, cfg, hist, seed, key, n_dec=MAX_LEN, temperature=None):
  """The fp32 oracle's own seeded run of one branch -> (tokens, top-2 key margins, the emulation's largest key distance)."""
  temperature = TEMPERATURE if temperature is None else temperature
  from oracle import opt_ref
  ids = [int(v) for v in hist]
  toks, margins, dist = [], [], 0.0
  table = sd["model.decoder.embed_tokens.weight"].float()
  for i in range(n_dec):
    x = F.embedding(torch.tensor(ids)[None], table)
    h = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, x)[0, -1]
    logits = opt_ref.opt_logits(sd, h[None])[0]
    (he,), _ = U.cached_forward_ref(sd, cfg, x, (len(ids),), rnd=U.bf)
    dist = max(dist, (opt_ref.opt_logits(sd, U.bf(he[0, -1])[None])[0] - logits).abs().max().item() / temperature)
    top = decision_keys(logits, seed, key, i, temperature).topk(2)
    toks.append(int(top.indices[0]))
    margins.append(float(top.values[0] - top.values[1]))
    ids.append(toks[-1])
  return toks, margins, dist


def oracle_row(r, n, prompt_seed, sample_seed, temperature=None):
  """One row of the test on the oracle -> dict(branches {(row, j): (tokens, margins)}, dist, margin, img: an [IMG] id was picked, distinct: the
  row's branches drew more than one reply, greedy_margin / greedy_dist: the smallest top-2 margin and the largest distance of the greedy
  decisions after the row's adopted reply)."""
  cfg, sd = R.gen_model()
  out = dict(branches={}, dist=0.0, margin=float("inf"), img=False, greedy_margin=float("inf"), greedy_dist=0.0)
  hist = prompt_ids(r, n, prompt_seed)
  for j in range(N):
    toks, margins, d = oracle_sampled(sd, cfg, hist, sample_seed, r * N + j, temperature=temperature)
    out["branches"][(r, j)] = (toks, margins)
    out["dist"], out["margin"] = max(out["dist"], d), min(out["margin"], min(margins))
    out["img"] = out["img"] or any(t in synth.IMG_TOKEN_IDS for t in toks)
  out["distinct"] = len({tuple(out["branches"][(r, j)][0]) for j in range(N)}) > 1
  for row, j, keep in ADOPT:
    if row == r:
      reply = out["branches"][(r, j)][0]
      _, gm, _, gd = R.oracle_greedy(sd, cfg, hist + (reply if keep is None else reply[:keep]))
      out["greedy_margin"], out["greedy_dist"] = min(out["greedy_margin"], min(gm)), max(out["greedy_dist"], gd)
  return out


def oracle_run(prompt_seeds, sample_seed, temperature=None):
  """The whole run of the test on the oracle: oracle_row of every row (prompt_seeds: {row: seed}), merged."""
  runs = [oracle_row(r, n, int(prompt_seeds[r]), sample_seed, temperature) for r, n in zip(ROWS, LENGTHS)]
  out = dict(branches={}, dist=max(x["dist"] for x in runs), margin=min(x["margin"] for x in runs), img=any(x["img"] for x in runs),
             distinct=all(x["distinct"] for x in runs), greedy_margin=min(x["greedy_margin"] for x in runs),
             greedy_dist=max(x["greedy_dist"] for x in runs))
  for x in runs:
    out["branches"].update(x["branches"])
  return out


def prompt_seeds(gold):
  return {int(k): int(v) for k, v in gold["prompt_seeds"].items()}
