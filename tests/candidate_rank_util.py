"""Shared by test_opt_score_candidates_gpu.py, test_candidate_rank_gpu.py, test_candidate_rank_host.py and tools/candidate_rank_tolerance.py
(not a test module): the inputs, the fp32 oracle and the bf16-operand emulation of candidate ranking on the OPT-125m synthetic rig
(ragged_decode_util.gill125_rig / gen_model).

Four dialogues with histories of HISTORIES tokens (context seeds 900 + i) and, per dialogue, ten candidates of COUNTS tokens (candidate seeds
1000 + 37 i + j), all through synth.synthetic_prompt_ids.  THE REFERENCE is oracle.opt_ref on every history + candidate alone: the candidate's
token log-probabilities log_softmax(lm_head(hidden))[token] at the positions that predict its tokens, and their mean.  The emulation restates the
scoring pass with bf16 operands: [history cached | last history token + candidate] through kv_cache_util.cached_forward_ref(rnd=bf), the hidden
rows rounded before the head (tools/lm_loss_tolerance.py term (b)).  The bars are 4 x the emulation's distances from the oracle
(tools/candidate_rank_tolerance.py --write -> tests/golden/candidate_rank_tolerance.json), that file's margin and reasoning."""
import json
import os

import torch
import torch.nn.functional as F

import kv_cache_util as K
import ragged_decode_util as R
from gill_amd import synth
from oracle import opt_ref

HISTORIES = (70, 33, 1, 31)
COUNTS = (1, 2, 7, 8, 9, 16, 31, 32, 33, 40)
TOLERANCE_FILE = "candidate_rank_tolerance.json"       # under tests/golden
LEFT_OUT_CAP = 0.10                                    # share of a dialogue's candidate pairs the ranking test may leave out
MARGIN = 4.0

_MEMO = {}


def history_ids(i):
  n = HISTORIES[i]
  return [int(v) for v in synth.synthetic_prompt_ids(1, n, seed=900 + i)[0, :n].tolist()]          # <bos> first


def candidate_ids(i, j):
  n = COUNTS[j]
  # the generator's rows as they are: a candidate's first id is the generator's leading 2, which is scored like any other token
  return [int(v) for v in synth.synthetic_prompt_ids(1, n, seed=1000 + 37 * i + j)[0, :n].tolist()]


def all_candidates():
  return [[candidate_ids(i, j) for j in range(len(COUNTS))] for i in range(len(HISTORIES))]


def _token_logprobs(sd, hidden, cand):
  """hidden (len(cand), D): the rows that predict cand's tokens -> their log-probabilities (len(cand),)."""
  lp = F.log_softmax(opt_ref.opt_logits(sd, hidden).float(), dim=-1)
  return lp[torch.arange(len(cand)), torch.tensor(cand)]


def oracle_candidate(sd, cfg, hist, cand):
  """The fp32 oracle on history + candidate alone -> the candidate's token log-probabilities."""
  x = opt_ref.opt_embed(sd, torch.tensor(hist + cand)[None])
  h = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, x)[0]
  return _token_logprobs(sd, h[len(hist) - 1:len(hist) + len(cand) - 1], cand)


def emulated_candidate(sd, cfg, hist, cand):
  """The scoring pass with bf16 operands: the history but its last token cached, then [last history token | candidate] against that cache."""
  x = opt_ref.opt_embed(sd, torch.tensor(hist + cand)[None])
  sched = (len(hist) - 1, 1 + len(cand)) if len(hist) > 1 else (len(hist) + len(cand),)
  outs, _ = K.cached_forward_ref(sd, cfg, x, sched, rnd=K.bf)
  h = K.bf(outs[-1][0])                                 # rounded before the head
  first = 0 if len(hist) > 1 else len(hist) - 1
  return _token_logprobs(sd, h[first:first + len(cand)], cand)


def oracle_all():
  """[dialogue][candidate] -> token log-probabilities of the fp32 oracle, computed once per process."""
  if "oracle" not in _MEMO:
    cfg, sd = R.gen_model()
    with torch.no_grad():
      _MEMO["oracle"] = [[oracle_candidate(sd, cfg, history_ids(i), c) for c in cands] for i, cands in enumerate(all_candidates())]
  return _MEMO["oracle"]


def close_pairs(means, mean_bar):
  """The pairs (a, b), a < b, of one dialogue's candidates whose oracle means are within 2 x the mean bar, closest first: two paths, each
  within one bar of the oracle, may order them either way."""
  n = len(means)
  gaps = [(abs(float(means[a]) - float(means[b])), a, b) for a in range(n) for b in range(a + 1, n)]
  return [(a, b) for g, a, b in sorted(gaps) if g <= 2 * mean_bar]


def left_out_pairs(means, mean_bar):
  """The pairs the ranking comparison leaves out: close_pairs, but never more than LEFT_OUT_CAP of the dialogue's pairs.  Where the cap binds,
  the closest pairs are left out and the others within 2 x the bar ARE compared: stricter than the two-paths argument grants (it then asks each
  path to stay within half that pair's gap of the oracle, less than one bar; tools/candidate_rank_tolerance.py prints and records the pair)."""
  n = len(means)
  return close_pairs(means, mean_bar)[:int(LEFT_OUT_CAP * (n * (n - 1) // 2))]


def check_order(tag, got, want, mean_bar):
  """Every pair that is not left out is ordered as the oracle orders it; at most LEFT_OUT_CAP of the pairs are left out."""
  n = len(want)
  out = set(left_out_pairs(want, mean_bar))
  pairs = n * (n - 1) // 2
  assert len(out) <= LEFT_OUT_CAP * pairs, f"{tag}: {len(out)} of {pairs} pairs are left out: the case shows too little"
  for a in range(n):
    for b in range(a + 1, n):
      if (a, b) not in out:
        assert (float(got[a]) > float(got[b])) == (float(want[a]) > float(want[b])), (tag, a, b, float(got[a]), float(got[b]), float(want[a]), float(want[b]))
  return len(out) / pairs


def load_tolerance():
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)) as f:
    return json.load(f)
