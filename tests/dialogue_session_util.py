"""Shared by test_dialogue_session_host.py, test_dialogue_session_gpu.py and tools/dialogue_session_tolerance.py (not a test module): the
multi-turn sessions those tests run, as plans, and the fp32 oracle's own run of them.

The rig is that of test_generate_batch_gpu.py (ragged_decode_util.gen_model: OPT-125m geometry, synth.opt_state_dict seed 5), greedy,
min_word_tokens = 3 and gen_scale_factor = 1e5 with max_len = 5: per turn three free decisions, then [IMG0] is certain at decisions 3 and 4 (two
forced blocks; the second ends the row), 19 tokens in all, and n_hidden = 11 covers the first block.

A plan is a list of operations on the B = 4 rows of a session:
  ("turn", {row: number of new ids})   the named rows extend by that many ids (new_ids) and generate; the other rows are idle
  ("rollback", row, keep)              keep only the first `keep` generated tokens of the row's last turn
  ("reset", row)                       empty the row: its next turn starts a new dialogue
The "concatenated prompts" of a plan are what each decoding row's history holds when it decodes; with greedy decoding they depend on the tokens
earlier turns emitted, so oracle_session replays the plan with the ORACLE's own greedy tokens (ragged_decode_util.oracle_greedy) and returns, per
(turn, row), the history it decoded from, its three free tokens, their top-2 margins and the bf16-emulation's logit distance.  The seed of every
(turn, row)'s new ids is chosen (tools/dialogue_session_tolerance.py, recorded beside m in the golden file) so that no margin is under
m = 10 x the largest distance: the reference alone never needs an excusal, and a session that agrees with it walks through the same histories."""
import json
import os

import ragged_decode_util as R
from gill_amd import synth

B = 4
CAPACITY = 128
MAX_LEN = 5
GEN_KW = dict(min_word_tokens=R.GEN_MWT, gen_scale_factor=1e5)
N_TOK, N_HID = 19, 11                  # per decoding row and turn
SEED = 61
TOLERANCE_FILE = "dialogue_session_tolerance.json"       # under tests/golden

PLANS = {
  # every row in both turns
  "two": [("turn", {0: 9, 1: 6, 2: 12, 3: 5}), ("turn", {0: 7, 1: 4, 2: 5, 3: 10})],
  # row 1 idle in turn 2, row 2 rolled back to two of its tokens after turn 1, row 3 reset after turn 2 and restarted in turn 3
  "three": [("turn", {0: 9, 1: 6, 2: 12, 3: 5}), ("rollback", 2, 2), ("turn", {0: 7, 2: 5, 3: 10}), ("reset", 3),
            ("turn", {0: 6, 1: 8, 2: 4, 3: 9})],
}


def _golden():
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)
  if not os.path.exists(path):
    return {}
  with open(path) as f:
    return json.load(f)


def load_seeds():
  """{plan: {(turn, row): seed of that row's new ids}} as tools/dialogue_session_tolerance.py chose them; a missing entry is SEED."""
  return {name: {tuple(int(v) for v in k.split(",")): int(s) for k, s in tab.items()} for name, tab in _golden().get("seeds", {}).items()}


def new_ids(turn, row, n, first, seed=SEED):
  """The n ids row `row` brings in turn `turn` (0-based count of "turn" operations): <bos> in front only where a dialogue starts."""
  ids = synth.synthetic_prompt_ids(B, n, seed=seed + 100 * turn)[row, :n].tolist()
  if not first:
    ids[0] = 3 + (ids[1] if n > 1 else 7) % 1000        # synthetic_prompt_ids puts <bos> first: a later turn starts with a word
  return ids


def walk(plan, seeds, decode, ids_of=None):
  """Replays a plan on host lists.  decode(turn, row, history) -> the tokens that row emits in that turn; seeds: {(turn, row): seed} of the
  rows' new ids, or ids_of(turn, row, n, history so far) -> the n new ids (the tool that chooses the seeds).  -> the final histories."""
  ids_of = ids_of or (lambda turn, row, n, h: new_ids(turn, row, n, first=not h, seed=seeds.get((turn, row), SEED)))
  hist, start, turn = [[] for _ in range(B)], [0] * B, 0
  for op in plan:
    if op[0] == "rollback":
      del hist[op[1]][start[op[1]] + op[2]:]
    elif op[0] == "reset":
      hist[op[1]], start[op[1]] = [], 0
    else:
      for row, n in sorted(op[1].items()):
        hist[row] += ids_of(turn, row, n, list(hist[row]))
        start[row] = len(hist[row])
        hist[row] += decode(turn, row, list(hist[row]))
      turn += 1
  return hist


def oracle_session(name, seeds=None, memo=None):
  """The oracle's own greedy run of PLANS[name] -> [(turn, row, history decoded from, free tokens, margins, distance)] in plan order."""
  cfg, sd = R.gen_model()
  memo = {} if memo is None else memo
  seeds = load_seeds().get(name, {}) if seeds is None else seeds
  out = []

  def decode(turn, row, hist):
    key = tuple(hist)
    if key not in memo:
      memo[key] = R.oracle_greedy(sd, cfg, hist)
    toks, margins, _, dist = memo[key]
    out.append((turn, row, hist, toks, margins, dist))
    return toks + synth.IMG_TOKEN_IDS * 2

  walk(PLANS[name], seeds, decode)
  return out


def load_tolerance():
  return float(_golden()["m"])
