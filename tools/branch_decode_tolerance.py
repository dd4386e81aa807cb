#!/usr/bin/env python3
"""The near-tie bar m of tests/test_branch_decode_gpu.py, measured on the CPU, on the recipe of tools/dialogue_session_tolerance.py: MARGIN (10) x
the largest distance between the decision keys of a bf16-operand emulation of the kernels' arithmetic (kv_cache_util.cached_forward_ref with
every GEMM operand rounded) and the fp32 oracle's, over the decisions of the oracle's own seeded run of the test (tests/branch_decode_util.py:
two histories of 33 and 70 tokens, four branches each, five decisions per branch).  It also chooses, per row and at one sampling seed, the prompt
seed: the first at which no decision of the oracle's run has a top-2 key margin under m, no branch picks an [IMG] token, and the greedy decisions after the replies the test adopts are clear of the session test's own bar (tests/golden/dialogue_session_tolerance.json).
  python tools/branch_decode_tolerance.py [--write]
Siblings draw different replies exactly where two decision keys are close, so a seed that is clear of the bar AND gives a row more than one reply
is rare: a row takes the first such seed among --tries, else the first clear one; the rows that draw more than one reply are recorded
(distinct_rows, at least one) and the GPU test asks for different replies on those.
--write stores m, the margin factor and the seeds in tests/golden/branch_decode_tolerance.json (the tests read them)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch   # noqa: E402
from gill_amd.synth import host_cores   # noqa: E402
import branch_decode_util as Bd   # noqa: E402
import dialogue_session_util as S   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--write", action="store_true")
ap.add_argument("--tries", type=int, default=24)
a = ap.parse_args()
torch.set_num_threads(host_cores())

m_session = S.load_tolerance()
SAMPLE_SEED = 7
seeds, distinct_rows = {}, []
for r, n in zip(Bd.ROWS, Bd.LENGTHS):
  first_clear = None
  for t in range(a.tries):
    run = Bd.oracle_row(r, n, 81 + t, SAMPLE_SEED)
    m_row = Bd.MARGIN * run["dist"]
    # a row's own distance is a lower bound of the run's: the bar over both rows is checked once both are chosen
    clear = run["margin"] >= 1.15 * m_row and not run["img"] and run["greedy_margin"] >= max(m_session, Bd.MARGIN * run["greedy_dist"])
    print(f"row {r} prompt seed {81 + t}: key distance bf16 emulation vs fp32 oracle {run['dist']:.3e} (x {Bd.MARGIN:g} = {m_row:.3e}); smallest "
          f"top-2 key margin of the oracle's {Bd.N * Bd.MAX_LEN} decisions {run['margin']:.3e}; [IMG] picked: {run['img']}; more than one reply: "
          f"{run['distinct']}; greedy decisions after the adopted reply: smallest margin {run['greedy_margin']:.3e}, distance "
          f"{run['greedy_dist']:.3e} (session bar {m_session:.3e}) -> {'clear' if clear else 'next'}", flush=True)
    if clear and first_clear is None:
      first_clear = 81 + t
    if clear and run["distinct"]:
      seeds[r] = 81 + t
      distinct_rows.append(r)
      break
  else:
    # siblings that draw different replies do so at decisions whose keys are close: a row may have no seed in reach that is both
    if first_clear is None:
      sys.exit(f"no prompt seed found for row {r}")
    print(f"row {r}: no seed of {a.tries} is clear of the bar AND draws more than one reply; taking the first clear one, {first_clear}")
    seeds[r] = first_clear
if not distinct_rows:
  sys.exit("no row draws more than one reply")
run = Bd.oracle_run(seeds, SAMPLE_SEED)
m = Bd.MARGIN * run["dist"]
print(f"both rows: largest key distance {run['dist']:.3e}, m = {Bd.MARGIN:g} x = {m:.3e}; smallest top-2 key margin {run['margin']:.3e}")
if run["margin"] < m:
  sys.exit("the rows' choices do not stand together")
for (r, j), (toks, margins) in sorted(run["branches"].items()):
  print(f"row {r} branch {j}: oracle tokens {toks}, key margins {[round(v, 3) for v in margins]}")
if a.write:
  path = os.path.join(ROOT, "tests", "golden", Bd.TOLERANCE_FILE)
  with open(path, "w") as f:
    json.dump({"m": m, "margin_factor": Bd.MARGIN, "largest_key_distance": run["dist"], "smallest_oracle_key_margin": run["margin"],
               "smallest_greedy_margin_after_adopt": run["greedy_margin"], "prompt_seeds": {str(r): s for r, s in sorted(seeds.items())},
               "distinct_rows": distinct_rows, "sample_seed": SAMPLE_SEED, "temperature": Bd.TEMPERATURE, "excused_share_cap": Bd.EXCUSED_SHARE}, f, indent=1)
    f.write("\n")
  print("wrote", path)
