#!/usr/bin/env python
"""The distances the bars of the candidate-ranking tests rest on (CPU only; tests/candidate_rank_util.py holds the inputs).

Follows tools/lm_loss_tolerance.py term (b): a bf16-operand emulation of the scoring pass, [history cached | last history token + candidate]
through kv_cache_util.cached_forward_ref(rnd=bf) with the hidden rows rounded before the head, against the fp32 oracle on every history +
candidate of the tests' own inputs, for a token's log-probability and for a candidate's mean.  Token bar and mean bar are 4 x the largest
distances (that file's margin and reasoning: the emulation is to stay within half a bar, the engine also accumulates in another order and
forms its LayerNorm statistics from fused partial sums).  Also recorded: the oracle's candidate means, and per dialogue the share of candidate
pairs whose oracle means lie within 2 x the mean bar, which the ranking test leaves out; the tool fails if that share exceeds the cap.

  python tools/candidate_rank_tolerance.py            # print
  python tools/candidate_rank_tolerance.py --write    # and write tests/golden/candidate_rank_tolerance.json and the tolerance section of
                                                      # profiles/candidate_ranking.md"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import candidate_rank_util as U  # noqa: E402
import ragged_decode_util as R  # noqa: E402

BEGIN, END = "<!-- tolerance:begin -->", "<!-- tolerance:end -->"


def measure():
  cfg, sd = R.gen_model()
  oracle = U.oracle_all()
  rows, d_tok, d_mean = [], 0.0, 0.0
  with torch.no_grad():
    for i, cands in enumerate(U.all_candidates()):
      hist = U.history_ids(i)
      t_i = m_i = 0.0
      for j, c in enumerate(cands):
        emu = U.emulated_candidate(sd, cfg, hist, c)
        t_i = max(t_i, float((emu - oracle[i][j]).abs().max()))
        m_i = max(m_i, abs(float(emu.mean()) - float(oracle[i][j].mean())))
      lo = min(float(-o.max()) for o in oracle[i])
      hi = max(float(-o.min()) for o in oracle[i])
      rows.append((i, len(hist), t_i, m_i, lo, hi))
      d_tok, d_mean = max(d_tok, t_i), max(d_mean, m_i)
      print(f"dialogue {i} (history {len(hist)}): max token distance {t_i:.3e}, max mean distance {m_i:.3e}, oracle token losses {lo:.1f} .. {hi:.1f}",
            flush=True)
  token_bar, mean_bar = U.MARGIN * d_tok, U.MARGIN * d_mean
  means = [[float(o.mean()) for o in row] for row in oracle]
  shares, close, bound = [], [], []
  for i, mrow in enumerate(means):
    n = len(mrow)
    pairs = n * (n - 1) // 2
    near, out = U.close_pairs(mrow, mean_bar), U.left_out_pairs(mrow, mean_bar)
    shares.append(len(out) / pairs)
    close.append(len(near) / pairs)
    print(f"dialogue {i}: {close[-1]:.1%} of the candidate pairs lie within 2 x the mean bar, {shares[-1]:.1%} are left out", flush=True)
    for (a, b) in near[len(out):]:      # the cap binds: compared although within 2 x the bar
      bound.append([i, a, b, abs(mrow[a] - mrow[b])])
      print(f"  the cap of {U.LEFT_OUT_CAP:.0%} binds: candidates {a} and {b} (oracle gap {bound[-1][3]:.3f} <= {2 * mean_bar:.3f}) are compared all the same",
            flush=True)
  assert max(shares) <= U.LEFT_OUT_CAP, f"the ranking test would leave out {max(shares):.1%} of a dialogue's pairs (cap {U.LEFT_OUT_CAP:.0%})"
  gold = dict(token_distance=d_tok, mean_distance=d_mean, margin=U.MARGIN, token_bar=token_bar, mean_bar=mean_bar, left_out_share=shares, within_two_bars_share=close, compared_within_two_bars=bound,
              left_out_cap=U.LEFT_OUT_CAP, oracle_means=means, histories=list(U.HISTORIES), counts=list(U.COUNTS))
  return gold, rows


def render(gold, rows):
  out = [BEGIN, "## Tolerances (CPU; `python tools/candidate_rank_tolerance.py --write`)", "",
         "bf16-operand emulation of the scoring pass ([history cached | last history token + candidate], hidden rows rounded before the head)",
         "against the fp32 oracle on every history + candidate alone; OPT-125m geometry, synthetic weights, V = 50274; ten candidates of",
         f"{', '.join(str(c) for c in U.COUNTS)} tokens per dialogue.", "",
         "| dialogue | history | max token log-prob distance | max candidate-mean distance | oracle token losses |", "|---|---|---|---|---|"]
  for (i, n, t, m, lo, hi) in rows:
    out.append(f"| {i} | {n} | {t:.3e} | {m:.3e} | {lo:.1f} .. {hi:.1f} |")
  out += ["", f"Bars: token {gold['token_bar']:.3e}, candidate mean {gold['mean_bar']:.3e} = {U.MARGIN:.0f} x the worst distances "
          f"({gold['token_distance']:.3e}, {gold['mean_distance']:.3e}); margin and reasoning of `tools/lm_loss_tolerance.py` term (b).  Token losses on",
          "this rig are far above those of the 2-layer rig of the LM-head loss tests, so those bars do not carry over.", "",
          "Share of a dialogue's 45 candidate pairs whose oracle means lie within 2 x the mean bar (left out of the ranking comparison, cap "
          f"{U.LEFT_OUT_CAP:.0%}): " + ", ".join(f"{s:.1%}" for s in gold["within_two_bars_share"]) + "; left out: "
          + ", ".join(f"{s:.1%}" for s in gold["left_out_share"]) + ".  Where the cap binds the closest pairs are left out and the rest are compared all the",
          "same (stricter than the two-paths argument grants): "
          + (", ".join(f"dialogue {i} candidates {a} / {b} (gap {g:.3f})" for i, a, b, g in gold["compared_within_two_bars"]) or "nowhere") + ".", END]
  return "\n".join(out) + "\n"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  args = ap.parse_args()
  torch.manual_seed(0)
  torch.set_num_threads(1)      # one thread: the fp32 sums, and with them the emulation's bf16 roundings, come out the same on every run
  gold, rows = measure()
  text = render(gold, rows)
  if args.write:
    with open(os.path.join(ROOT, "tests", "golden", U.TOLERANCE_FILE), "w") as f:
      json.dump(gold, f, indent=1)
      f.write("\n")
    path = os.path.join(ROOT, "profiles", "candidate_ranking.md")
    old = open(path).read() if os.path.exists(path) else "# Candidate ranking: tolerances and timings\n\n" + BEGIN + "\n" + END + "\n"
    i, j = old.index(BEGIN), old.index(END) + len(END)
    open(path, "w").write(old[:i] + text.rstrip("\n") + old[j:])
    print("wrote", path)
  else:
    print(text)


if __name__ == "__main__":
  main()
