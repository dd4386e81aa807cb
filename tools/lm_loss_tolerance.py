#!/usr/bin/env python
"""The distances the bars of the LM-head loss tests rest on (CPU only; tests/lm_loss_util.py holds the bars).

  (a) operator level: on the operator tests' own inputs, fp32 accumulation in a permuted K order (lm_loss_util.fp32_permuted: an emulation
      of the kernel's arithmetic) against the fp64 restatement, for the logits, lse and tgt;
  (b) engine level: a bf16-operand emulation of the OPT pass (kv_cache_util.cached_forward_ref(rnd=bf), hidden rows rounded to bf16 before
      the head) against the fp32 oracle, for the batch loss and the token losses, on the engine test's inputs.

  python tools/lm_loss_tolerance.py            # print
  python tools/lm_loss_tolerance.py --write    # and write the tolerance section of profiles/lm_loss.md"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import kv_cache_util as K  # noqa: E402
import lm_loss_util as U  # noqa: E402

BEGIN, END = "<!-- tolerance:begin -->", "<!-- tolerance:end -->"
TILE = (128, 128, 512)      # row tile, column tile, columns per slab of csrc/lmloss.hip (the library says the same: test_lm_loss_host.py)


def geom_of(M, V, D):
  try:
    from gill_amd import ops
    return ops.lm_loss_geometry(M, V, D)
  except Exception:
    return (TILE[0], TILE[1], (V + TILE[2] - 1) // TILE[2], TILE[2])


def term_a():
  rows = []
  for (M, V, D) in U.operator_shapes(geom_of):
    geom = geom_of(M, V, D)
    x, w, t = U.build_inputs(M, V, D, U.OP_SEED, geom)
    ref = U.reference(x, w, t, geom)
    emu = U.fp32_permuted(x, w, t, geom, seed=1)
    d_logit = float((emu["logits"].double() - ref["logits"]).abs().max())
    d_lse = float((emu["lse"].double() - ref["lse"]).abs().max())
    d_tgt = float((emu["tgt"].double() - ref["tgt"]).abs().max())
    valid = t != -100
    r = ref["rank"][valid]
    hist = [int((r == 0).sum()), int(((r >= 1) & (r < 5)).sum()), int(((r >= 5) & (r <= 50)).sum()), int((r > 50).sum())]
    rows.append((M, V, D, d_logit, d_lse, d_tgt, float(ref["logits"].abs().max()), hist, len(U.ambiguous_rows(ref, t))))
    print(f"(a) M={M} V={V} D={D}: |logit| {d_logit:.2e} |lse| {d_lse:.2e} |tgt| {d_tgt:.2e}  max|L| {rows[-1][6]:.1f}  ranks 0/1-4/5-50/>50 {hist}  ambiguous {rows[-1][8]}",
          flush=True)
  return rows


def term_b():
  rows = []
  for B in (1, 3):
    cfg, sd, ids, full, last = U.engine_case(B)
    emb = torch.nn.functional.embedding(ids, sd["model.decoder.embed_tokens.weight"])
    ref = U.lm_scores(sd, cfg.num_layers, cfg.num_heads, emb, full)
    emu_hidden = lambda e: U.bf(K.cached_forward_ref(sd, cfg, e, (e.shape[1],), rnd=U.bf)[0][0])      # noqa: E731
    emu = U.lm_scores(sd, cfg.num_layers, cfg.num_heads, emb, full, hidden_fn=emu_hidden)
    d_loss = abs(float(emu["loss"]) - float(ref["loss"]))
    d_tok = float((emu["token_loss"] - ref["token_loss"]).abs().max())
    d_log = float((emu["logits"] - ref["logits"]).abs().max())
    rows.append((B, float(ref["loss"]), d_loss, d_tok, d_log))
    print(f"(b) B={B} T={ids.shape[1]}: oracle loss {rows[-1][1]:.4f}  |loss| {d_loss:.2e}  max |token_loss| {d_tok:.2e}  max |logit| {d_log:.2e}", flush=True)
  return rows


def render(a, b):
  out = [BEGIN, "## Tolerances (CPU; `python tools/lm_loss_tolerance.py --write`)", "",
         "### (a) operator: fp32 accumulation in a permuted K order against fp64, on the tests' own inputs", "",
         "| M | V | D | max abs logit distance | lse | tgt | max abs logit | true ranks 0 / 1-4 / 5-50 / >50 | ambiguous rows |", "|---|---|---|---|---|---|---|---|---|"]
  for (M, V, D, dl, ds, dt, mx, hist, amb) in a:
    out.append(f"| {M} | {V} | {D} | {dl:.2e} | {ds:.2e} | {dt:.2e} | {mx:.1f} | {hist[0]} / {hist[1]} / {hist[2]} / {hist[3]} | {amb} |")
  worst = max(r[3] for r in a)
  out += ["", f"Worst logit distance {worst:.2e}.  Bars (tests/lm_loss_util.py): logit / tgt {U.LOGIT_BAR:.1e} = {U.LOGIT_BAR / worst:.1f}x the worst distance, "
          f"lse {U.LSE_BAR:.1e}, mean {U.MEAN_BAR:.1e}.",
          "",
          "Why 8x and not 2x.  The emulation rounds to nearest at every add and takes the 32 products of a chunk in torch's order.  The matrix",
          "instruction's internal adder is not documented: an adder that truncates costs one ulp per add where the emulation has half (x2); the 32-term",
          "sum inside one instruction has an order of its own (x2); and the table's maximum is over one draw of 10^4 .. 2 x 10^6 logits (x2).  The",
          "fp32-output GEMMs of this library, on the same instruction, were recorded at 3e-7 .. 7e-7 of the largest output at K = 4096",
          "(`profiles/r06_gpu_tests_with_stats.log`): 8e-6 on logits of at most 11.5, inside the bar.  lse is",
          "1-Lipschitz in the logits under the sup norm, so it takes the logit bar; the 4e-6 on top is the fast exponential (`v_exp_f32` of",
          "`(v - m) log2 e`: rounding the argument at `|v - m| <= 16` is 1.4e-6 relative on a term, the instruction itself one ulp), the fp32 sums",
          "of at most 50 274 positive terms (relative 1e-6 on the sum, the same absolute on its log) and `logf`.  The mean's bar is the two bars of",
          "its terms plus 1e-5 for an fp32 mean of losses of about 10.",
          "",
          "### (b) engine: bf16-operand emulation of the 2-layer OPT pass against the fp32 oracle (V = 50274, T = 24, padded)", "",
          "| B | oracle loss | loss distance | max token-loss distance | max logit distance |", "|---|---|---|---|---|"]
  for (B, l, dl, dt, dg) in b:
    out.append(f"| {B} | {l:.4f} | {dl:.2e} | {dt:.2e} | {dg:.2e} |")
  wl, wt, wg = max(r[2] for r in b), max(r[3] for r in b), max(r[4] for r in b)
  out += ["", f"Bars: loss {U.LOSS_BAR:.1e} = {U.LOSS_BAR / wl:.1f}x the worst distance, token loss {U.TOKEN_LOSS_BAR:.1e} = {U.TOKEN_LOSS_BAR / wt:.1f}x, a logits row "
          f"(last_output_logit) {U.LAST_LOGIT_BAR:.1e} = {U.LAST_LOGIT_BAR / wg:.1f}x.  The emulation",
          "rounds every GEMM operand and the final hidden rows and is to stay within half a bar; the engine also accumulates in another order and",
          "forms its LayerNorm statistics from fused partial sums, hence a margin of 4 and not 2.", END]
  return "\n".join(out) + "\n"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  args = ap.parse_args()
  torch.manual_seed(0)
  a, b = term_a(), term_b()
  text = render(a, b)
  if args.write:
    path = os.path.join(ROOT, "profiles", "lm_loss.md")
    old = open(path).read() if os.path.exists(path) else "# LM-head loss kernel: tolerances and timings\n\n" + BEGIN + "\n" + END + "\n"
    i, j = old.index(BEGIN), old.index(END) + len(END)
    open(path, "w").write(old[:i] + text.rstrip("\n") + old[j:])
    print("wrote", path)
  else:
    print(text)


if __name__ == "__main__":
  main()
