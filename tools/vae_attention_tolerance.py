"""The bars of tests/test_vae_attention_gpu.py, measured on the CPU: how far bf16 STORAGE alone moves the VAE's single-head attention chain.

For every (shape, gain) of the GPU test (tests/vae_attention_util.py SHAPES x GAINS, the committed inputs) prints
distances(attn_storage, attn_exact) — worst-sample and worst-row relative L2 — for out without the residual, out with it and P; the test's bars
are twice these figures (the factor covers the MFMA accumulation and split-K order and __expf).  Also the whole-block case, and gain 16 — not run
on the GPU — with the bf16 SCORE storage alone.  Prints the STORAGE / BLOCK_STORAGE literals of the util module (figures rounded up to four
digits); `--write` records the table in profiles/vae_attention.md.

    python tools/vae_attention_tolerance.py [--write]
"""
import math
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vae_attention_util as A  # noqa: E402
from gill_amd import synth  # noqa: E402


def ceil4(x: float) -> float:
  """x rounded up to four significant digits"""
  e = math.floor(math.log10(x)) - 3
  return float(f"{math.ceil(x / 10.0 ** e) * 10.0 ** e:.3e}")


def measure(B, HW, C, gain, store=A.STORED):
  inp = A.attn_inputs(B, HW, C, gain, A.case_seed(B, HW, C, gain))
  exact = A.exact_of(inp)
  out, P = A.attn_chain(inp, False, store=store)
  outr, _ = A.attn_chain(inp, True, store=store)
  S = (inp["n"] @ inp["wq"].T + inp["bq"]) @ (inp["n"] @ inp["wk"].T + inp["bk"]).transpose(1, 2) / math.sqrt(C)
  info = (S.std().item(), exact["P"].amax(-1).median().item())
  return {"out": A.distances(out, exact["out"]), "out_resid": A.distances(outr, exact["out_resid"]), "P": A.distances(P, exact["P"])}, info


def block_groupnorm(x, gamma, beta, groups=32, eps=1e-6):
  B, HW, C = x.shape
  g = x.reshape(B, HW, groups, C // groups)
  mu = g.mean(dim=(1, 3), keepdim=True)
  var = g.var(dim=(1, 3), keepdim=True, unbiased=False)
  return ((g - mu) / (var + eps).sqrt()).reshape(B, HW, C) * gamma + beta


def measure_block():
  B, HW, C, gain = A.BLOCK_CASE
  x, gamma, beta, inp = A.block_inputs(B, HW, C, gain, A.case_seed(B, HW, C, gain))
  n = block_groupnorm(x, gamma, beta)
  ref = A.attn_chain({**inp, "n": n, "resid": x}, True)[0]
  low = A.attn_chain({**inp, "n": A.bf16_round(n), "resid": x}, True, store=A.STORED)[0]
  return A.distances(low, ref)


def row(tag, B, HW, C, gain, m, info):
  f = lambda t: f"{t[0]:.3e} | {t[1]:.3e}"   # noqa: E731
  return f"| {tag}({B}, {HW}, {C}) | {gain} | {info[0]:.2f} | {info[1]:.2f} | {f(m['out'])} | {f(m['out_resid'])} | {f(m['P'])} |"


if __name__ == "__main__":
  torch.set_num_threads(synth.host_cores())
  lines, lit = [], []
  for shape in A.SHAPES:
    for gain in A.GAINS:
      m, info = measure(*shape, gain)
      lines.append(row("", *shape, gain, m, info))
      lit.append(f"  {(*shape, gain)}: {{" + ", ".join(f'"{k}": ({ceil4(v[0]):.3e}, {ceil4(v[1]):.3e})' for k, v in m.items()) + "},")
  extra = []
  for shape in A.SHAPES[1:3]:
    m, info = measure(*shape, 16)
    extra.append(row("", *shape, 16, m, info))
    m, info = measure(*shape, 16, store=("S",))
    extra.append(row("S only: ", *shape, 16, m, info))
  bs, br = measure_block()
  head = ("| (B, HW, C) | gain | score std | median top p | out: sample | row | out + resid: sample | row | P: sample | row |\n"
          "|---|---|---|---|---|---|---|---|---|---|\n")
  table = head + "\n".join(lines)
  table16 = head + "\n".join(extra)
  print(table + "\n\n" + table16 + f"\n\nblock {A.BLOCK_CASE}: sample {bs:.3e}, row {br:.3e}\n")
  print("STORAGE = {\n" + "\n".join(lit) + "\n}")
  print(f"BLOCK_STORAGE = ({ceil4(bs):.3e}, {ceil4(br):.3e})")
  if "--write" in sys.argv:
    path = os.path.join(ROOT, "profiles", "vae_attention.md")
    text = open(path).read() if os.path.exists(path) else "# VAE attention\n"
    block = ("<!-- tolerance -->\n## bf16 storage distance (tools/vae_attention_tolerance.py, CPU)\n\n"
             "distances(attn_storage, attn_exact) of tests/vae_attention_util.py: the fp64 chain with q, k, v, S, P, O and out rounded to bf16 where the\n"
             "engine stores them, against the fp64 chain with no rounding; worst-sample and worst-row relative L2.  The GPU bars are twice these.\n\n"
             + table + "\n\n"
             f"Whole block (GroupNorm + chain + residual, {A.BLOCK_CASE}): sample {bs:.3e}, row {br:.3e}.\n\n"
             "Gain 16 (|score| up to ~80; not run on the GPU), all storage and the bf16 SCORE storage alone:\n\n" + table16 + "\n<!-- /tolerance -->\n")
    if "<!-- tolerance -->" in text:
      text = re.sub(r"<!-- tolerance -->.*?<!-- /tolerance -->\n", lambda _: block, text, flags=re.S)
    else:
      text = text.rstrip("\n") + "\n\n" + block
    open(path, "w").write(text)
