"""The measured terms of tests/test_ends_gpu.py's bars, computed on the CPU from the committed inputs of tests/ends_util.py.

  REDUCE_A[(D, kind)]    4 x the largest distance of a plain fp32 two-pass LayerNorm from the fp64 one over every (sk, M, eps) of the reducer test,
                         on the rows the fp32 ordered sum gives (the rows the kernel must reproduce bit for bit)
  LINEAR_A[(M,N,K,sk)]   the same on the rows of the fused-against-unfused linear cases
  TIMESTEP_E[dim]        2 x the largest distance of oracle.unet_ref.timestep_embedding (fp32) from the fp64 restatement over the test's timesteps

Prints the literals of the util module (figures rounded up to four digits); `--write` records the table in profiles/ends.md.

    python tools/ends_tolerance.py [--write]
"""
import math
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ends_util as U  # noqa: E402
from gill_amd import synth  # noqa: E402
from oracle import unet_ref  # noqa: E402


def ceil4(x: float) -> float:
  """x rounded up to four significant digits"""
  if x == 0.0:
    return 0.0
  e = math.floor(math.log10(x)) - 3
  return float(f"{math.ceil(x / 10.0 ** e) * 10.0 ** e:.3e}")


def reduce_a(D, kind):
  worst = 0.0
  for sk in U.REDUCE_SK:
    for M in U.REDUCE_M:
      ws, bias, resid, gamma, beta = U.reduce_case(D, sk, M, kind)
      h = U.reduce_sum_f32(ws, sk, bias, resid)
      for eps in U.REDUCE_EPS:
        worst = max(worst, U.layernorm_f32_distance(h, gamma, beta, eps))
  return 4.0 * worst


def linear_a(M, N, K, sk):
  a, w, bias, h, gamma, beta = U.linear_case(M, N, K, sk)
  return 4.0 * U.layernorm_f32_distance(U.linear_ref(a, w, bias, h)[0].float(), gamma, beta, 1e-5)


def timestep_e(dim):
  worst = 0.0
  for t in U.timestep_sets():
    worst = max(worst, (unet_ref.timestep_embedding(t, dim).double() - U.timestep_ref(t, dim)).abs().max().item())
  return 2.0 * worst


if __name__ == "__main__":
  torch.set_num_threads(synth.host_cores())
  A = {(D, k): ceil4(reduce_a(D, k)) for D in U.REDUCE_D for k in U.REDUCE_KINDS}
  L = {c: ceil4(linear_a(*c)) for c in U.LINEAR_CASES}
  E = {d: ceil4(timestep_e(d)) for d in U.TIMESTEP_DIMS}
  print("REDUCE_A = {")
  for D in U.REDUCE_D:
    print("  " + " ".join(f'({D}, "{k}"): {A[(D, k)]:.3e},' for k in U.REDUCE_KINDS))
  print("}")
  print("LINEAR_A = {" + ", ".join(f"{c}: {v:.3e}" for c, v in L.items()) + "}")
  print("TIMESTEP_E = {" + ", ".join(f"{d}: {v:.3e}" for d, v in E.items()) + "}")
  table = ("| D | " + " | ".join(U.REDUCE_KINDS) + " |\n|---|" + "---|" * len(U.REDUCE_KINDS) + "\n"
           + "\n".join(f"| {D} | " + " | ".join(f"{A[(D, k)]:.3e}" for k in U.REDUCE_KINDS) + " |" for D in U.REDUCE_D))
  block = ("<!-- tolerance -->\n## Measured terms of the bars (tools/ends_tolerance.py, CPU)\n\n"
           "A of the reduce + LayerNorm bar (one bf16 ulp of the fp64 LayerNorm + A): four times the largest distance of a plain fp32 two-pass LayerNorm\n"
           "from the fp64 one over every (sk, M, eps) of the test, per (D, row kind).  Constant rows: the fp32 emulation is exact.\n\n" + table + "\n\n"
           "The fused-against-unfused linear cases (M, N, K, splitk), eps 1e-5: " + ", ".join(f"{c}: {v:.3e}" for c, v in L.items()) + ".\n\n"
           "E of the timestep-embedding bar (2^-8 |exact| + E): twice the largest distance of the oracle's fp32 `timestep_embedding` from the fp64 one over the\n"
           "test's timesteps and every channel; its rough bound is |angle| 2^-22 = 2.4e-4.  " + ", ".join(f"dim {d}: {v:.3e}" for d, v in E.items())
           + ".\n<!-- /tolerance -->\n")
  if "--write" in sys.argv:
    path = os.path.join(ROOT, "profiles", "ends.md")
    text = open(path).read() if os.path.exists(path) else "# Operator tests of the end kernels\n"
    if "<!-- tolerance -->" in text:
      text = re.sub(r"<!-- tolerance -->.*?<!-- /tolerance -->\n", lambda _: block, text, flags=re.S)
    else:
      text = text.rstrip("\n") + "\n\n" + block
    open(path, "w").write(text)
