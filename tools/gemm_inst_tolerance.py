"""Measures the transcendental-approximation term of the GEMM epilogue's SiLU and GELU (gemm_dev.h: silu_f, gelu_erf) for the bar of
tests/gemm_inst_util.py, and writes tests/golden/gemm_inst_tolerance.json.

For every SiLU / GELU case of the table, run the same call on the fp32-output path and compare with act(pre) in fp64 on the CPU (never with
another run of the kernels).  What the linear part of the bar does not explain, per unit of |pre|,

    measured = max over elements of (|got - act(pre)| - L (2^-24 |pre| + (K + 4) 2^-24 S)) / |pre|        (0 where negative)

is the activation's own error: the erf approximation of gelu_erf (Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7) and the v_exp_f32 / v_rcp_f32
pair of silu_f.  The cases sample only part of the argument range, so the bar uses term = max(4 x measured, 4 x 2^-24) — the floor is the
activation's four fp32 roundings.  Needs the GPU.

  python tools/gemm_inst_tolerance.py [--out tests/golden/gemm_inst_tolerance.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
  import torch
  import gemm_inst_util as G
  from gill_amd import ops
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=G.TOLERANCE_JSON)
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  res = {a: {"measured": 0.0, "worst_ratio_of_linear_bar": 0.0, "cases": []} for a in ("silu", "gelu")}
  for c in G.CASES:
    act = c.kw.get("act", "none")
    if c.op != "gemm" or act not in res or "gn" in c.kw:
      continue
    kw = dict(c.kw, out_f32=True)
    a, w, bias, resid, alpha = G.gemm_operands(kw, False)
    pre, S = G.gemm_ref(a, w, bias, resid, alpha)
    b16 = torch.bfloat16
    got = ops.gemm(a.to(b16).to(dev), w.to(b16).to(dev), None if bias is None else bias.to(dev), None if resid is None else resid.to(b16).to(dev),
                   alpha=alpha, act=act, out_f32=True, splitk=kw.get("splitk", 0)).cpu().double()
    err = (got - G.ACT_FP64[act](pre)).abs()
    linear = G.LIPSCHITZ[act] * G.bar(pre, S, kw["K"], True)
    excess = ((err - linear) / pre.abs().clamp_min(1e-30)).clamp_min(0)
    m, r = float(excess.max()), float((err / linear).max())
    print(f"{c.id}: {act} {kw['M']}x{kw['N']}x{kw['K']} |pre| up to {float(pre.abs().max()):.2f}: measured {m:.3e}, |err| / linear bar up to {r:.3f}")
    res[act]["measured"] = max(res[act]["measured"], m)
    res[act]["worst_ratio_of_linear_bar"] = max(res[act]["worst_ratio_of_linear_bar"], r)
    res[act]["cases"].append(c.id)
  for a in res:
    res[a]["term"] = G.act_term_from_measured(res[a]["measured"])
  res["margin"], res["floor"] = G.ACT_TERM_MARGIN, G.ACT_TERM_FLOOR
  res["unit"] = "term x |pre-activation|, added to lipschitz x (u |pre| + (K + 4) 2^-24 S)"
  with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
  print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
  main()
