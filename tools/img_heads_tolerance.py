#!/usr/bin/env python3
"""The bars of the image-block heads' operator test (tests/test_img_heads_gpu.py), measured on the CPU.
  python tools/img_heads_tolerance.py [--write]

An fp32 emulation of gill_op_img_block_heads with K in a permuted sequential order (tests/img_heads_util.heads_emulate) against fp64 on the
same bf16 operands, at the operator test's own shapes and seeds: the largest element distance of ret_emb and the largest probability
distance of probs.  The same pair for the rerank cosine (gill_op_img_rerank_scores).  The bars are 10 x those distances, the convention of
tools/w8_tolerance.py.  --write records them in tests/golden/img_heads_tolerance.json; tests/test_img_heads_host.py re-derives them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import img_heads_util as H     # noqa: E402


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  a = ap.parse_args()
  for ci, (D, E, C, n) in enumerate(H.OP_CASES):
    d_emb, d_p = H.heads_distances(D, E, C, n, H.case_seed(ci))
    margin = H.decision_margin(H.op_inputs(D, E, C, n, H.case_seed(ci)))
    print(f"heads D={D} E={E} C={C} n={n}: ret_emb {d_emb:.3e} probs {d_p:.3e}; smallest fp64 decision margin {margin:.3e}")
  for ci, (n, g, E) in enumerate(H.RERANK_CASES):
    print(f"rerank n={n} g={g} E={E}: {H.rerank_distance(n, g, E, H.case_seed(ci)):.3e}")
  d = H.measure()
  bars = {k: 10.0 * v for k, v in d.items()}
  print("largest distances", d)
  print("bars (10 x)", bars)
  if a.write:
    with open(H.TOLERANCE_FILE, "w") as f:
      json.dump({"bars": bars, "largest_distance": d}, f, indent=1)
      f.write("\n")
    print("wrote", H.TOLERANCE_FILE)
