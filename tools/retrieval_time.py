"""HIP-event time of GillRetrievalIndex.search on a CC3M-sized index (2.7 M x 256, seeded normal rows, unit rows x exp(logit_scale)) beside the
path it replaces — GILL._scores (padded copy + GEMM with the query in 4 output columns) + the seen penalty + topk, once per query, on the same
matrix in the same process, alternating.  Q = 1, 8, 16, 32 and k = 3, 10; three seen rows per query on both sides; warm-up, then at least
0.5 s of timed work per point and side.

`--write` records the table in profiles/retrieval.md (a "Where the time of one search goes" section behind it is kept): ms per search, GB/s of matrix bytes (one pass per 16 queries) and the share of the
6.3 TB/s achievable HBM rate.  The one condition: search is not slower than the legacy path at any point (the tool exits non-zero otherwise).

    python tools/retrieval_time.py [--write] [--rows 2700000] [--min-seconds 0.5]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gill_amd  # noqa: E402
from gill_amd.models import GILL  # noqa: E402
from gill_amd.retrieval import GillRetrievalIndex  # noqa: E402

DIM = 256
HBM_GBS = 6300.0        # achievable HBM rate of the MI355X (float4 copy), GB/s
POINTS = [(q, k) for q in (1, 8, 16, 32) for k in (3, 10)]
TRACE_HEADING = "## Where the time of one search goes"


def _events(fn, n):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(n):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / 1000.0


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--rows", type=int, default=2_700_000)
  ap.add_argument("--min-seconds", type=float, default=0.5)
  args = ap.parse_args()
  gill_amd.configure_hip_runtime()
  dev = torch.device("cuda:0")
  n, scale = args.rows, math.exp(2.6592)       # CLIP's logit scale at initialisation, exp(log(1 / 0.07))
  g = torch.Generator(device=dev).manual_seed(1234)

  index = GillRetrievalIndex(DIM, n, dev)
  for lo in range(0, n, 1 << 18):               # seeded rows in pieces: the fp32 draw never exists whole
    index.add(torch.randn((min(1 << 18, n - lo), DIM), device=dev, generator=g), normalize=True, scale=scale)
  matrix = torch.cat([index.rows(lo, min(1 << 18, n - lo)) for lo in range(0, n, 1 << 18)], 0)     # what load_gill leaves in emb_matrix (bf16)
  torch.cuda.synchronize()
  nbytes = n * DIM * 2
  print(f"index: {n} x {DIM} bf16 = {nbytes / 1e9:.3f} GB; first row of the main pass, lists, rows per list = {index.slabs()}")

  queries = torch.randn((32, DIM), device=dev, generator=g)
  seen = torch.randint(0, n, (32, 3), device=dev, generator=g)
  seen_host = seen.cpu().tolist()

  def legacy(Q, k):
    out = None
    for q in range(Q):
      ret_emb = queries[q:q + 1] / queries[q:q + 1].norm(dim=-1, keepdim=True)
      scores = GILL._scores(matrix, ret_emb.to(matrix.dtype))
      for s in seen_host[q]:
        scores[s, :] -= 1000
      out = scores.squeeze().topk(k)
    return out

  # the two paths rank the same rows (bf16 ties aside: the legacy path rounds the scores to bf16 before topk)
  ls, li = legacy(1, 10)
  ns, ni = index.search(queries[:1], 10, normalize=True, exclude=seen[:1], penalty=1000.0)
  agree = len(set(li.tolist()) & set(ni[0].tolist()))
  print(f"top-10 of query 0: legacy {li.tolist()} / search {ni[0].tolist()} ({agree} shared; legacy scores are bf16-rounded)")

  rows, slower = [], []
  for Q, k in POINTS:
    new = lambda: index.search(queries[:Q], k, normalize=True, exclude=seen[:Q], penalty=1000.0)  # noqa: E731
    old = lambda: legacy(Q, k)  # noqa: E731
    for fn in (new, old, new, old):
      fn()
    torch.cuda.synchronize()
    t_new1, t_old1 = _events(new, 3) / 3, _events(old, 1)
    reps_new, reps_old = max(3, int(0.1 / t_new1) + 1), max(1, int(0.1 / t_old1) + 1)
    tn = to = 0.0
    cn = co = 0
    best_new, best_old = float("inf"), float("inf")
    while tn < args.min_seconds or to < args.min_seconds:      # alternating batches of about 0.1 s
      t = _events(new, reps_new)
      tn, cn, best_new = tn + t, cn + reps_new, min(best_new, t / reps_new)
      t = _events(old, reps_old)
      to, co, best_old = to + t, co + reps_old, min(best_old, t / reps_old)
    ms_new, ms_old = tn / cn * 1e3, to / co * 1e3
    passes = (Q + 15) // 16
    gbs = passes * nbytes / (ms_new * 1e-3) / 1e9
    rows.append(f"| {Q} | {k} | {ms_new:.3f} | {best_new * 1e3:.3f} | {passes} | {gbs:.0f} | {gbs / HBM_GBS * 100:.1f} % | {ms_old:.2f} | {best_old * 1e3:.2f} | "
                f"{ms_old / ms_new:.1f} x |")
    print(rows[-1])
    if ms_new > ms_old:
      slower.append((Q, k, ms_new, ms_old))

  if args.write:
    path = os.path.join(ROOT, "profiles", "retrieval.md")
    keep = open(path).read() if os.path.exists(path) else ""      # the kernel-trace section behind the table is written by hand: keep it
    keep = keep[keep.index(TRACE_HEADING):] if TRACE_HEADING in keep else ""
    open(path, "w").write(
      "# Retrieval: measured times (tools/retrieval_time.py)\n\n"
      f"One MI355X.  Index: {n} x {DIM} seeded normal rows, normalised on the device to exp(logit_scale) x unit rows, bf16 = {nbytes / 1e9:.3f} GB "
      "(beyond the 256 MiB Infinity Cache: every pass streams from HBM); first row of the main pass, its lists, rows per list = " f"{index.slabs()}.  HIP events around batches of "
      f"about 0.1 s, the two paths alternating in one process, at least {args.min_seconds} s of timed work per point and side; mean over all batches "
      "and the best batch.  Three seen rows per query on both sides.\n\n"
      "`search`: GillRetrievalIndex.search(normalize=True) — query normalise + prefix pass + merge + main pass + merge, five launches per 16 queries; one "
      "pass over the matrix per 16 queries.  GB/s = passes x matrix bytes / time; share of the 6.3 TB/s achievable HBM rate "
      "(MI355X: float4 copy).  `legacy`: what the parent commit runs per [IMG0] — GILL._scores (a fresh padded bf16 copy of the matrix + the "
      "general GEMM with the query in 4 output columns + the (N, 1) score vector rounded to bf16) + `scores[seen] -= 1000` + `topk(k)` — "
      "called once per query, as generate_for_images_and_texts does.\n\n"
      "| Q | k | search ms | best | passes | GB/s | of 6.3 TB/s | legacy ms | best | legacy / search |\n|---|---|---|---|---|---|---|---|---|---|\n" +
      "\n".join(rows) + "\n\n" +
      ("search is faster than the legacy path at every point.\n" if not slower else
       "search is SLOWER than the legacy path at: " + ", ".join(f"Q={q} k={k} ({a:.3f} vs {b:.3f} ms)" for q, k, a, b in slower) + "\n") +
      ("\n" + keep if keep else ""))
  if slower:
    sys.exit(f"search slower than the legacy path at {slower}")


if __name__ == "__main__":
  main()
