#!/usr/bin/env python
"""Times the fused LM-head loss operator beside the unfused route built from what the package had before it (GPU).

  fused    ops.lm_head_loss: lse, target logit and rank per row, no (M, V) buffer;
  unfused  ops.gemm to an (M, V) fp32 logits tensor, then torch.logsumexp, a gather of the target column and topk(5) on the device.

The two arms alternate in one process and are timed with HIP events after warm-up; a figure is the median of the rounds.  Each row also gives
the bytes of W (V x D bf16) over the fused time: at small M the operator can do no better than stream W once.

  python tools/lm_loss_time.py            # print
  python tools/lm_loss_time.py --write    # and write the timing section of profiles/lm_loss.md"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(64, 50272, 4096), (320, 50272, 4096), (2048, 50272, 4096), (8192, 50272, 4096), (320, 50272, 768)]
BEGIN, END = "<!-- timing:begin -->", "<!-- timing:end -->"


def fused(x, w, t):
  from gill_amd import ops
  return ops.lm_head_loss(x, w, t, check=False)


def unfused(x, w, t):
  from gill_amd import ops
  logits = ops.gemm(x, w, out_f32=True)
  lse = torch.logsumexp(logits, dim=-1)
  tgt = logits.gather(1, t.clamp(min=0)[:, None])[:, 0]
  top5 = logits.topk(5, dim=-1).indices
  return lse, tgt, top5


def time_arm(fn, args, iters):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn(*args)
  b.record()
  b.synchronize()
  return a.elapsed_time(b) / iters


def measure(M, V, D, rounds, dev):
  g = torch.Generator().manual_seed(M + D)
  w = (torch.randn((V, D), generator=g) / D ** 0.5).to(dev, torch.bfloat16)
  x = torch.randn((M, D), generator=g).to(dev, torch.bfloat16)
  t = torch.randint(0, V, (M,), generator=g).to(dev)
  for fn in (fused, unfused):      # warm-up: code objects, workspaces, the allocator's blocks
    fn(x, w, t)
    fn(x, w, t)
  torch.cuda.synchronize()
  # a timed window of about 0.1 s per arm and round (a window of a few milliseconds measures the clock as much as the kernel)
  iters = max(5, min(400, int(100.0 / max(time_arm(unfused, (x, w, t), 3), 1e-3))))
  torch.cuda.reset_peak_memory_stats()
  fused(x, w, t)
  torch.cuda.synchronize()
  fused_extra = torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()
  tf, tu = [], []
  for _ in range(rounds):          # alternating arms
    tf.append(time_arm(fused, (x, w, t), iters))
    tu.append(time_arm(unfused, (x, w, t), iters))
  tf.sort(), tu.sort()
  # agreement of the two routes on what they both produce (the same operands; fp32 accumulation in two orders)
  lse_f, tgt_f, rank_f, _ = fused(x, w, t)
  lse_u, tgt_u, top5 = unfused(x, w, t)
  d_lse = float((lse_f - lse_u).abs().max())
  in5 = (top5 == t[:, None]).any(-1)
  flips = int((in5 != (rank_f < 5)).sum())
  del lse_u, tgt_u, top5
  torch.cuda.empty_cache()
  return dict(M=M, V=V, D=D, fused_ms=tf[len(tf) // 2], unfused_ms=tu[len(tu) // 2], fused_min=tf[0], fused_max=tf[-1], unfused_min=tu[0],
              unfused_max=tu[-1], w_gbs=V * D * 2 / (tf[len(tf) // 2] * 1e-3) / 1e9, tflops=2.0 * M * V * D / (tf[len(tf) // 2] * 1e-3) / 1e12,
              fused_peak_extra_mb=fused_extra / 2 ** 20, logits_mb=M * V * 4 / 2 ** 20, d_lse=d_lse, top5_flips=flips)


def render(rows, name):
  out = [BEGIN, f"## Timing (`python tools/lm_loss_time.py --write`, {name})", "",
         "Median of alternating rounds, HIP events, after warm-up; [min .. max] over the rounds.  `W / t`: bytes of the head over the fused time.",
         "`extra`: device memory the fused call allocates while it runs beyond its three (M) outputs' allocator blocks; `logits`: the (M, V) fp32",
         "tensor the unfused arm writes and reads three times.", "",
         "| M | V | D | fused ms | unfused ms | fused / unfused | fused TFLOP/s | W / t GB/s | extra MB | logits MB | max abs lse distance | top-5 verdicts differing |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in rows:
    out.append(f"| {r['M']} | {r['V']} | {r['D']} | {r['fused_ms']:.3f} [{r['fused_min']:.3f} .. {r['fused_max']:.3f}] | "
               f"{r['unfused_ms']:.3f} [{r['unfused_min']:.3f} .. {r['unfused_max']:.3f}] | {r['fused_ms'] / r['unfused_ms']:.2f} | {r['tflops']:.0f} | "
               f"{r['w_gbs']:.0f} | {r['fused_peak_extra_mb']:.1f} | {r['logits_mb']:.0f} | {r['d_lse']:.1e} | {r['top5_flips']} |")
  out.append(END)
  return "\n".join(out) + "\n"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--out", default=None, help="also write the table to this file")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("lm_loss_time.py measures on the GPU; none is visible")
  dev = torch.device("cuda:0")
  rows = []
  for (M, V, D) in SHAPES:
    rows.append(measure(M, V, D, args.rounds, dev))
    print(rows[-1], flush=True)
  p = torch.cuda.get_device_properties(0)
  text = render(rows, f"{p.name}, {getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs")
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
  if args.write:
    path = os.path.join(ROOT, "profiles", "lm_loss.md")
    old = open(path).read() if os.path.exists(path) else "# LM-head loss kernel: tolerances and timings\n"
    if BEGIN not in old:
      old = old.rstrip("\n") + "\n\n" + BEGIN + "\n" + END + "\n"
    i, j = old.index(BEGIN), old.index(END) + len(END)
    open(path, "w").write(old[:i] + text.rstrip("\n") + old[j:])
    print("wrote", path)


if __name__ == "__main__":
  main()
