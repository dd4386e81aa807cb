#!/usr/bin/env python3
"""Timing of the weight-only fp8 decoder (w8) on the MI355X, OPT-6.7b shapes, synthetic weights drawn on the device.
  python tools/w8_decode_time.py [--write] [--profile PATH] [--layers 32]

1. Milliseconds per ragged decode iteration (gill_opt_decode_step after a 16-token prefill) at B = 1, 4, 16 on a w8 handle and on a mode-0
   handle of the same weights, alternating, device events around blocks of steps.  gill_opt_decode_step on a mode-0 handle is the code
   path of the commit before the w8 mode, launch for launch.
2. Each of the four linears of a layer alone at M = 1 and 16: ops.linear_w8 (bias epilogue; the narrow matrices with the launcher's own
   K split and its finishing pass) beside ops.gemm (the STREAM64 tile on the blocked copy of the dequantised matrix), per launch from the
   difference of two GILL_OP_REPEAT counts, as microseconds and as TB/s of weight bytes (N K for fp8, 2 N K for bf16).  Repeats of one
   launch re-read a 50 - 134 MB matrix back to back: part of it can come from the 256 MB memory-side cache, so these rates are an upper
   view of the kernel; the decode iteration (6.4 GB of fp8 weights per step) is the figure that counts.
--write replaces the "timing" section of profiles/w8_decode.md (or of --profile)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gill_amd import _native as N, ops, synth   # noqa: E402


def device_opt_state_dict(cfg, dev, seed):
  """OPTForCausalLM names, bf16 values drawn on the device (fan-in scaled like gill_amd.synth)."""
  g = torch.Generator(device=dev).manual_seed(seed)
  D, F = cfg.hidden_size, cfg.ffn_dim
  rn = lambda shape, std: (torch.randn(shape, device=dev, generator=g) * std).to(torch.bfloat16)   # noqa: E731
  sd = {"model.decoder.embed_tokens.weight": rn((cfg.vocab_size, D), 0.5),
        "model.decoder.embed_positions.weight": rn((cfg.max_positions + 2, D), 0.25)}

  def norm(p):
    sd[p + ".weight"] = (1.0 + 0.1 * torch.randn(D, device=dev, generator=g)).to(torch.bfloat16)
    sd[p + ".bias"] = rn((D,), 0.02)

  def linear(p, out, inp):
    sd[p + ".weight"] = rn((out, inp), inp ** -0.5)
    sd[p + ".bias"] = rn((out,), 0.02)
  norm("model.decoder.final_layer_norm")
  for i in range(cfg.num_layers):
    p = f"model.decoder.layers.{i}"
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
      linear(f"{p}.self_attn.{n}", D, D)
    norm(f"{p}.self_attn_layer_norm")
    linear(f"{p}.fc1", F, D)
    linear(f"{p}.fc2", D, F)
    norm(f"{p}.final_layer_norm")
  return sd


def create(sd, cfg, dev, mode, max_batch, max_seq):
  c = N.gill_opt_config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                        ffn_dim=cfg.ffn_dim, max_positions=cfg.max_positions, max_batch=max_batch, max_seq=max_seq)
  arr, keep = N.make_tensor_table(sd, dev)
  h = C.c_void_p()
  N.check(N.lib().gill_opt_create_ex(C.byref(h), C.byref(c), arr, len(keep), mode))
  return h


def decode_iterations(cfg, dev, lines, steps=20, rounds=7):
  sd = device_opt_state_dict(cfg, dev, 0)
  T0 = 16
  handles = {"bf16": create(sd, cfg, dev, 0, 16, 64), "w8": create(sd, cfg, dev, 1, 16, 64)}
  ids = synth.synthetic_prompt_ids(16, T0, seed=3, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:, :T0].to(dev)
  x = sd["model.decoder.embed_tokens.weight"][ids[:, -1]].contiguous()
  lib, stream = N.lib(), N.current_stream()
  lines += ["## Ragged decode iteration, OPT-6.7b shapes (MI355X)", "",
            f"`python tools/w8_decode_time.py --write`: {cfg.num_layers} layers, D = {cfg.hidden_size}, F = {cfg.ffn_dim}; gill_opt_decode_step after a {T0}-token",
            f"prefill, median of {rounds} alternating blocks of {steps} steps, device events.  bf16 = a mode-0 handle (the code path before this mode).", "",
            "| B | bf16 ms / iteration | w8 ms / iteration | w8 / bf16 |", "|---|---|---|---|"]
  for B in (1, 4, 16):
    lens = torch.full((B,), T0, dtype=torch.int32, device=dev)
    out = torch.empty((B, cfg.hidden_size), device=dev, dtype=torch.float32)
    hid = torch.empty((B, T0, cfg.hidden_size), device=dev, dtype=torch.float32)
    times = {k: [] for k in handles}
    xb = x[:B].contiguous()

    def step(h):
      N.check(lib.gill_opt_decode_step(h, N.ptr(xb), N.ptr(lens), B, T0 + 1, N.ptr(out), stream))
    for k, h in handles.items():
      N.check(lib.gill_opt_prefill_ids(h, N.ptr(ids[:B].contiguous()), B, T0, None, 0, N.ptr(hid), stream))
      for _ in range(3):
        step(h)
    torch.cuda.synchronize()
    for _ in range(rounds):
      for k, h in handles.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
          step(h)
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / steps)
    a, b = statistics.median(times["bf16"]), statistics.median(times["w8"])
    print(f"B={B}: bf16 {a:.3f} ms (min {min(times['bf16']):.3f} max {max(times['bf16']):.3f}), w8 {b:.3f} ms (min {min(times['w8']):.3f} "
          f"max {max(times['w8']):.3f}), ratio {b / a:.3f}")
    lines.append(f"| {B} | {a:.3f} ({min(times['bf16']):.3f} - {max(times['bf16']):.3f}) | {b:.3f} ({min(times['w8']):.3f} - {max(times['w8']):.3f}) | {b / a:.2f} |")
  for h in handles.values():
    lib.gill_opt_destroy(h)
  wbytes = cfg.num_layers * (4 * cfg.hidden_size ** 2 + 2 * cfg.hidden_size * cfg.ffn_dim)
  lines += ["", f"fp8 weight bytes per iteration: {wbytes / 1e9:.2f} GB; at 5 - 6 TB/s of HBM that is {wbytes / 6e12 * 1e3:.2f} - {wbytes / 5e12 * 1e3:.2f} ms, "
            f"with {7 * cfg.num_layers} launches of fixed cost on top.", ""]


def timed_call(fn, rep):
  os.environ["GILL_OP_REPEAT"] = str(rep)
  try:
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3
  finally:
    os.environ.pop("GILL_OP_REPEAT", None)


def linears(cfg, dev, lines, r1=20, r2=120, rounds=5):
  D, F = cfg.hidden_size, cfg.ffn_dim
  g = torch.Generator(device=dev).manual_seed(1)
  lines += ["## The four linears alone (MI355X)", "",
            f"Per launch from the difference of GILL_OP_REPEAT = {r2} and {r1}, median of {rounds} alternating rounds; TB/s of weight bytes (fp8: N K, bf16: 2 N K).",
            "Back-to-back repeats of one matrix: see the caveat in the tool's docstring.", "",
            "| matrix (N x K) | M | w8 us | w8 TB/s | bf16 GEMM us | bf16 TB/s |", "|---|---|---|---|---|---|"]
  for name, Nn, K in (("qkv", 3 * D, D), ("out_proj", D, D), ("fc1", F, D), ("fc2", D, F)):
    w = (torch.randn((Nn, K), device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    w8, sc, _ = ops.w8_quant(w)
    wdq, _ = ops.w8_dequant(w8, sc, Nn, K)
    bias = torch.zeros(Nn, device=dev)
    for M in (1, 16):
      a = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
      f8 = lambda: ops.linear_w8(a, w8, sc, bias=bias, splitk=0 if name in ("out_proj", "fc2") else 1)   # noqa: E731
      fb = lambda: ops.gemm(a, wdq, bias=bias)                                                           # noqa: E731
      t8, tb = [], []
      for _ in range(rounds):
        t8.append((timed_call(f8, r2) - timed_call(f8, r1)) / (r2 - r1))
        tb.append((timed_call(fb, r2) - timed_call(fb, r1)) / (r2 - r1))
      u8, ub = statistics.median(t8), statistics.median(tb)
      print(f"{name} {Nn}x{K} M={M}: w8 {u8:.1f} us ({Nn * K / u8 / 1e6:.2f} TB/s), bf16 {ub:.1f} us ({2 * Nn * K / ub / 1e6:.2f} TB/s)")
      lines.append(f"| {name} ({Nn} x {K}) | {M} | {u8:.1f} | {Nn * K / u8 / 1e6:.2f} | {ub:.1f} | {2 * Nn * K / ub / 1e6:.2f} |")
  lines.append("")


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--profile", default=None)
  ap.add_argument("--layers", type=int, default=32)
  a = ap.parse_args()
  assert torch.cuda.is_available(), "timings are taken on the MI355X"
  dev = torch.device("cuda:0")
  cfg = synth.OptConfig(vocab_size=2048, hidden_size=4096, num_layers=a.layers, num_heads=32, ffn_dim=16384, max_positions=2048)
  lines = []
  with torch.cuda.device(dev):
    decode_iterations(cfg, dev, lines)
    linears(cfg, dev, lines)
  if a.write:
    import w8_tolerance as T
    if a.profile:
      T.PROFILE = a.profile
    T.write_section("timing", lines)
