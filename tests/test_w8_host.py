"""The w8 format and the bars of its operator test, on the CPU (tests/w8_util.py; no GPU, no library).

Format: on kv_cache_util.peaked_opt_state_dict weights plus two constructed rows (all zero; one 100 x outlier) the dequantised values are
bf16 numbers, max|w / s| lies in (224, 448], |w8 s - w| <= 2^-4 |w| wherever |w| >= 2^-6 s (the e4m3 normal range: 3 mantissa bits, half
an ulp is 2^-4 relative), and the zero row gives zero bytes and s = 1.

Bars: w8_util.W8_ACC_DIST is re-measured (tools/w8_tolerance.py's figure) and each way the kernel could be wrong, emulated on the CPU,
misses the operator bar (10 x that distance, times the magnitude) by 3 x or more; the factors are printed.  `padding_rows_nan` cannot
reach a stored row of this kernel: the activation rows are the 16 columns of the MFMA's second operand and no output element mixes two of
them.  It is therefore measured on the 16-row accumulator tile the emulation returns (rows M .. 15 must hold bias-only values); on the GPU
the canary test of test_w8_ops_gpu.py covers what those rows could do, namely be stored."""
import pytest
import torch

import kv_cache_util as U
import w8_util as W


def _rows():
  g = U.GEOMETRIES["opt125"]
  sd = U.peaked_opt_state_dict(g["cfg"], g["seed"])
  w = sd["model.decoder.layers.0.fc1.weight"].float()[:62].clone()        # (62, 768)
  zero = torch.zeros(1, w.shape[1])
  outlier = w[:1].clone()
  outlier[0, 5] = U.bf(100.0 * outlier.abs().max())
  return torch.cat([w, zero, outlier])       # 64 rows: 62 = zero, 63 = outlier


def test_format_properties():
  w = _rows()
  q, s = W.quantise(w)
  dq = W.dequantise(q, s)
  assert torch.equal(U.bf(dq), dq), "a dequantised value is not a bf16 number"
  r = (w / s[:, None]).abs().amax(1)
  nz = w.abs().amax(1) > 0
  assert bool(((r[nz] > 224) & (r[nz] <= 448)).all()), (r.min().item(), r.max().item())
  assert torch.isfinite(q.float()).all(), "a NaN code was produced"
  normal = w.abs() >= (2.0 ** -6) * s[:, None]
  err = (dq - w).abs()
  assert bool((err[normal] <= 2.0 ** -4 * w.abs()[normal]).all()), (err[normal] / w.abs()[normal]).max().item()
  assert bool((err <= 2.0 ** -10 * s[:, None] + 2.0 ** -4 * w.abs()).all())      # below the normal range: half a subnormal step
  assert s[62].item() == 1.0 and int(q[62].view(torch.uint8).max()) == 0
  assert bool((torch.log2(s) == torch.log2(s).round()).all()), "a scale is no power of two"
  # the outlier row: its scale follows the outlier, the rest of the row lands in the subnormals or at zero, still within the bound above
  assert s[63] > 32 * s[0]
  # every finite e4m3 code times a power of two is a bf16 number
  codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
  codes = codes[torch.isfinite(codes)]
  assert codes.numel() == 254
  for e in (-100, -20, 0, 7, 100):
    v = codes * 2.0 ** e
    assert torch.equal(U.bf(v), v)


def test_kernel_order_is_a_permutation_with_the_documented_index():
  N, K = 64, 128
  q = torch.arange(N * K, dtype=torch.int64).remainder(251).to(torch.uint8).view(N, K).view(torch.float8_e4m3fn)
  b = W.kernel_order(q)
  raw = q.view(torch.uint8)
  for n, k in ((0, 0), (17, 5), (63, 127), (31, 64), (16, 79)):
    idx = ((n // 16) * (K // 64) + k // 64) * 1024 + ((k % 64) // 16 * 16 + n % 16) * 16 + k % 16
    assert b[idx] == raw[n, k]


def test_recorded_distance_is_the_measured_one():
  worst = max(W.acc_distance(N, K, M, sk, seed=100 + ci) for ci, (N, K, sk) in enumerate(W.OP_CASES) if N * K <= 768 * 3072
              for M in sorted(set(W.OP_ROWS)))
  print(f"largest accumulation distance {worst:.3e}; recorded W8_ACC_DIST {W.W8_ACC_DIST:.3e}")
  assert worst <= 1.25 * W.W8_ACC_DIST and W.W8_ACC_DIST <= 1.5 * worst


def test_quantisation_moves_the_oracle_by_3_bars():
  """For test_w8_decode_gpu.py's last check: the oracle on sd against the oracle on w8_state_dict(sd) on run b3's rows (opt125 geometry):
  some step's rel-L2 is 3 x the agreement bar (kv_cache_util.CACHED_VS_FULL_REL_BAR) or more."""
  import ragged_decode_util as R
  g = U.GEOMETRIES["opt125"]
  cfg, sd = g["cfg"], U.peaked_opt_state_dict(g["cfg"], g["seed"])
  lengths, steps = R.RUNS["b3"]
  seqs, _, _ = R.ragged_inputs(sd, cfg, lengths, steps, g["seed"] + 10)
  _, a = R.oracle_rows(sd, cfg, seqs, lengths, steps)
  _, b = R.oracle_rows(W.w8_state_dict(sd, cfg), cfg, seqs, lengths, steps)
  rel = max(((a[:, s] - b[:, s]).norm() / a[:, s].norm()).item() for s in range(steps))
  print(f"oracle on sd vs oracle on w8_state_dict(sd): largest per-step rel-L2 {rel:.3e} = {rel / U.CACHED_VS_FULL_REL_BAR:.1f} x the bar")
  assert rel >= 3 * U.CACHED_VS_FULL_REL_BAR


def test_generate_margin_claim_holds_on_the_dequantised_weights():
  """tests/golden/w8_generate_tolerance.json (tools/w8_tolerance.py --write): the oracle's greedy run on w8_state_dict of the gen_model
  weights, prompts of the recorded seed, has no decision with a top-2 margin under m, and m is 10 x the measured logit distance."""
  import json
  import os
  import ragged_decode_util as R
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w8_generate_tolerance.json")) as f:
    rec = json.load(f)
  cfg, sd = R.gen_model()
  sdq = W.w8_state_dict(sd, cfg)
  ids, lens = R.gen_prompt_ids(rec["seed"])
  runs = [R.oracle_greedy(sdq, cfg, ids[b, :n]) for b, n in enumerate(lens)]
  dist, margin = max(r[3] for r in runs), min(min(r[1]) for r in runs)
  print(f"logit distance {dist:.4f} (recorded {rec['largest_logit_distance']:.4f}), smallest margin {margin:.4f}, m = {rec['m']:.4f}")
  assert margin >= rec["m"] and rec["m"] >= 10 * dist * 0.99


@pytest.mark.parametrize("out_bf16", [False, True])
def test_every_defect_misses_the_operator_bar(out_bf16):
  """(N, K) = (192, 320), M = 3, two K slices, bias + ReLU: every defect applies.  The sound emulation stays under the bar."""
  N, K, M, sk = 192, 320, 3, 2
  o = W.operands(N, K, M, seed=7)
  q, s = W.quantise(o["w"])
  qv = q.float()
  ref = torch.zeros(16, N, dtype=torch.float64)
  ref[:M] = W.reference_linear(o["A"], qv, s, o["bias"], None, "relu")
  ref[M:] = torch.relu(o["bias"].double())[None]          # the padding rows' accumulators: zero products
  mag = torch.zeros(16, N, dtype=torch.float64)
  mag[:M] = W.magnitude(o["A"], qv, s, o["bias"])
  mag[M:] = o["bias"].double().abs()[None] + 1e-30
  bar = W.element_bar(ref, mag, out_bf16)
  sound = W.figure("sound", W.emulate_linear(o["A"], qv, s, o["bias"], None, "relu", sk, out_bf16), ref, bar)
  assert sound <= 1.0
  for d in W.DEFECTS:
    f = W.figure(d, W.emulate_linear(o["A"], qv, s, o["bias"], None, "relu", sk, out_bf16, defect=d), ref, bar)
    print(f"defect {d} (bf16 out: {out_bf16}): misses the bar by {f:.1f} x")
    assert f >= 3.0, (d, f)
