"""Proof, on the CPU, that the KV-cache tests of test_kv_cache_gpu.py and the decode-offset attention tests of test_ops_gpu.py can fail.

kv_cache_util.cached_forward_ref restates gill_opt_forward_cached call by call in fp32 and can be broken in six ways (DEFECTS: newest
key of a step not visible; causal offset off by one inside a multi-token step; positions not advanced by past_len; one stale key of
an earlier sequence visible at index nkv; K/V of batch row b read from row 0; an 8-token step's V written one slot early).  Here:

  0. with defect=None the restatement reproduces oracle.opt_ref.opt_hidden_states to fp32 round-off over the whole schedule, on a
     cache that still holds an earlier, longer sequence;
  1. for every defect, at both geometries, the engine-level check of the GPU file (kv_cache_util.check_calls: same function, same
     per-call statistics, same bars, the defective output standing in for the GPU's) fails, and misses a bar by 3x or more;
  2. at the operator shapes, the attention-level defects applied to test_ops_gpu._attn_ref fail the per-row 2e-2 bar;
  3. an oracle pass with every GEMM operand (activations, Q, K, V, P) rounded to bf16 -- a CPU emulation of the kernels' arithmetic,
     not the kernels -- stays within half of each bar.

Each test prints its margin: the defect's ratio to the bar, or the emulation's.  The weights and inputs that make 1 and 3 hold together
(kv_cache_util.peaked_opt_state_dict) are the ones the GPU tests use.  Host batch: the first 2 rows of the GPU tests' inputs."""
import copy

import pytest
import torch

import kv_cache_util as U
from oracle import opt_ref

HOST_B = 2


class _Geom:
  def __init__(self, name):
    g = U.GEOMETRIES[name]
    self.name, self.cfg, self.schedule = name, g["cfg"], g["schedule"]
    self.calls = U.calls_of(self.schedule)
    self.T = sum(self.schedule)
    self.sd = U.peaked_opt_state_dict(self.cfg, g["seed"])
    self.x = U.token_embeds(self.sd, self.cfg, HOST_B, self.T, g["seed"])
    self.ref = opt_ref.opt_hidden_states(self.sd, self.cfg.num_layers, self.cfg.num_heads, self.x)
    # what an earlier sequence leaves in the handle: other tokens, 8 tokens longer, all batch rows
    prev = U.token_embeds(self.sd, self.cfg, HOST_B, self.T + 8, g["seed"] + 100)
    _, self.stale = U.cached_forward_ref(self.sd, self.cfg, prev, (self.T + 8,))

  def run(self, defect=None, rnd=None, schedule=None):
    outs, _ = U.cached_forward_ref(self.sd, self.cfg, self.x, schedule or self.schedule, defect=defect, cache=copy.deepcopy(self.stale), rnd=rnd)
    return outs


_GEOMS = {}


@pytest.fixture(params=list(U.GEOMETRIES))
def geom(request):
  if request.param not in _GEOMS:
    _GEOMS[request.param] = _Geom(request.param)
  return _GEOMS[request.param]


def test_oracle_rows_are_order_one_and_finite(geom):
  assert torch.isfinite(geom.ref).all()
  rms = geom.ref.pow(2).mean(-1).sqrt()
  print(f"[{geom.name}] oracle hidden row rms: min {rms.min().item():.3f} max {rms.max().item():.3f}")
  assert 0.3 < rms.min().item() and rms.max().item() < 3.0


def test_restatement_reproduces_oracle(geom):
  """defect=None, stale rows in the cache: fp32 round-off only.  1e-4 of the bars' scale: fp32 GEMMs of K <= 16384 carry ~1e-6
  relative error each, a dozen layers of them stay far below 3e-6 rel / 1e-7 (1 - cos)."""
  stats = U.compare_calls(f"{geom.name} restatement", geom.run(), geom.ref, geom.calls)
  ratio = U.worst_ratio(stats)
  print(f"[{geom.name}] restatement vs oracle: worst ratio to the bars {ratio:.2e}")
  assert ratio < 1e-3


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_defect_fails_the_engine_check(geom, defect):
  outs = geom.run(defect=defect)
  stats = U.compare_calls(f"{geom.name} {defect}", outs, geom.ref, geom.calls)
  ratio = U.worst_ratio(stats)
  first = next(c for c, s in enumerate(stats) if U.worst_ratio([s]) > 1.0)
  print(f"[{geom.name}] defect {defect}: worst call misses a bar by {ratio:.1f}x; first failing call {first} = (past, T_new) {geom.calls[first]}")
  with pytest.raises(AssertionError):
    U.assert_calls(stats)
  assert ratio >= 3.0


def test_bf16_emulation_stays_within_half_of_each_bar(geom):
  outs = geom.run(rnd=U.bf, schedule=(geom.T,))[0].split(list(geom.schedule), dim=1)
  stats = U.compare_calls(f"{geom.name} bf16 emulation", outs, geom.ref, geom.calls)
  ratio = U.worst_ratio(stats)
  print(f"[{geom.name}] bf16-operand emulation: worst ratio to the bars {ratio:.3f}")
  U.assert_calls(stats)
  assert ratio <= 0.5


@pytest.mark.parametrize("B,H,nq,nkv,d", U.DECODE_SHAPES)
def test_attention_defects_fail_per_row(B, H, nq, nkv, d):
  from test_ops_gpu import _attn_ref
  q, k, v = U.decode_attn_inputs(B, H, nq, nkv, d, seed=40)
  scale = d ** -0.5
  ref = _attn_ref(q, k, v, H, scale, True)
  assert torch.isfinite(ref).all()
  # the emulated kernel arithmetic (Q scaled then rounded, P rounded) stays within half of the bar on these operands
  emu = _attn_ref(U.bf(q * scale), k, v, H, 1.0, True)
  assert U.report_rows(f"attn decode B{B} H{H} {nq}x{nkv} d{d} bf16 q", emu, ref) <= U.ATTN_BAR / 2
  for defect in U.ATTN_DEFECTS:
    if not U.attn_defect_applies(defect, B, nq, nkv):
      continue
    bad = U.defective_attn_ref(_attn_ref, q, k, v, H, scale, defect)
    rel = U.report_rows(f"attn decode B{B} H{H} {nq}x{nkv} d{d} {defect}", bad, ref)
    print(f"  -> {rel / U.ATTN_BAR:.1f}x the bar")
    assert not rel < U.ATTN_BAR
