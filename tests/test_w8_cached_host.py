"""Proof, on the CPU, that test_w8_cached_gpu.py can fail: test_kv_cache_host.py's argument repeated on the QUANTISED model, the weights the
w8 handle's cached forward computes with (w8_util.w8_state_dict of kv_cache_util.peaked_opt_state_dict).

  1. every defect of kv_cache_util.DEFECTS, put into kv_cache_util.cached_forward_ref on the dequantised weights, fails the engine-level
     check (kv_cache_util.check_calls: the same function, statistics and bars the GPU file uses against opt_ref on the same weights) and
     misses a bar by 3x or more, at both geometries;
  2. the bf16-operand emulation of the kernels' arithmetic on those weights stays within half of each bar;
  3. the quantised and the unquantised oracle differ by more than REL_BAR: a cached forward that ran on the original weights, or a
     reference on them, would not pass for the other.

Each test prints its measured factor.  Host batch: the first 2 rows of the GPU tests' inputs."""
import copy

import pytest
import torch

import kv_cache_util as U
import w8_util as W
from oracle import opt_ref

HOST_B = 2


class _Geom:
  def __init__(self, name):
    g = U.GEOMETRIES[name]
    self.name, self.cfg, self.schedule = name, g["cfg"], g["schedule"]
    self.calls = U.calls_of(self.schedule)
    self.T = sum(self.schedule)
    self.sd = U.peaked_opt_state_dict(self.cfg, g["seed"])
    self.sdq = W.w8_state_dict(self.sd, self.cfg)
    self.x = U.token_embeds(self.sd, self.cfg, HOST_B, self.T, g["seed"])
    self.ref = opt_ref.opt_hidden_states(self.sdq, self.cfg.num_layers, self.cfg.num_heads, self.x)
    # what an earlier sequence leaves in the handle: other tokens, 8 tokens longer, all batch rows
    prev = U.token_embeds(self.sd, self.cfg, HOST_B, self.T + 8, g["seed"] + 100)
    _, self.stale = U.cached_forward_ref(self.sdq, self.cfg, prev, (self.T + 8,))

  def run(self, defect=None, rnd=None, schedule=None):
    outs, _ = U.cached_forward_ref(self.sdq, self.cfg, self.x, schedule or self.schedule, defect=defect, cache=copy.deepcopy(self.stale), rnd=rnd)
    return outs


_GEOMS = {}


@pytest.fixture(params=list(U.GEOMETRIES))
def geom(request):
  if request.param not in _GEOMS:
    _GEOMS[request.param] = _Geom(request.param)
  return _GEOMS[request.param]


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_defect_fails_the_engine_check_on_the_dequantised_weights(geom, defect):
  stats = U.compare_calls(f"{geom.name} w8 {defect}", geom.run(defect=defect), geom.ref, geom.calls)
  ratio = U.worst_ratio(stats)
  print(f"[{geom.name}] dequantised weights, defect {defect}: worst call misses a bar by {ratio:.1f}x")
  with pytest.raises(AssertionError):
    U.assert_calls(stats)
  assert ratio >= 3.0


def test_bf16_emulation_stays_within_half_of_each_bar_on_the_dequantised_weights(geom):
  outs = geom.run(rnd=U.bf, schedule=(geom.T,))[0].split(list(geom.schedule), dim=1)
  stats = U.compare_calls(f"{geom.name} w8 bf16 emulation", outs, geom.ref, geom.calls)
  ratio = U.worst_ratio(stats)
  print(f"[{geom.name}] dequantised weights, bf16-operand emulation: worst ratio to the bars {ratio:.3f}")
  U.assert_calls(stats)
  assert ratio <= 0.5


def test_quantised_and_unquantised_oracles_differ_by_more_than_the_bar(geom):
  plain = opt_ref.opt_hidden_states(geom.sd, geom.cfg.num_layers, geom.cfg.num_heads, geom.x)
  rel = ((geom.ref - plain).norm() / plain.norm()).item()
  print(f"[{geom.name}] quantised vs unquantised oracle: rel-L2 {rel:.3e} (REL_BAR {U.REL_BAR})")
  assert rel > U.REL_BAR
