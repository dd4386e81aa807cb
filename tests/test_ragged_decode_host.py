"""Proof, on the CPU, that the ragged decode tests of test_ragged_decode_gpu.py can fail.

ragged_decode_util.ragged_ref restates the ragged run (padded prefill, then one token per row at per-row lengths) in fp32 and can be
broken in six ways (DEFECTS).  The reference is every row as its own sequence through oracle.opt_ref.opt_hidden_states.  Here, on the
runs and the weights the GPU tests use (opt125 geometry, kv_cache_util.peaked_opt_state_dict):

  0. with defect=None the restatement reproduces the reference to fp32 round-off, on a cache that still holds an earlier sequence;
  1. every defect fails the engine-level check (same statistics, same bars) and misses a bar by 3x or more;
  2. the restatement with every GEMM operand rounded to bf16 stays within half of each bar;
  3. on the prompts of test_generate_batch_gpu.py the oracle's own greedy run has no decision with a top-2 margin under that test's
     near-tie bar m, and the recorded m is 10 x the bf16 emulation's logit distance from the oracle.

Each test prints its factor."""
import copy

import pytest
import torch

import kv_cache_util as U
import ragged_decode_util as R

MISS = 3.0


class _Run:
  def __init__(self, name):
    g = U.GEOMETRIES["opt125"]
    self.name, self.cfg = name, g["cfg"]
    self.lengths, self.steps = R.RUNS[name]
    self.sd = U.peaked_opt_state_dict(self.cfg, g["seed"])
    self.seqs, self.prompt, self.step_x = R.ragged_inputs(self.sd, self.cfg, self.lengths, self.steps, g["seed"] + 10)
    self.oracle = R.oracle_rows(self.sd, self.cfg, self.seqs, self.lengths, self.steps)
    # what an earlier, longer sequence leaves in the handle
    B, T = len(self.lengths), max(self.lengths) + self.steps + 8
    _, self.stale = U.cached_forward_ref(self.sd, self.cfg, U.token_embeds(self.sd, self.cfg, B, T, g["seed"] + 110), (T,))

  def stats(self, tag, defect=None, rnd=None):
    pre_h, step_h, _ = R.ragged_ref(self.sd, self.cfg, self.prompt, self.lengths, self.step_x, defect=defect, rnd=rnd,
                                    cache=copy.deepcopy(self.stale))
    return R.compare_ragged(f"{self.name} {tag}", pre_h, step_h, self.oracle[0], self.oracle[1], self.lengths)


_RUNS = {}


@pytest.fixture(params=list(R.RUNS))
def run(request):
  if request.param not in _RUNS:
    _RUNS[request.param] = _Run(request.param)
  return _RUNS[request.param]


def test_restatement_reproduces_the_reference(run):
  ratio = U.worst_ratio(run.stats("restatement"))
  print(f"[{run.name}] ragged restatement vs per-row oracle: worst ratio to the bars {ratio:.2e}")
  assert ratio < 1e-3


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_fails_the_engine_check(run, defect):
  stats = run.stats(defect, defect=defect)
  ratio = U.worst_ratio(stats)
  print(f"[{run.name}] defect {defect}: worst call misses a bar by {ratio:.1f}x")
  with pytest.raises(AssertionError):
    U.assert_calls(stats)
  assert ratio >= MISS


def test_oracle_greedy_run_of_the_end_to_end_prompts_has_no_near_tie():
  """test_generate_batch_gpu.py excuses a token disagreement only inside the bar m (tools/ragged_decode_tolerance.py: 10 x the logit
  distance of the bf16 emulation from the oracle).  The prompts are chosen so that the reference itself needs no excuse: the oracle's own
  greedy run has no decision with a top-2 margin under m, and the recorded m is 10 x the distance measured here."""
  m = R.load_gen_tolerance()
  cfg, sd = R.gen_model()
  ids, lens = R.gen_prompt_ids()
  runs = [R.oracle_greedy(sd, cfg, ids[b, :n]) for b, n in enumerate(lens)]
  dist, margin = max(r[3] for r in runs), min(min(r[1]) for r in runs)
  print(f"[generate_batch prompts] bf16 emulation vs oracle logit distance {dist:.3e}, m = {m:.3e}; smallest oracle top-2 margin {margin:.3e}")
  assert abs(m - 10 * dist) <= 1e-3 * m
  assert margin >= m


def test_bf16_emulation_stays_within_half_of_each_bar(run):
  stats = run.stats("bf16 emulation", rnd=U.bf)
  ratio = U.worst_ratio(stats)
  print(f"[{run.name}] bf16-operand emulation: worst ratio to the bars {ratio:.3f}")
  U.assert_calls(stats)
  assert ratio <= 0.5
