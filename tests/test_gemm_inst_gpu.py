"""Every reachable gemm_kernel instantiation against fp64, on the GPU: one operator call per case of tests/gemm_inst_util.py.

Each case clears the launcher's plan record (ops.gemm_plan_log), runs its operator once into a NaN-prefilled, guarded buffer, and asserts
  * the number of GEMM launches and that the instantiation the case names is among the plans the launcher ran — with the tile rows, N-tile walk,
    n_major / XCD block map, ragged edges and uneven split the case claims, read from the launcher's own plan, not from a descriptor of ours;
  * no NaN left in the output (a tile the tile -> workgroup map never visits shows), the guard words intact (a store past row M or column N shows);
  * the numbers: bit-equal to the rounded fp64 result on small-integer operands, and within the per-element bound
    u |ref| + (K + 4) 2^-24 S on random ones (gemm_inst_util's docstring; activations: tests/golden/gemm_inst_tolerance.json); the GEGLU, QKV,
    softmax and GroupNorm-finish epilogues under the bars of their standing operator tests;
  * a second run into a fresh buffer gives identical bits.
The last test asserts that the union of instantiations the launcher reported over the module is exactly the 56 reachable ones."""
import pytest

import gemm_inst_util as G
from test_gemm_plan_host import N_INSTANTIATIONS, UNREACHABLE

pytestmark = pytest.mark.gpu

SEEN = set()          # instantiations the launcher reported, over the module
RAN = []              # ids of the table cases that ran


@pytest.fixture(scope="module")
def terms():
  return G.act_terms()


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_instantiation(cuda, terms, case):
  G.run_case(case, cuda, terms, SEEN)
  RAN.append(case.id)


def test_every_reachable_instantiation_ran():
  if len(RAN) < len(G.CASES):
    pytest.skip(f"only {len(RAN)} of {len(G.CASES)} table cases ran (deselected or failed): the union is not the table's")
  assert not (SEEN & UNREACHABLE), sorted(SEEN & UNREACHABLE)
  want = {c.inst for c in G.CASES}
  assert SEEN >= want and len(SEEN) == N_INSTANTIATIONS - len(UNREACHABLE), (sorted(want - SEEN), sorted(SEEN - want))


def test_plan_log_keeps_the_32_most_recent(cuda):
  """35 launches: the count is 35, the record holds the last 32 oldest first, and reading it clears it."""
  import torch
  from gill_amd import ops
  w = torch.zeros(128, 64, dtype=torch.bfloat16, device=cuda)
  a64, a128 = (torch.zeros(m, 64, dtype=torch.bfloat16, device=cuda) for m in (64, 128))
  ops.gemm_plan_log()
  for i in range(35):
    ops.gemm(a64 if i < 5 else a128, w, splitk=1)
  rows, launched = ops.gemm_plan_log()
  assert launched == 35 and rows.shape == (32, 34) and (rows[:, G.R["rc"]] == 0).all()
  assert [int(m) for m in rows[:, G.R["M"]]] == [64] * 2 + [128] * 30
  assert [G.inst_of(r) for r in rows[:3]] == [(4, 128, 0, 4, 2, 64, 4)] * 2 + [(4, 128, 0, 4, 3, 64, 2)]
  assert ops.gemm_plan_log()[1] == 0
