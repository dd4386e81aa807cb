"""CPU checks of the VAE attention tests' own yardstick (tests/vae_attention_util.py): the bars of tests/test_vae_attention_gpu.py leave the
bf16-storage chain a factor of two, and every seeded mistake exceeds one of them by at least a factor of two at every tested (shape, gain)."""
import pytest
import torch

import vae_attention_util as A

SOFTMAX_SHAPES = A.SOFTMAX_SHAPES
CASES = [(*s, g) for s in A.SHAPES for g in A.GAINS]


@pytest.fixture(scope="module")
def rigs():
  out = {}
  for key in CASES:
    inp = A.attn_inputs(*key, A.case_seed(*key))
    out[key] = (inp, A.exact_of(inp))
  return out


def _run(key, inp, exact, mutate=None):
  out, P = A.attn_chain(inp, False, store=A.STORED, mutate=mutate)
  outr, _ = A.attn_chain(inp, True, store=A.STORED, mutate=mutate)
  return A.check_chain(key, out, outr, P, exact)


def test_inputs_are_bf16_representable_and_samples_differ(rigs):
  for key, (inp, _) in rigs.items():
    for name, t in inp.items():
      assert torch.equal(A.bf16_round(t), t), (key, name)
    m = inp["n"].mean(1)
    assert (m[0] - m[1]).abs().mean() > 0.1     # the per-sample offset (std 0.3 per channel)


@pytest.mark.parametrize("key", CASES, ids=str)
def test_storage_chain_stays_within_half_of_each_bar(rigs, key):
  inp, exact = rigs[key]
  for name, got, bar in _run(key, inp, exact):
    assert got <= 0.5 * bar or name == "P.rowsum" and got <= bar, (name, got, bar)


# "to_k bias dropped" is deliberately absent: bk adds the same q_i . bk to every score of row i, and a softmax cannot see a per-row constant.
@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_every_seeded_mistake_exceeds_a_bar_twofold_at_every_case(rigs, mutant):
  worst = None
  for key in CASES:
    inp, exact = rigs[key]
    res = _run(key, inp, exact, mutate=mutant)
    name, got, bar = max(res, key=lambda r: r[1] / r[2])
    if worst is None or got / bar < worst[0]:
      worst = (got / bar, key, name)
    assert got >= 2 * bar, f"{mutant} at {key}: best metric {name} = {got:.3e} is only {got / bar:.2f} x its bar {bar:.3e}"
  print(f"[vae attention mutant] {mutant}: at least {worst[0]:.1f} x a bar (weakest case {worst[1]}, metric {worst[2]})")


@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=str)
def test_fp32_softmax_emulation_passes_the_softmax_bars(shape):
  a, b = A.softmax_cases(*shape, seed=shape[1])
  ga, gb = (torch.softmax(s.float(), dim=-1).to(torch.bfloat16) for s in (a, b))
  assert A.check_softmax(ga, a) == [] and A.check_softmax(gb, b) == []
  # the special rows are what they claim to be
  uniform = torch.full((shape[1],), 1.0 / shape[1]).to(torch.bfloat16)
  assert torch.equal(ga[0], uniform) and torch.equal(gb[0], uniform)
  last = gb[-1].float()
  assert last.sum() == 1.0 and last.max() == 1.0 and torch.softmax(b.double(), dim=-1)[-1].min() < 2.0 ** -110


def test_softmax_bars_see_a_truncated_row_and_a_wrong_base():
  s = A.softmax_cases(7, 520, seed=520)[0]
  cut = s.float().clone()
  cut[:, 512:] = -float("inf")
  assert A.check_softmax(torch.softmax(cut, dim=-1).to(torch.bfloat16), s) != []
  assert A.check_softmax(torch.softmax(s.float() * 0.6931472, dim=-1).to(torch.bfloat16), s) != []
