"""Every instantiation of the register-staged attention_kernel<DP, NTHR> (csrc/attention.hip) through ops.attention, on operands that do not
average a mistake away.  The case table, the builders and their premises are in attention_inst_util; test_attention_inst_host.py shows on
the CPU which kernel each case runs (the launcher's own plan) and that each check fails, by 10 x or more, for the mistake it is there for.

  routing        every output row equals V[pi(i)] to 2^-5 (test_attention_pv48_gpu.ROUTING_BAR): V^T slot permutation, rotated tile walk,
                 d rows, the ones-row pick-up, the ragged and the causal mask;
  rescale        per row at 2e-2 (kv_cache_util.ATTN_BAR) against the fp32 oracle on the pre-scaled operands: the lazy running max's slow
                 path, half the rows of every wave jumping while the other half keeps delta = 0;
  shift          per row at 2e-2, finite: a padding key of the ragged last tile seen by the kernel would own the row;
  large scores   whole tensor at 2e-2, finite: the fp32 accumulator offset -m_run at |score| up to ~1e5;
  independence   the rescale operands twice, the second time with other queries in the upper half of every wave: the lower halves
                 must have the same bits.
The bars are the ones of the neighbouring files; profiles/attention_instantiations.md holds the measured worst rows."""
import pytest
import torch

import attention_inst_util as U

pytestmark = pytest.mark.gpu
IDS = U.case_id


def _plan(case):
  """The instantiation the case claims, checked against the function the launcher dispatches on (no table row depends on GILL_ATT_DMA)."""
  from gill_amd import ops
  family, dp, nthr = U.EXPECTED[case]
  assert ops.attention_plan(*case)[:3] == (family, dp, nthr) and family == U.REG
  return f"<{dp}, {nthr}>"


@pytest.mark.parametrize("case", U.ROUTING_CASES, ids=IDS)
def test_attention_inst_routing_rows_equal_their_v_row(cuda, case):
  """Query i is aligned with key pi(i) = (5 i + 3) mod (keys row i may see) by a lead of >= 30 in the exp2 domain; V holds small integers.
  Every output row must equal V[pi(i)] to 2^-5."""
  B, H, nq, nkv, d, causal = case
  plan = _plan(case)
  q, k, v, want, lead, oracle_err = U.routing_case(*case)
  out = U.run(q, k, v, H, causal, cuda)
  err = U.row_abs(out, want)                                                    # per (batch, head, query) row
  print(f"[attention inst routing {IDS(case)} {plan}] lead {lead:.1f}, oracle err {oracle_err:.2e}, worst row (flat {int(err.argmax())}) "
        f"err {err.max().item():.4e}, rows over the bar {(err > U.ROUTING_BAR).sum().item()} of {err.numel()}")
  assert torch.isfinite(out).all()
  assert err.max().item() <= U.ROUTING_BAR


@pytest.mark.parametrize("case", U.RESCALE_CASES, ids=IDS)
def test_attention_inst_rescale_per_row(cuda, case):
  """The running-max jump, with the two 16-row halves of every wave jumping in different tiles: test_attention's bar, per row, against the
  fp32 oracle on the kernel's own pre-scaled bf16 operands."""
  B, H, nq, nkv, d, causal = case
  plan = _plan(case)
  q, k, v, ref, lead, rest = U.rescale_case(B, H, nq, nkv, d)
  out = U.run(q, k, v, H, False, cuda)
  rel = U.row_rel(out, ref)
  print(f"[attention inst rescale {IDS(case)} {plan}] lead {lead[0]:.2f}..{lead[1]:.2f}, other keys keep {100 * rest[0]:.1f}..{100 * rest[1]:.1f} %, "
        f"worst row (flat {int(rel.argmax())}) {rel.max().item():.4e}, rows over the bar {(rel >= U.ATTN_BAR).sum().item()} of {rel.numel()}")
  assert torch.isfinite(out).all()
  assert rel.max().item() < U.ATTN_BAR


@pytest.mark.parametrize("case", U.SHIFT_CASES, ids=IDS)
def test_attention_inst_shift_padding_keys_stay_masked(cuda, case):
  """Every real score is <= -20 in the exp2 domain (a common shift: the softmax over the real keys is test_attention's); the zero padding
  keys of the ragged last tile score 0."""
  B, H, nq, nkv, d, causal = case
  plan = _plan(case)
  q, k, v, ref, top = U.shift_case(B, H, nq, nkv, d)
  out = U.run(q, k, v, H, False, cuda)
  rel = U.row_rel(out, ref)
  print(f"[attention inst shift {IDS(case)} {plan}] largest real score {top:.1f}, worst row (flat {int(rel.argmax())}) {rel.max().item():.4e}, "
        f"rows over the bar {(rel >= U.ATTN_BAR).sum().item()} of {rel.numel()}")
  assert torch.isfinite(out).all()
  assert rel.max().item() < U.ATTN_BAR


@pytest.mark.parametrize("mag", U.LARGE_MAGS)
@pytest.mark.parametrize("case", U.LARGE, ids=IDS)
def test_attention_inst_large_scores(cuda, case, mag):
  """test_attention_d40_large_scores on the register-staged kernel (d 64: explicit row sum; d 80: ones row): a spike in the last tile and
  scores far outside bf16's integer range; the reference on the pre-scaled bf16 Q."""
  B, H, nq, nkv, d, causal = case
  plan = _plan(case)
  q, k, v, ref = U.large_case(B, H, nq, nkv, d, mag)
  out = U.run(q, k, v, H, False, cuda)
  rel = U.whole_rel(out, ref)
  print(f"[attention inst large {IDS(case)} {plan} mag {mag:g}] rel_to_max {rel:.4e}, worst row {U.row_rel(out, ref).max().item():.4e}")
  assert torch.isfinite(out).all()
  assert rel < U.ATTN_BAR


@pytest.mark.parametrize("case", U.INDEPENDENCE_CASES, ids=IDS)
def test_attention_inst_rows_do_not_depend_on_their_wave(cuda, case):
  """A row that did not ask for a running-max move keeps its max: its bits do not depend on what the other rows of its wave see.  The
  queries with (i mod 32) >= 16 are replaced by ones that jump in another tile; the rows with (i mod 32) < 16 keep their bits."""
  B, H, nq, nkv, d, causal = case
  plan = _plan(case)
  q, q2, k, v, kept = U.independence_pair(B, H, nq, nkv, d)
  out = U.run(q, k, v, H, False, cuda)
  out2 = U.run(q2, k, v, H, False, cuda)
  same = torch.equal(out[:, :, kept], out2[:, :, kept])
  moved = (out[:, :, ~kept] != out2[:, :, ~kept]).any(-1)
  print(f"[attention inst independence {IDS(case)} {plan}] kept rows bit-equal: {same}; replaced rows that differ: {moved.sum().item()} of {moved.numel()}")
  assert torch.isfinite(out).all() and torch.isfinite(out2).all()
  assert same
  assert moved.all()
