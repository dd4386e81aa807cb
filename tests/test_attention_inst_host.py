"""Proof, on the CPU, that the cases of test_attention_inst_gpu.py run the kernels they claim and that its checks can fail.

  plan      gill_attention_plan (ops.attention_plan, host only: the function the launcher itself dispatches on) gives every row of
            attention_inst_util's table its expected (family, DP, NTHR): the non-causal rows cover all ten register-staged
            instantiations <48 | 64 | 80 | 128 | 160, 256 | 512>, the causal rows <64 | 128, 256 | 512>, test_attention_pv48_gpu's shapes both
            LDS-DMA forms — and, with GILL_ATT_DMA = 0, <48, 256 | 512> register-staged;
  premises  every builder's own assertions hold for every case it is used on (the builders assert them; here they are all built);
  defects   on these very operands attention_inst_util.emulate — the kernel's online softmax in fp32 — passes each check's bar, and the same
            emulation with one of six mistakes (attention_inst_util.DEFECTS) misses it by 10 x or more.

Each test prints its margins."""
import pytest

import attention_inst_util as U
from gill_amd import ops

IDS = U.case_id


# ------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("case", list(U.EXPECTED), ids=IDS)
def test_plan_of_every_table_row(case):
  B, H, nq, nkv, d, causal = case
  family, dp, nthr, grid = ops.attention_plan(B, H, nq, nkv, d, causal)
  print(f"[attention plan {IDS(case)}] family {family} DP {dp} NTHR {nthr} grid {grid}")
  assert (family, dp, nthr) == U.EXPECTED[case]
  # one workgroup per (XCD, pair slot, query tile): whole rounds of eight pairs, surplus workgroups exit
  assert grid == 8 * ((B * H + 7) // 8) * ((nq + nthr // 2 - 1) // (nthr // 2))
  assert ops.attention_plan(B, H, nq, nkv, d, causal, att_dma=0) == (family, dp, nthr, grid)      # (no table row is DMA-eligible)


def test_plan_covers_twelve_instantiations():
  plans = {c: ops.attention_plan(*c)[:3] for c in U.EXPECTED}
  noncausal = {plans[c] for c in U.NONCAUSAL}
  assert noncausal == {(U.REG, dp, nthr) for dp in (48, 64, 80, 128, 160) for nthr in (256, 512)}
  causal = {plans[c] for c in U.CAUSAL256 + U.CAUSAL512}
  assert causal == {(U.REG, dp, nthr) for dp in (64, 128) for nthr in (256, 512)}
  pv48 = {c: ops.attention_plan(*c)[:3] for c in U.PV48_EXPECTED}
  assert pv48 == U.PV48_EXPECTED
  assert {p for p in pv48.values() if p[0] == U.DMA} == {(U.DMA, 48, 256), (U.DMA, 48, 512)}
  off = {c: ops.attention_plan(*c, att_dma=0) for c in U.PV48_EXPECTED}
  assert {p[:3] for p in off.values()} == {(U.REG, 48, 256), (U.REG, 48, 512)}
  for c, p in off.items():      # the switch changes the family, never the workgroup size or the grid
    assert p[1:] == ops.attention_plan(*c)[1:]
  print(f"[attention plan] register-staged non-causal {sorted(noncausal)}, causal {sorted(causal)}, LDS-DMA {sorted(set(pv48.values()))}")


def test_plan_restates_the_launcher_rules_over_a_sweep():
  """The rules attention_launch() had inline before the plan existed, restated here and compared over ~16000 shapes under both values of
  GILL_ATT_DMA: 512 threads when cdiv(nq, 256) * B * H >= 256; the LDS-DMA kernel for d = 40 in DP 48, no mask, whole query tiles and
  nkv_pad % 64 == 0; one workgroup per (XCD, pair slot, query tile)."""
  cdiv = lambda a, b: (a + b - 1) // b
  n = 0
  for B in (1, 2, 3, 8, 43):
    for H in (1, 8, 12, 16, 32):
      for nq in (1, 33, 128, 256, 257, 300, 2048, 4096):
        for nkv in (1, 64, 77, 100, 192, 200, 4096):
          for d in (40, 48, 64, 80, 128, 160):
            for causal in (False, True):
              for att_dma in (1, 0):
                nthr = 512 if cdiv(nq, 256) * B * H >= 256 else 256
                dma = bool(att_dma) and d == 40 and not causal and nq % (nthr // 2) == 0 and (cdiv(nkv, 32) * 32) % 64 == 0
                want = (U.DMA if dma else U.REG, U.padded(d), nthr, 8 * cdiv(B * H, 8) * cdiv(nq, nthr // 2))
                assert ops.attention_plan(B, H, nq, nkv, d, causal, att_dma) == want, (B, H, nq, nkv, d, causal, att_dma)
                n += 1
  print(f"[attention plan] {n} shapes agree with the restated rules")


def test_plan_thresholds_and_errors():
  """The 512 form starts at cdiv(nq, 256) * B * H = 256; the LDS-DMA kernel needs d = 40, no mask, whole query tiles and nkv_pad % 64 == 0."""
  assert ops.attention_plan(1, 255, 256, 64, 64)[2] == 256 and ops.attention_plan(1, 256, 256, 64, 64)[2] == 512
  assert ops.attention_plan(1, 128, 257, 64, 64)[2] == 512
  assert ops.attention_plan(1, 2, 128, 128, 40)[0] == U.DMA
  for B, H, nq, nkv, d, causal in ((1, 2, 128, 128, 40, True), (1, 2, 100, 128, 40, False), (1, 2, 128, 96, 40, False), (1, 2, 128, 128, 48, False),
                                   (1, 256, 128, 128, 40, False)):      # (the last: 512 threads want 256-query tiles)
    assert ops.attention_plan(B, H, nq, nkv, d, causal)[0] == U.REG, (B, H, nq, nkv, d, causal)
  for bad in ((0, 1, 1, 1, 64), (1, 1, 0, 1, 64), (1, 1, 1, 1, 161)):
    with pytest.raises(Exception):
      ops.attention_plan(*bad)


# ------------------------------------------------------------------------------------------------ premises and defects
def _report(tag, good, bad, bar):
  print(f"[{tag}] emulation as built {good:.3e} ({good / bar:.3f} of the bar); " + ", ".join(f"{df} {b / bar:.1f}x" for df, b in bad.items()))
  assert good <= bar
  for df, b in bad.items():
    assert b >= 10 * bar, (df, b)


@pytest.mark.parametrize("case", U.ROUTING_CASES, ids=IDS)
def test_routing_premises_and_defects(case):
  """(a) exchanged V blocks, (b) a wrong wrap of query tile 1's walk, (c) the row sum from the wrong O^T row: whole-number errors."""
  B, H, nq, nkv, d, causal = case
  nthr = U.EXPECTED[case][2]
  q, k, v, want, lead, oracle_err = U.routing_case(*case)
  good = U.row_abs(U.emulate(q, k, v, H, nthr, causal), want).max().item()
  bad = {df: U.row_abs(U.emulate(q, k, v, H, nthr, causal, df), want).max().item()
         for df in ("v_blocks_exchanged", "walk_wraps_wrong", "row_sum_wrong_row") if U.defect_applies(df, case) and nkv > 16}
  _report(f"routing {IDS(case)} lead {lead:.1f} oracle {oracle_err:.1e}", good, bad, U.ROUTING_BAR)


@pytest.mark.parametrize("case", U.RESCALE_CASES, ids=IDS)
def test_rescale_premises_and_defects(case):
  """(d) a jump that rescales O but not l_run (DP 64 / 128 / 160), (e) a jump that rescales every row of the wave by the wave's largest delta."""
  B, H, nq, nkv, d, causal = case
  nthr = U.EXPECTED[case][2]
  q, k, v, ref, lead, rest = U.rescale_case(B, H, nq, nkv, d)
  good = U.row_rel(U.emulate(q, k, v, H, nthr), ref).max().item()
  bad = {df: U.row_rel(U.emulate(q, k, v, H, nthr, False, df), ref).max().item()
         for df in ("l_not_rescaled", "wave_max_delta") if U.defect_applies(df, case)}
  _report(f"rescale {IDS(case)} lead {lead[0]:.2f}..{lead[1]:.2f}, other keys keep {100 * rest[0]:.1f}..{100 * rest[1]:.1f} %", good, bad, U.ATTN_BAR)
  assert len(bad) == (2 if U.padded(d) % 32 == 0 else 1)


@pytest.mark.parametrize("case", U.INDEPENDENCE_CASES, ids=IDS)
def test_independence_pair_premises(case):
  B, H, nq, nkv, d, causal = case
  q, q2, k, v, kept = U.independence_pair(B, H, nq, nkv, d)
  assert case in U.RESCALE_CASES and kept.sum().item() * 2 >= nq - 16
  assert U.torch.equal(q[:, kept], q2[:, kept])


def test_independence_cases_cover_every_dp_and_both_forms():
  plans = {U.EXPECTED[c] for c in U.INDEPENDENCE_CASES}
  assert {p[1] for p in plans if p[2] == 256} == {48, 64, 80, 128, 160} and any(p[2] == 512 for p in plans)


@pytest.mark.parametrize("case", U.SHIFT_CASES, ids=IDS)
def test_shift_premises_and_defects(case):
  """(f) the zero padding keys of the ragged last tile visible: they score 0 against real scores <= -20 and own the row."""
  B, H, nq, nkv, d, causal = case
  nthr = U.EXPECTED[case][2]
  assert U.defect_applies("padding_visible", case)
  q, k, v, ref, top = U.shift_case(B, H, nq, nkv, d)
  good = U.row_rel(U.emulate(q, k, v, H, nthr), ref).max().item()
  bad = {"padding_visible": U.row_rel(U.emulate(q, k, v, H, nthr, False, "padding_visible"), ref).max().item()}
  _report(f"shift {IDS(case)} largest real score {top:.1f}", good, bad, U.ATTN_BAR)


@pytest.mark.parametrize("mag", U.LARGE_MAGS)
@pytest.mark.parametrize("case", U.LARGE, ids=IDS)
def test_large_scores_emulation_meets_the_bar(case, mag):
  B, H, nq, nkv, d, causal = case
  q, k, v, ref = U.large_case(B, H, nq, nkv, d, mag)
  assert U.torch.isfinite(ref).all()
  good = U.whole_rel(U.emulate(q, k, v, H, U.EXPECTED[case][2]), ref)
  print(f"[large {IDS(case)} mag {mag:g}] emulation as built {good:.3e} ({good / U.ATTN_BAR:.3f} of the bar)")
  assert good < U.ATTN_BAR


def test_every_listed_defect_is_caught_somewhere():
  """Each of the six mistakes applies to at least one case of the builder that is meant to catch it, at every DP it can occur at."""
  by = {"v_blocks_exchanged": U.ROUTING_CASES, "walk_wraps_wrong": U.ROUTING_CASES, "row_sum_wrong_row": U.ROUTING_CASES,
        "l_not_rescaled": U.RESCALE_CASES, "wave_max_delta": U.RESCALE_CASES, "padding_visible": U.SHIFT_CASES}
  assert set(by) == set(U.DEFECTS)
  dps = {df: {(U.padded(c[4]), U.EXPECTED[c][2]) for c in cases if U.defect_applies(df, c) and c[3] > 16} for df, cases in by.items()}
  both = lambda s: {(dp, n) for dp in s for n in (256, 512)}
  assert dps["v_blocks_exchanged"] == dps["wave_max_delta"] == dps["padding_visible"] == dps["walk_wraps_wrong"] == both((48, 64, 80, 128, 160))
  # (DP 160 = 5 * 32 has no spare V^T row: like 64 and 128 it sums its row explicitly, AttCfg::HAS_ONES)
  assert dps["row_sum_wrong_row"] == both((48, 80)) and dps["l_not_rescaled"] == both((64, 128, 160))
