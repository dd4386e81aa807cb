"""CPU-side evidence that tests/test_gn_stats_gpu.py would notice a subtly wrong kernel (no GPU, nothing provoked): for every geometry of that
file the fp32 emulations of gn_stats_util meet half the bars, every defect of its lists fails the very check the GPU test applies by 2x or
more, and the host-made partials add up to the fp64 totals."""
import pytest
import torch

import gn_stats_util as U


@pytest.mark.parametrize("name", list(U.PRODUCER_CASES))
def test_producer_partials_emulation_and_defects(name):
  c = U.producer_case(name)
  y = U.bf(c["ref"])
  for slab_rows in sorted({64, U.expected_slab_rows(name)}):
    ref, den = U.partials_ref(y, slab_rows, c["bin"], c["ups"])
    emu = U.partials_figure(f"{name} rows {slab_rows} emulation", U.emulate_partials(y, slab_rows, c["bin"], c["ups"]), ref, den)
    assert emu <= 0.5 * U.STAT_BAR, f"fp32 emulation at {emu:.3e}"
    for defect in U.PRODUCER_DEFECTS:
      if not U.producer_defect_applies(defect, name):
        continue
      bad = U.partials_ref(y, slab_rows, c["bin"], c["ups"], defect=defect, unrounded=c["ref"], resid=c.get("resid"))[0]
      fig = U.partials_figure(f"{name} rows {slab_rows} {defect}", bad, ref, den)
      assert fig >= 2 * U.STAT_BAR, f"{defect} would pass: {fig:.3e}"


def _consumer_figures(tag, case, silu, eps, defect=None):
  C1, bin1, C2, bin2, B, HW, ns1, ns2 = case
  x1, st1, x2, st2, gamma, beta = U.consumer_case(*case)
  y, table = U.emulate_apply(x1, st1, bin1, gamma, beta, U.GROUPS, eps, silu, x2, st2, bin2, defect=defect)
  x = x1 if x2 is None else torch.cat([x1, x2], -1)
  yf = U.group_figure(tag, y, U.groupnorm_ref(x, U.GROUPS, gamma, beta, eps, silu), U.GROUPS)
  tf = U.table_figure(tag, table, x, U.GROUPS, gamma, beta, eps) if C2 == 0 else None     # the table is single-source only
  return yf, tf


def _check_consumer(case, silu, eps):
  C1, bin1, C2, bin2, B, HW, ns1, ns2 = case
  x1, st1, x2, st2, _, _ = U.consumer_case(*case)
  for x, st, bin in ((x1, st1, bin1),) + (((x2, st2, bin2),) if C2 else ()):
    tot = U.bin_totals(x, bin)
    assert ((st.double().sum(1) - tot).abs() <= 1e-7 * tot.abs()).all(), "host-made partials do not add up to the totals"
    assert (st * tot[:, None].sign().float() > 0).all(), "shares must be positive fractions of their total"
  tag = f"C {C1}/{bin1}+{C2}/{bin2} HW {HW} ns {ns1},{ns2}"
  yf, tf = _consumer_figures(tag + " emulation", case, silu, eps)
  assert yf <= 0.5 * U.Y_BAR and (tf is None or tf <= 0.5 * U.STAT_BAR), f"fp32 emulation at y {yf:.3e} table {tf}"
  for defect in U.CONSUMER_DEFECTS:
    if not U.consumer_defect_applies(defect, C1, bin1, C2, bin2, ns1, ns2):
      continue
    yf, tf = _consumer_figures(f"{tag} {defect}", case, silu, eps, defect)
    # the GPU test asserts y < Y_BAR and, single source, table < STAT_BAR: a defect must fail one of them by 2x
    assert yf >= 2 * U.Y_BAR or (tf is not None and tf >= 2 * U.STAT_BAR), f"{defect} would pass: y {yf:.3e} table {tf}"


@pytest.mark.parametrize("C,bin,B,HW,ns,silu,eps", U.one_block_cases())
def test_consumer_one_block_emulation_and_defects(C, bin, B, HW, ns, silu, eps):
  _check_consumer((C, bin, 0, 0, B, HW, ns, 0), silu, eps)


@pytest.mark.parametrize("C1,bin1,C2,bin2,B,HW,ns1,ns2,silu,eps", U.two_block_cases())
def test_consumer_two_blocks_emulation_and_defects(C1, bin1, C2, bin2, B, HW, ns1, ns2, silu, eps):
  _check_consumer((C1, bin1, C2, bin2, B, HW, ns1, ns2), silu, eps)


def test_every_listed_defect_is_exercised_somewhere():
  used_p = {d for d in U.PRODUCER_DEFECTS for n in U.PRODUCER_CASES if U.producer_defect_applies(d, n)}
  cases = [(C, bin, 0, 0, ns, 0) for C, bin, _, _, ns, _, _ in U.one_block_cases()] + [(c[0], c[1], c[2], c[3], c[6], c[7]) for c in U.two_block_cases()]
  used_c = {d for d in U.CONSUMER_DEFECTS for c in cases if U.consumer_defect_applies(d, *c)}
  assert used_p == set(U.PRODUCER_DEFECTS) and used_c == set(U.CONSUMER_DEFECTS)
