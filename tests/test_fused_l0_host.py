"""Proof, on the CPU, that the checks of test_fused_l0_gpu.py rest on premises that hold and that each of them can fail.

  premises  every builder of fused_l0_util asserts its own (exact representability, row classes in every wave, plane splits, the rotation
            of the big run): here they are all built;
  bars      fused_l0_util's emulation of ffn.hip / lnproj.hip — the kernels' dataflow in fp32 with their rounding points — meets every check;
            its worst rows against fp64 are the figures the GPU test's bars come from (fused_l0_util.row_bar);
  defects   the same emulation with one mistake (fused_l0_util.DEFECTS) misses the check named for it: the fp64 comparisons and the hidden-unit
            sweep by 10 x the bar or more, the exact checks by a whole unit or more on at least one row.

Each test prints its margins."""
import pytest
import torch

import fused_l0_util as U

MARGIN = 10.0


# ------------------------------------------------------------------------------------------------ premises
def test_builders_premises_hold():
  for form in U.FORMS_LNPROJ:
    U.exact_lnproj(form)
  U.exact_ffn_pre()
  for pre in (False, True):
    U.rowclass_ffn(pre)
    U.position_ffn(pre)
    for pattern in ("gate", "value"):
      for p in range(4):
        U.sweep_case(pre, pattern, p)
  for mode in (0, 1):
    U.rowclass_lnproj(mode)
    for B, HW in U.GEOMETRY:
      a = U.geometry_case(mode, B, HW)
      assert (B * HW) % 128 == 0 and HW % 32 == 0 and a["x"].shape == (B * HW, U.C)
  for form in U.FORMS_LNPROJ:
    U.position_lnproj(form)
  src = U.big_index()
  assert src.numel() == 128 * U.BIG_TILES
  for planes in (3, 5):
    a, _ = U.planes_case(planes)
    one = torch.stack([a["t"].sum(1), (a["t"] ** 2).sum(1)], 1)
    got = a["ln_stats"].sum(0)
    # the planes' sum is the one-plane value up to fp32 addition order: close, and (on some row) not the same bits
    assert torch.allclose(got, one, rtol=1e-5, atol=1e-4)
    print(f"[fused_l0 planes {planes}] {int((got != one).any(1).sum())} of {one.shape[0]} rows differ from the one-plane sums in their last bits")
  U.wrap_case()
  assert set(U.perm16(U.H).tolist()) == set(range(U.H)) and U.perm16(16).tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def test_constant_row_never_reaches_the_clamp_in_lane():
  """Why var_not_clamped is shown on the planes-fed kernel only: summed in the lane, a constant bf16 row has variance exactly 0."""
  for quad in (False, True):
    s, q, mean, var = U.constant_row_stats(quad)
    print(f"[fused_l0 constant row, {'lnproj' if quad else 'ffn PRE'} order] sum {s} sum of squares {q} mean {mean} one-pass variance {var}")
    assert (s, q, mean, var) == (U.CONSTANT * U.C, U.CONSTANT ** 2 * U.C, U.CONSTANT, 0.0)


def test_gelu_restatement_is_inside_the_documented_bound():
  worst, ratio = U.gelu_restatement_ratio()
  print(f"[fused_l0 gelu_logistic restated] largest |error| on [-12, 12] {worst:.3e} = {ratio:.3f} of common.h's {U.GELU_DOC}")
  assert ratio < 1.0


# ------------------------------------------------------------------------------------------------ the checks, on the emulation
def b1_lnproj(form, defect=None):
  a, want = U.exact_lnproj(form)
  return U.exact_diff(f"B1 lnproj {form} {defect or 'emulation'}", U.emulate_lnproj(a, defect)[0], want)


def b1_ffn_pre(defect=None):
  a, want = U.exact_ffn_pre()
  return U.exact_diff(f"B1 ffn PRE {defect or 'emulation'}", U.emulate_ffn(a, defect), want)


def b2(kind, defect=None, cls=None):
  """(worst row over the bar's rows, bar); cls: one row class only"""
  sel = slice(None) if cls is None else slice(U.ROW_CLASSES.index(cls), None, U.NCLS)
  if kind.startswith("ffn"):
    a, ref = U.rowclass_ffn(kind == "ffn_pre")
    errs = {"out": U.row_err(U.emulate_ffn(a, defect), ref)}
  else:
    a, t = U.rowclass_lnproj(int(kind[-1]))
    outs = U.emulate_lnproj(a, defect)
    assert torch.equal(outs[0], t)                  # the prescribed rows are reached exactly
    errs = U.lnproj_row_errs(a, outs)
  bar = U.row_bar(kind)
  return max(U.figure(f"B2 {kind} {n} {defect or 'emulation'}" + (f" [{cls}]" if cls else ""), e[sel], bar)[0] for n, e in errs.items()), bar


def b3(pre, pattern, defect=None):
  worst = 0.0
  for p in range(4):
    a, ref, absval = U.sweep_case(pre, pattern, p)
    out = U.emulate_ffn(a, defect)
    assert bool((out == out[0]).all())
    worst = max(worst, U.check_sweep(f"B3 {'PRE ' if pre else ''}{pattern} sweep pass {p} {defect or 'emulation'}", out, ref, absval)[0])
  return worst


def b5_planes(planes, defect=None):
  a, ref = U.planes_case(planes)
  return U.figure(f"B5 {planes} planes {defect or 'emulation'}", U.row_err(U.emulate_ffn(a, defect), ref), U.row_bar("ffn"))[0]


def b5_wrap(defect=None):
  return U.check_wrap(f"B5 wrap {defect or 'emulation'}", U.emulate_ffn(U.wrap_case(), defect))


def b6(mode, B, HW, defect=None):
  a = U.geometry_case(mode, B, HW)
  return U.check_geometry(f"B6 lnproj mode {mode} B={B} HW={HW} {defect or 'emulation'}", a, U.emulate_lnproj(a, defect))


def test_emulation_meets_every_bar():
  for form in U.FORMS_LNPROJ:
    assert b1_lnproj(form) == (0.0, 0)
  assert b1_ffn_pre() == (0.0, 0)
  for kind in ("ffn", "ffn_pre", "lnproj0", "lnproj1"):
    worst, bar = b2(kind)
    print(f"[fused_l0 B2 {kind}] emulation's worst row {U.emu_worst(kind):.3e} -> bar {bar:.3e}")
    assert worst == U.emu_worst(kind) <= U.EMU_CEIL and worst < bar <= U.PROJECT_BAR
  for pre in (False, True):
    for pattern in ("gate", "value"):
      assert b3(pre, pattern) < 1.0
  for planes in (3, 5):
    assert b5_planes(planes) < U.row_bar("ffn")
  assert b5_wrap() == 0
  for mode in (0, 1):
    for B, HW in U.GEOMETRY:
      assert b6(mode, B, HW)[0] == []


# ------------------------------------------------------------------------------------------------ every defect misses the check named for it
EXACT = [("row_half_swapped", f) for f in U.FORMS_LNPROJ + ("ffn_pre",)] + [("kperm_identity", "ffn_pre"), ("residual_rows_shifted", "mode1"),
                                                                            ("residual_rows_shifted", "ffn_pre"), ("gn_table_of_sample0", "mode0_gn"),
                                                                            ("gn_scale_shift_swapped", "mode0_gn")]


@pytest.mark.parametrize("defect,form", EXACT, ids=lambda v: str(v))
def test_defect_misses_the_exact_check(defect, form):
  worst, rows = b1_ffn_pre(defect) if form == "ffn_pre" else b1_lnproj(form, defect)
  assert worst >= 1.0 and rows >= 1


ROWCLASS = ([("kperm_identity", k, None) for k in ("ffn", "ffn_pre", "lnproj0", "lnproj1")] +
            [("ln_own_half_only", k, None) for k in ("ffn_pre", "lnproj0", "lnproj1")] +
            [("eps_outside_sqrt", k, "tiny") for k in ("ffn", "ffn_pre", "lnproj0", "lnproj1")] + [("var_not_clamped", "ffn", "constant")])


@pytest.mark.parametrize("defect,kind,cls", ROWCLASS, ids=lambda v: str(v))
def test_defect_misses_the_row_class_check(defect, kind, cls):
  worst, bar = b2(kind, defect, cls)
  print(f"[fused_l0 B2 {kind} {defect}] worst row {worst:.3e} = {worst / bar:.1f} x the bar")
  assert worst >= MARGIN * bar
  if cls is not None:      # the other classes do not show it: why the figure is per row, and not one per tensor
    assert max(b2(kind, defect, c)[0] for c in ("mu0", "scale64")) < bar


SWEEP = [("kperm_identity", "gate"), ("kperm_identity", "value"), ("bias_value_gate_swapped", "gate"), ("bias_value_gate_swapped", "value"),
         ("chunk_bias_off_by_one", "gate"), ("chunk_bias_off_by_one", "value"), ("quick_gelu", "gate")]


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "PRE"])
@pytest.mark.parametrize("defect,pattern", SWEEP, ids=lambda v: str(v))
def test_defect_misses_the_hidden_unit_sweep(defect, pattern, pre):
  worst = b3(pre, pattern, defect)
  print(f"[fused_l0 B3 {defect} {pattern} sweep] worst |err| / bound {worst:.3g}")
  assert worst >= MARGIN


def test_defects_miss_the_planes_and_wrap_checks():
  for planes in (3, 5):
    worst = b5_planes(planes, "planes_first_only")
    print(f"[fused_l0 B5 planes_first_only, {planes} planes] {worst / U.row_bar('ffn'):.1f} x the bar")
    assert worst >= MARGIN * U.row_bar("ffn")
  assert b5_wrap("ln_rows_ignored") >= 1


@pytest.mark.parametrize("B,HW", U.GEOMETRY)
def test_defects_miss_the_geometry_checks(B, HW):
  for mode in (0, 1):
    bad, figs = b6(mode, B, HW, "q_unscaled")
    assert "q" in bad and figs["q"][0] >= MARGIN * figs["q"][1]
  bad, _ = b6(0, B, HW, "ones_row_missing")
  assert "V^T ones-row" in bad


def test_every_listed_defect_is_shown():
  shown = {d for d, _ in EXACT} | {d for d, _, _ in ROWCLASS} | {d for d, _ in SWEEP} | {"planes_first_only", "ln_rows_ignored", "q_unscaled", "ones_row_missing"}
  assert shown == set(U.DEFECTS)
