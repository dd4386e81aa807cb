"""The fused level-0 kernels (csrc/ffn.hip, csrc/lnproj.hip) on the operands of fused_l0_util: what test_fused_l0_host.py shows on the
emulation, here on the device.

  B1  integer operands: the residual stream / the PRE kernel's output equal the integer result exactly;
  B2  LayerNorm row classes (mean 0 / 4 / 16, variance ~ eps, scale 64, outlier channel, constant row; on the planes-fed kernel the constant
      rows' variance comes out negative: the clamp) against fp64, per row, at fused_l0_util.row_bar;
  B3  every hidden unit alone on an output column: value * gelu(gate) within 2^-8 |ref| + 4e-5 |value| of fp64 erf-GELU;
  B4  264 tiles (one round of the 256 CUs and a tail) of three base tiles with rotated rows: every row's bits equal the 3-tile run's;
  B5  3 and 5 unequal planes against fp64 at the B2 bar; half as many plane rows as rows (the wrap), NaN behind the planes;
  B6  lnproj at (B, HW) = (4, 32) and (8, 160).

Measured worst rows: profiles/fused_l0_operator_tests.md."""
import pytest
import torch

import fused_l0_util as U

pytestmark = pytest.mark.gpu


BF16_OPERANDS = ("t", "w1", "w2", "wp", "resid", "o2", "wo", "x", "t0")      # the wrappers take these as bf16; every builder makes them bf16-valued


def on_device(a, dev):
  """the operands of a builder on the device, the bf16 ones converted (losslessly: asserted)"""
  out = {}
  for k, v in a.items():
    if torch.is_tensor(v) and k in BF16_OPERANDS:
      assert U.is_bf16(v), k
      v = U.bf(v)
    out[k] = v.to(dev) if torch.is_tensor(v) else v
  return out


def run_ffn(a, dev, **kw):
  from gill_amd import ops
  a = on_device(a, dev)
  if a.get("ln_stats") is not None:
    kw.update(ln_stats=a["ln_stats"], ln_rows=a.get("ln_rows", 0))
  return ops.ffn_fused(a["t"], a["ln_g"], a["ln_b"], a["w1"], a["b1"], a["w2"], a["b2"], a["wp"], a["bp"], a["resid"], o2=a.get("o2"), wo=a.get("wo"),
                       bo2=a.get("bo2"), **kw)


def run_lnproj(a, dev):
  from gill_amd import ops
  a = on_device(a, dev)
  return ops.lnproj(a["mode"], a["x"], a.get("t0"), a["w1"], a["b1"], a["ln_g"], a["ln_b"], a["w2"], a["B"], a["HW"], gn_ss=a.get("gn_ss"))


def written(outs, HW):
  """the NaN pre-fill of the wrapper shows unwritten elements: all of t, q, k, and rows 0 .. 48 of V^T (rows 49 .. 63 are never written)"""
  t, q, k, vt = outs
  ok = bool(torch.isfinite(t.float()).all()) and bool(torch.isfinite(q.float()).all())
  if k is not None:
    ok = ok and bool(torch.isfinite(k.float()).all()) and bool(torch.isfinite(vt[:, :, :U.DP + 1].float()).all())
  return ok


# ------------------------------------------------------------------------------------------------ B1
@pytest.mark.parametrize("form", U.FORMS_LNPROJ)
def test_exact_first_stage_lnproj(cuda, form):
  a, want = U.exact_lnproj(form)
  outs = run_lnproj(a, cuda)
  worst, rows = U.exact_diff(f"B1 lnproj {form}", outs[0], want)
  assert written(outs, a["HW"])
  assert worst == 0.0 and rows == 0


def test_exact_first_stage_and_proj_out_ffn_pre(cuda):
  a, want = U.exact_ffn_pre()
  worst, rows = U.exact_diff("B1 ffn PRE", run_ffn(a, cuda), want)
  assert worst == 0.0 and rows == 0


# ------------------------------------------------------------------------------------------------ B2
@pytest.mark.parametrize("pre", [False, True], ids=["planes-fed", "PRE"])
def test_layernorm_row_classes_ffn(cuda, pre):
  a, ref = U.rowclass_ffn(pre)
  kind = "ffn_pre" if pre else "ffn"
  out = run_ffn(a, cuda)
  err = U.row_err(out, ref)
  for i, cls in enumerate(U.ROW_CLASSES):
    print(f"[fused_l0 B2 {kind} {cls}] worst row {float(err[i::U.NCLS].max()):.3e}")
  worst, over = U.figure(f"B2 {kind} (emulation: {U.emu_worst(kind):.3e})", err, U.row_bar(kind))
  assert bool(torch.isfinite(out.float()).all())
  assert over == 0 and worst < U.row_bar(kind)


@pytest.mark.parametrize("mode", [0, 1])
def test_layernorm_row_classes_lnproj(cuda, mode):
  a, t = U.rowclass_lnproj(mode)
  kind = f"lnproj{mode}"
  outs = run_lnproj(a, cuda)
  assert written(outs, a["HW"])
  assert torch.equal(outs[0].float().cpu(), t)                 # the prescribed rows are reached exactly
  for n, err in U.lnproj_row_errs(a, outs).items():
    for i, cls in enumerate(U.ROW_CLASSES):
      print(f"[fused_l0 B2 {kind} {n} {cls}] worst row {float(err[i::U.NCLS].max()):.3e}")
    worst, over = U.figure(f"B2 {kind} {n} (emulation: {U.emu_worst(kind):.3e})", err, U.row_bar(kind))
    assert over == 0 and worst < U.row_bar(kind)


# ------------------------------------------------------------------------------------------------ B3
@pytest.mark.parametrize("pattern", ["gate", "value"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "PRE"])
def test_hidden_unit_sweep(cuda, pre, pattern):
  worst_all, over_all = 0.0, 0
  for p in range(4):
    a, ref, absval = U.sweep_case(pre, pattern, p)
    out = run_ffn(a, cuda).float().cpu()
    assert bool(torch.isfinite(out).all())
    worst, over = U.check_sweep(f"B3 {'PRE ' if pre else ''}{pattern} sweep pass {p}", out, ref, absval)
    worst_all, over_all = max(worst_all, worst), over_all + over
  assert over_all == 0 and worst_all <= 1.0


# ------------------------------------------------------------------------------------------------ B4
def same_rows(name, big, base, src):
  """bit equality of every row of the big run with the base run's row it holds; both (rows, n) bf16 on the device.  (NaN pre-fill in rows
  the kernel never writes compares equal as bits.)"""
  want = base[src]
  diff = int((big.view(torch.int16) != want.view(torch.int16)).any(1).sum())
  print(f"[fused_l0 B4 {name}] {diff} of {big.shape[0]} rows differ from the 3-tile run")
  return diff == 0 and torch.equal(big.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "PRE"])
def test_position_independence_ffn(cuda, pre):
  from gill_amd import ops
  a = on_device(U.position_ffn(pre), cuda)
  src = U.big_index().to(cuda)
  rows = lambda x: x[src].contiguous()
  call = lambda t, resid, o2: ops.ffn_fused(t, a["ln_g"], a["ln_b"], a["w1"], a["b1"], a["w2"], a["b2"], a["wp"], a["bp"], resid, o2=o2, wo=a.get("wo"),
                                            bo2=a.get("bo2"))
  base = call(a["t"], a["resid"], a.get("o2"))
  big = call(rows(a["t"]), rows(a["resid"]), rows(a["o2"]) if pre else None)
  assert bool(torch.isfinite(base.float()).all()) and bool(torch.isfinite(big.float()).all())
  assert same_rows(f"ffn {'PRE ' if pre else ''}out", big, base, src)


@pytest.mark.parametrize("form", U.FORMS_LNPROJ)
def test_position_independence_lnproj(cuda, form):
  from gill_amd import ops
  a = on_device(U.position_lnproj(form), cuda)
  src = U.big_index().to(cuda)
  rows = lambda x: None if x is None else x[src].contiguous()
  call = lambda x, t0, B, ss: ops.lnproj(a["mode"], x, t0, a["w1"], a["b1"], a["ln_g"], a["ln_b"], a["w2"], B, 128, gn_ss=ss)
  ss = a.get("gn_ss")
  base = call(a["x"], a.get("t0"), 3, ss)
  big = call(rows(a["x"]), rows(a.get("t0")), U.BIG_TILES, None if ss is None else ss[torch.arange(U.BIG_TILES, device=cuda) % 3].contiguous())
  assert written(base, 128) and written(big, 128)
  tok = lambda q: q.permute(0, 2, 1, 3).reshape(-1, q.shape[1] * q.shape[3])            # (B, 8, 128, 48) -> (B * 128, 384): one row per token
  tokv = lambda vt: vt.permute(0, 3, 1, 2).reshape(-1, vt.shape[1] * vt.shape[2])       # (B, 8, 64, 128) -> (B * 128, 512)
  ok = same_rows(f"lnproj {form} t", big[0], base[0], src)
  ok = same_rows(f"lnproj {form} q", tok(big[1]), tok(base[1]), src) and ok
  if a["mode"] == 0:
    ok = same_rows(f"lnproj {form} k", tok(big[2]), tok(base[2]), src) and ok
    ok = same_rows(f"lnproj {form} v^T", tokv(big[3]), tokv(base[3]), src) and ok
  assert ok


# ------------------------------------------------------------------------------------------------ B5
@pytest.mark.parametrize("planes", [3, 5])
def test_unequal_planes(cuda, planes):
  a, ref = U.planes_case(planes)
  out = run_ffn(a, cuda)
  one = run_ffn({k: v for k, v in a.items() if k not in ("ln_stats", "ln_planes", "ln_rows")}, cuda)
  print(f"[fused_l0 B5 {planes} planes] {int((out != one).any(1).sum())} of {out.shape[0]} rows differ in bits from the one-plane run")
  worst, over = U.figure(f"B5 {planes} planes", U.row_err(out, ref), U.row_bar("ffn"))
  worst1, over1 = U.figure("B5 one plane (the entry's own row sums)", U.row_err(one, ref), U.row_bar("ffn"))
  assert bool(torch.isfinite(out.float()).all())
  assert over == 0 and worst < U.row_bar("ffn") and over1 == 0


def test_planes_wrap_and_poison(cuda):
  from gill_amd import ops
  a = U.wrap_case()
  M, planes = a["t"].shape[0], a["ln_planes"]
  flat = a["ln_stats"].to(cuda)                                        # the planes proper, NaN behind them
  view = flat[:planes * (M // 2) * 2].view(planes, M // 2, 2)
  assert bool(torch.isnan(flat[view.numel():]).all()) and view.data_ptr() == flat.data_ptr()
  d = on_device(a, cuda)
  out = ops.ffn_fused(d["t"], d["ln_g"], d["ln_b"], d["w1"], d["b1"], d["w2"], d["b2"], d["wp"], d["bp"], d["resid"], ln_stats=view, ln_rows=M // 2)
  assert bool(torch.isfinite(out.float()).all())                      # (nothing behind the planes was read)
  assert U.check_wrap("B5 wrap", out) == 0
  ref = U.rowclass_ffn(False, M // 2)[1]
  worst, over = U.figure("B5 wrap, first half against fp64", U.row_err(out[:M // 2], ref), U.row_bar("ffn"))
  assert over == 0


def test_ex_entries_report_errors(cuda):
  """what the launchers require is an error message, not a fault: a GroupNorm table in mode 1 or with HW % 128 != 0; planes with o2; a wrap
  that would read behind the planes"""
  from gill_amd import _native as N
  a = dict(U.geometry_case(0, 4, 32))
  a["gn_ss"] = U.gn_table(4, 900)
  with pytest.raises(N.GillNativeError):
    run_lnproj(a, cuda)
  b = dict(U.exact_lnproj("mode1")[0])
  b["gn_ss"] = U.gn_table(3, 901)
  with pytest.raises(N.GillNativeError):
    run_lnproj(b, cuda)
  c = dict(U.exact_ffn_pre()[0])
  M = c["t"].shape[0]
  with pytest.raises(N.GillNativeError):
    run_ffn(c, cuda, ln_stats=torch.zeros(1, M, 2, device=cuda))
  e = {k: v for k, v in U.rowclass_ffn(False)[0].items() if k not in ("ln_stats", "ln_planes", "ln_rows")}
  with pytest.raises(N.GillNativeError):
    run_ffn(e, cuda, ln_stats=torch.zeros(1, M // 2 - 1, 2, device=cuda), ln_rows=M // 2 - 1)


# ------------------------------------------------------------------------------------------------ B6
@pytest.mark.parametrize("B,HW", U.GEOMETRY)
@pytest.mark.parametrize("mode", [0, 1])
def test_geometry_lnproj(cuda, mode, B, HW):
  a = U.geometry_case(mode, B, HW)
  outs = run_lnproj(a, cuda)
  assert tuple(outs[1].shape) == (B, U.NH, HW, U.DP)                  # hw_pad == HW: no token slot beyond HW exists to be written
  assert written(outs, HW)
  bad, _ = U.check_geometry(f"B6 lnproj mode {mode} B={B} HW={HW}", a, outs)
  assert bad == []
