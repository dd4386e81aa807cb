"""The e4m3 KV cache on the CPU (tests/kv8_util.py): the row quantiser's rule and edge rows, the reference, and that the bars the GPU tests use
tell an honest run from a broken one.

  operator level  the fp32 emulation of the two kernels' arithmetic (P rounded to bf16 for the extend kernel, not for the decode kernel) meets
                  kv_cache_util.ATTN_BAR against fp64 on the dequantised operands, and every defect of kv8_util.DEFECTS misses it by 3 x or more.
                  `own_token_unquantised` is measured on kv8_util.tie_operands: on the peaked random operands the e4m3 rounding of one row moves
                  the output by 2.6 .. 4.7 of the bar (printed), not 3 x at every shape, so the inputs were changed, not the bar; test_attention_kv8_gpu.py runs those
                  inputs through both kernels.
  engine level    the bf16-storage emulation of the OPT engine stays within the hidden-state bar of tests/golden/kv8_tolerance.json (4 x its own
                  worst distance from the fp64 run, tools/kv8_tolerance.py: 1.1e-1, because it has to admit e4m3 code flips between two honest
                  runs), and the defects that break the engine's plumbing whatever the operands are (ENGINE_DEFECTS: the scale dropped, the
                  exponent read as unsigned, a stale exponent visible) miss that bar by 3 x or more (measured: 11.8 x and up).  The other three
                  CANNOT be separated by this bar on this rig and are not asserted at this level; their factors are printed (measured, worst
                  row of the batch: scale_of_neighbour 2.0 x, v_scale_on_k 1.5 x, own_token_unquantised 0.24 x).  The rig's model is given, and in
                  it the exponents of neighbouring tokens, and of a token's key and value, differ by at most one in a fraction of the rows, and a
                  token's own unquantised row is a perturbation of the kind and size of a code flip.  The inputs that separate them are the
                  operator level's (exponents that differ from slot to slot; the tie), where all six are asserted; the bar stays as measured.
  prompts         the reference's own greedy decisions on the engine test's prompts (the batch on bf16 and fp8 weights, the session plan) have
                  no top-2 margin under the near-tie bar m_logit: the reference alone needs no excusal."""
import pytest
import torch

import dialogue_session_util as S
import kv8_util as K
import kv_cache_util as U
from gill_amd import synth

ENGINE_DEFECTS = ("scale_dropped", "exponent_unsigned", "stale_exponent_visible")
OP_CASES = ((4, 64, 5, 40), (2, 128, 33, 97), (3, 80, 1, 66), (2, 64, 64, 64))      # (H, d, nq, nkv)


def test_quantiser_rule_on_the_edge_rows():
  g = torch.Generator().manual_seed(3)
  for d in (64, 80, 128):
    for kind in K.EDGE_ROWS:
      x = K.edge_row(kind, d, g)
      assert torch.equal(U.bf(x), x), kind
      q, e = K.quantise_rows(x[None])
      code, e = q[0].float(), int(e[0])
      deq = K.dequantise_rows(q, torch.tensor([e]))[0]
      assert torch.equal(U.bf(deq), deq), f"{kind}: a code times 2^e is not a bf16 number"
      if kind == "zero":
        assert e == 0 and bool((code == 0).all())
        continue
      assert 224 <= code.abs().max().item() <= 448, (kind, code.abs().max().item())
      assert e == {"exact_448": -8, "one_step_above": -7, "subnormal_rest": -8}.get(kind, e), (kind, e)
      rest = code.abs().sort().values[:-1]
      if kind == "exact_448":
        assert code.abs().max().item() == 448
      if kind == "subnormal_rest":
        assert bool((rest < 2.0 ** -6).all()) and bool((rest > 0).any()) and not torch.equal(deq, x), "the rest should round among the subnormal codes"
      if kind == "one_element_2e20":
        assert bool((rest == 0).all())


def test_reference_is_plain_attention_on_the_dequantised_operands():
  H, d, nq, nkv = 4, 64, 5, 40
  q, k, v = K.attn_operands(H, nq, nkv, d, seed=3)
  K.plant_edge_rows(k, v, H, d, nkv - nq, seed=9)
  kq, ke = K.quantise_heads(k, H, d)
  vq, ve = K.quantise_heads(v, H, d)
  assert len(set(ke[0].tolist())) > 1 and bool((ke != ve).any()), "neighbouring slots, and a slot's key and value, should differ in exponent"
  kd, vd = K.dequantise_rows(kq, ke, torch.float64), K.dequantise_rows(vq, ve, torch.float64)
  s = (q.view(nq, H, d).transpose(0, 1).double() * d ** -0.5) @ kd.transpose(1, 2)
  vis = torch.arange(nkv)[None, :] <= (torch.arange(nq)[:, None] + nkv - nq)
  plain = (s.masked_fill(~vis, float("-inf")).softmax(-1) @ vd).transpose(0, 1).reshape(nq, H * d)
  assert (plain - K.attention_ref(q, kq, ke, vq, ve, H, d)).abs().max().item() < 1e-6


def _op_figures(q, k, v, H, d, defect, stale):
  nq, nkv = q.shape[0], k.shape[0]
  kq, ke = K.quantise_heads(k, H, d)
  vq, ve = K.quantise_heads(v, H, d)
  ref = K.attention_ref(q, kq, ke, vq, ve, H, d)
  heads = lambda t: t.view(-1, H, d).transpose(0, 1)   # noqa: E731
  out = []
  for n_ext in (nq, 0):      # the extend kernel's arithmetic, the decode kernel's
    o = K.attend(heads(q) * d ** -0.5, kq.float(), ke, vq.float(), ve, defect=defect, rnd_p=U.bf, n_ext=n_ext, k_raw=heads(k), v_raw=heads(v),
                 stale_e=stale)
    out.append(U.report_rows(f"kv8 host H{H} d{d} nq{nq} nkv{nkv} {defect or 'honest'} {'extend' if n_ext else 'decode'}",
                             o.transpose(0, 1).reshape(nq, H * d)[None], ref[None]))
  return out


def test_operator_emulation_meets_the_bar_and_every_defect_misses_it():
  worst = 0.0
  factors = {df: float("inf") for df in K.DEFECTS}
  for ci, (H, d, nq, nkv) in enumerate(OP_CASES):
    q, k, v = K.attn_operands(H, nq, nkv, d, seed=40 + ci)
    K.plant_edge_rows(k, v, H, d, nkv - nq, seed=50 + ci)
    worst = max(worst, *_op_figures(q, k, v, H, d, None, 0))
    for df in K.DEFECTS:
      if df == "own_token_unquantised":
        print(f"[kv8 host] own_token_unquantised on the peaked operands: {max(_op_figures(q, k, v, H, d, df, 0)) / U.ATTN_BAR:.2f} of the bar")
        qt, kt, vt = K.tie_operands(H, d, seed=60 + ci)
        worst = max(worst, *_op_figures(qt, kt, vt, H, d, None, 0))
        f = min(_op_figures(qt, kt, vt, H, d, df, 0))
      else:
        f = min(_op_figures(q, k, v, H, d, df, 127 if ci % 2 else -127))
      factors[df] = min(factors[df], f / U.ATTN_BAR)
  print(f"[kv8 host] operator level: honest emulation {worst / U.ATTN_BAR:.3f} of ATTN_BAR; defects miss it by " +
        ", ".join(f"{df} {x:.1f}x" for df, x in factors.items()))
  assert worst < U.ATTN_BAR
  for df, x in factors.items():
    assert x >= 3.0, (df, x)


def test_engine_emulation_meets_the_hidden_bar_and_defects_miss_it():
  gold = K.golden()
  bar = gold["hid_bar"]
  b = len(K.LENGTHS) - 1                 # the shortest row of the batch: 9 prompt tokens and the reference's own 6
  ref = K.batch_reference("bf16", tuple(gold["seeds"]))[b]
  cfg, sd = K.model("bf16")
  n0 = K.LENGTHS[b]
  x = torch.nn.functional.embedding(torch.tensor(ref["ids"])[None], sd["model.decoder.embed_tokens.weight"].float())
  want = ref["hidden"][n0 - 1:]
  honest = K.row_rel(K.kv8_forward(sd, cfg, x, rnd=U.bf, n_ext=n0)[0, n0 - 1:], want)
  print(f"[kv8 host] engine level: honest emulation {honest:.3e} = {honest / bar:.3f} of hid_bar {bar:.3e}")
  assert honest < bar
  for df in K.DEFECTS:
    f = K.row_rel(K.kv8_forward(sd, cfg, x, defect=df)[0, n0 - 1:], want) / bar
    print(f"[kv8 host] engine level: {df} misses hid_bar by {f:.2f}x")
    if df in ENGINE_DEFECTS:      # module docstring: the others are separated at the operator level
      assert f >= 3.0, (df, f)


def test_the_reference_alone_has_no_decision_inside_the_near_tie_bar():
  gold = K.golden()
  m = gold["m_logit"]
  assert gold["hid_bar"] == pytest.approx(K.MARGIN * gold["largest_hidden_distance"]) and m == pytest.approx(K.MARGIN * gold["largest_logit_distance"])
  small = float("inf")
  for w in ("bf16", "fp8"):
    for r in K.batch_reference(w, tuple(gold["seeds"])):
      small = min(small, min(r["margins"]))
  cfg, sd = K.model("bf16")
  seeds = {tuple(int(v) for v in k.split(",")): int(s) for k, s in gold["session_seeds"].items()}
  margins = []

  def decode(turn, row, hist):
    r = K.greedy_ref(sd, cfg, hist, n_dec=3, emulate=False)
    margins.extend(r["margins"])
    return r["tokens"] + synth.IMG_TOKEN_IDS * 2

  S.walk(S.PLANS[gold["plan"]], seeds, decode)
  print(f"[kv8 host] smallest top-2 margin of the reference: batch {small:.3f}, session {min(margins):.3f} ({len(margins)} decisions); m_logit {m:.3f}")
  assert small >= m and min(margins) >= m
