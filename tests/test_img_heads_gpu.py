"""gill_op_img_block_heads and gill_op_img_rerank_scores on the MI355X against fp64 on the same operands (tests/img_heads_util.py), within
the bars tools/img_heads_tolerance.py recorded (10 x the distance of an fp32 accumulation in another K order from fp64, measured on the CPU at
these shapes).  tests/test_img_heads_host.py asserts that no decision of these inputs is a near tie, so choice is compared exactly."""
import numpy as np
import pytest
import torch

import img_heads_util as H
from gill_amd import _native as N
from gill_amd import ops

pytestmark = pytest.mark.gpu
CANARY = -77.0


def _dev(inp, cuda):
  t = {k: torch.from_numpy(v).to(cuda) for k, v in inp.items()}
  return t["hidden"], t["row_idx"], (t["Wr"].bfloat16(), t["br"]), (t["Wd"].bfloat16(), t["bd"])


def _close(got, want, bar, what):
  d = float(np.abs(got.double().cpu().numpy() - want).max())
  print(f"[img_heads] {what}: largest distance {d:.3e} (bar {bar:.3e})")
  assert np.isfinite(got.cpu().numpy()).all() and d <= bar, (what, d, bar)


@pytest.mark.parametrize("ci", range(len(H.OP_CASES)))
def test_heads_against_fp64(cuda, ci):
  """Retrieval only, decision only and both, per shape; a head's outputs do not depend on whether the other head runs."""
  D, E, C, n = H.OP_CASES[ci]
  bars = H.load_bars()
  inp = H.op_inputs(D, E, C, n, H.case_seed(ci))
  emb, probs, choice, _ = H.heads_ref(inp)
  hidden, row_idx, ret, dec = _dev(inp, cuda)
  e3, p3, c3 = ops.img_block_heads(hidden, row_idx, ret=ret, decision=dec)
  assert e3.shape == (n, E) and e3.dtype == torch.float32 and p3.shape == (n, C) and c3.shape == (n,) and c3.dtype == torch.int32
  _close(e3, emb, bars["ret_emb"], f"case {ci} ret_emb")
  _close(p3, probs, bars["probs"], f"case {ci} probs")
  assert c3.cpu().tolist() == choice.tolist()
  e1, p1, c1 = ops.img_block_heads(hidden, row_idx, ret=ret)
  assert p1 is None and c1 is None and torch.equal(e1, e3)
  e2, p2, c2 = ops.img_block_heads(hidden, row_idx, decision=dec)
  assert e2 is None and torch.equal(p2, p3) and torch.equal(c2, c3)
  if n >= 3:      # the repeated row
    assert torch.equal(e3[-1], e3[0]) and torch.equal(p3[-1], p3[0])


def test_zero_row_clamped_indices_and_canaries(cuda):
  """An all-zero hidden row with a zero bias gives a zero ret_emb (no NaN); row_idx -5 and rows + 3 give the results of rows 0 and rows - 1;
  the rows around every output keep their canary."""
  D, E, C, n = H.OP_CASES[1]
  bars = H.load_bars()
  inp = H.op_inputs(D, E, C, 4, 77)
  rows = inp["hidden"].shape[0]
  inp["hidden"][5] = 0
  inp["br"][:] = 0
  inp["row_idx"][:] = (5, -5, rows + 3, 2)
  emb, probs, choice, _ = H.heads_ref(inp)
  hidden, row_idx, ret, dec = _dev(inp, cuda)
  eb = torch.full((6, E), CANARY, device=cuda)
  pb = torch.full((6, C), CANARY, device=cuda)
  cb = torch.full((6,), int(CANARY), device=cuda, dtype=torch.int32)
  ops.img_block_heads(hidden, row_idx, ret=ret, decision=dec, _out=(eb[1:5], pb[1:5], cb[1:5]))
  assert (eb[0] == CANARY).all() and (eb[5] == CANARY).all() and (pb[0] == CANARY).all() and (pb[5] == CANARY).all()
  assert cb[0] == int(CANARY) and cb[5] == int(CANARY)
  assert (eb[1] == 0).all()
  _close(eb[1:5], emb, bars["ret_emb"], "zero / clamped ret_emb")
  _close(pb[1:5], probs, bars["probs"], "zero / clamped probs")
  assert cb[1:5].cpu().tolist() == choice.tolist()
  # the clamped entries are the results of the rows they were clamped to, bit for bit
  idx = torch.tensor([0, rows - 1], dtype=torch.int32, device=cuda)
  e2, p2, c2 = ops.img_block_heads(hidden, idx, ret=ret, decision=dec)
  assert torch.equal(e2, eb[2:4]) and torch.equal(p2, pb[2:4]) and torch.equal(c2, cb[2:4])


def test_a_block_has_the_same_bits_at_any_n_and_position(cuda):
  D, E, C, n = H.OP_CASES[2]
  inp = H.op_inputs(D, E, C, n, H.case_seed(2))
  hidden, row_idx, ret, dec = _dev(inp, cuda)
  e, p, c = ops.img_block_heads(hidden, row_idx, ret=ret, decision=dec)
  again = ops.img_block_heads(hidden, row_idx, ret=ret, decision=dec)
  assert all(torch.equal(a, b) for a, b in zip((e, p, c), again))
  er, pr, cr = ops.img_block_heads(hidden, row_idx.flip(0).contiguous(), ret=ret, decision=dec)
  assert torch.equal(er.flip(0), e) and torch.equal(pr.flip(0), p) and torch.equal(cr.flip(0), c)
  for k in range(n):
    e1, p1, c1 = ops.img_block_heads(hidden, row_idx[k:k + 1].contiguous(), ret=ret, decision=dec)
    assert torch.equal(e1[0], e[k]) and torch.equal(p1[0], p[k]) and torch.equal(c1[0], c[k]), k


def test_argument_errors_launch_nothing(cuda):
  hidden = torch.zeros((4, 770), device=cuda)
  idx = torch.zeros((2,), dtype=torch.int32, device=cuda)
  out = (torch.full((2, 8), CANARY, device=cuda), torch.full((2, 5), CANARY, device=cuda), torch.full((2,), 7, device=cuda, dtype=torch.int32))

  def untouched():
    torch.cuda.synchronize()
    return bool((out[0] == CANARY).all() and (out[1] == CANARY).all() and (out[2] == 7).all())
  w = lambda r, d: torch.zeros((r, d), device=cuda, dtype=torch.bfloat16)     # noqa: E731
  b = lambda r: torch.zeros((r,), device=cuda)                                  # noqa: E731
  with pytest.raises(N.GillNativeError, match="multiple of 8"):
    ops.img_block_heads(hidden, idx, ret=(w(8, 770), b(8)), decision=(w(2, 770), b(2)), _out=out)
  assert untouched()
  hidden = torch.zeros((4, 768), device=cuda)
  with pytest.raises(N.GillNativeError, match="C <= 4"):
    ops.img_block_heads(hidden, idx, ret=(w(8, 768), b(8)), decision=(w(5, 768), b(5)), _out=out)
  assert untouched()
  with pytest.raises(N.GillNativeError, match="NULL"):
    ops.img_block_heads(hidden, idx, _out=out)
  assert untouched()
  with pytest.raises(N.GillNativeError, match="aligned"):
    ops.img_block_heads(torch.zeros((4 * 768 + 1,), device=cuda)[1:].view(4, 768), idx, ret=(w(8, 768), b(8)), _out=out)
  assert untouched()


@pytest.mark.parametrize("ci", range(len(H.RERANK_CASES)))
def test_rerank_scores_against_fp64(cuda, ci):
  n, g, E = H.RERANK_CASES[ci]
  bar = H.load_bars()["rerank"]
  visual, ret_emb = H.rerank_inputs(n, g, E, H.case_seed(ci))
  want = H.rerank_ref(visual, ret_emb)
  v, r = torch.from_numpy(visual).to(cuda), torch.from_numpy(ret_emb).to(cuda)
  buf = torch.full((n + 2, g), CANARY, device=cuda)
  got = ops.img_rerank_scores(v, r, _out=buf[1:n + 1])
  assert (buf[0] == CANARY).all() and (buf[n + 1] == CANARY).all()
  _close(got, want, bar, f"rerank case {ci}")
  # a block's scores do not depend on the other blocks
  for k in range(n):
    one = ops.img_rerank_scores(v[k * g:(k + 1) * g].contiguous(), r[k:k + 1].contiguous())
    assert torch.equal(one[0], got[k]), k


def test_rerank_zero_rows_score_zero(cuda):
  """A zero visual row, and every image of a block whose ret_emb is zero, score exactly 0 (no NaN); the other scores are those of the
  untouched inputs, bit for bit."""
  n, g, E = H.RERANK_CASES[1]
  visual, ret_emb = H.rerank_inputs(n, g, E, 91)
  base = ops.img_rerank_scores(torch.from_numpy(visual).to(cuda), torch.from_numpy(ret_emb).to(cuda))
  visual[1] = 0             # block 0, image 1
  ret_emb[2] = 0            # block 2
  want = H.rerank_ref(visual, ret_emb)
  got = ops.img_rerank_scores(torch.from_numpy(visual).to(cuda), torch.from_numpy(ret_emb).to(cuda))
  _close(got, want, H.load_bars()["rerank"], "rerank with zero rows")
  assert got[0, 1] == 0 and (got[2] == 0).all() and want[0, 1] == 0 and not want[2].any()
  assert torch.equal(got[0, 0], base[0, 0]) and torch.equal(got[1], base[1])
