"""gill_opt_score_candidates (packed candidate continuations scored against the rows' cached prefixes, nothing appended) on the MI355X, on the
OPT-125m synthetic rig (ragged_decode_util.gill125_rig).

Four cache rows hold the histories of candidate_rank_util (70, 33, 1 and 31 tokens), put there by gill_opt_extend through a dialogue session; ten
candidates per row with counts (1, 2, 7, 8, 9, 16, 31, 32, 33, 40) go through ONE call (716 packed rows; the row with a one-token history has
plen = 0).  Checked:

  oracle          token log-probabilities and candidate means against oracle.opt_ref on every history + candidate alone, within the bars of
                  tools/candidate_rank_tolerance.py (tests/golden/candidate_rank_tolerance.json: 4 x the bf16 emulation's distances);
  cross-path      agreement with lm_forward_loss / gill_opt_forward_loss on the concatenation at the candidate's positions within twice the
                  token bar (two GPU paths, each within one bar of the oracle);
  bits            the same call twice gives equal bits (bit-independence across pack sizes is the operator's property: the bf16 GEMM's split
                  depends on M; test_attention_fork_gpu.py);
  cache untouched a decode step of every row after a scoring call gives the hidden rows, bit for bit, of the same session replayed without
                  the scoring call; gill_opt_kv_bytes is unchanged;
  empty candidate n_scored = 0 and a NaN mean;
  refusals        an e4m3-cache handle (the error names the format), a handle without a cache, len_bound beyond the position table;
  w8 handle       a GILL_OPT_W8 handle meets the same bars against the oracle on w8_util.w8_state_dict weights."""
import math

import pytest
import torch

import candidate_rank_util as CU
import ragged_decode_util as R
from gill_amd.dialogue import pack_candidates

pytestmark = pytest.mark.gpu

CAPACITY = 128


@pytest.fixture(scope="module")
def gill125(cuda):
  return R.gill125_rig(cuda)


@pytest.fixture(scope="module")
def tol():
  return CU.load_tolerance()


def _session(m):
  s = m.open_session(len(CU.HISTORIES), CAPACITY)
  s.extend(list(range(len(CU.HISTORIES))), ids=[CU.history_ids(i) for i in range(len(CU.HISTORIES))])
  return s


def _pack(s, candidates=None):
  candidates = CU.all_candidates() if candidates is None else candidates
  packs = pack_candidates([(r, s.books[r].ids, s.books[r].cached, 0) for r in range(s.B)], candidates)
  assert len(packs) == 1
  return packs[0]


def _score(m, p, cuda, **kw):
  out = m._lm_score_candidates(p, **kw)
  torch.cuda.synchronize()
  return out


def _split(p, out):
  """-> per candidate (token log-probabilities of its own tokens, sum, mean, n_scored), host."""
  o = out.cpu()
  T, C = p.total_new, p.n_candidates
  n_scored = o[T + 2 * C:].view(torch.int32)
  return [(o[first:first + n], float(o[T + c]), float(o[T + C + c]), int(n_scored[c])) for c, (_, _, first, n) in enumerate(p.own)]


def _check_against(tag, p, got, oracle, tol):
  worst_t = worst_m = 0.0
  for c, (k, j, _, n) in enumerate(p.own):
    tok, s_sum, s_mean, n_sc = got[c]
    want = oracle[k][j]
    assert n_sc == n == want.numel(), (tag, k, j, n_sc, n)
    assert torch.isfinite(tok).all() and math.isfinite(s_mean)
    d_t = float((tok - want).abs().max())
    d_m = abs(s_mean - float(want.mean()))
    worst_t, worst_m = max(worst_t, d_t), max(worst_m, d_m)
    assert abs(s_sum - s_mean * n) <= 1e-4 * max(1.0, abs(s_sum)), (tag, k, j, s_sum, s_mean, n)
    assert d_t < tol["token_bar"] and d_m < tol["mean_bar"], (tag, k, j, d_t, d_m)
  print(f"[{tag}] worst token log-prob distance {worst_t:.3e} (bar {tol['token_bar']:.3e}), worst candidate-mean distance {worst_m:.3e} "
        f"(bar {tol['mean_bar']:.3e})")


def test_one_call_meets_the_oracle_twice_with_equal_bits_and_agrees_with_forward_loss(cuda, gill125, tol):
  from gill_amd import _native as N
  m = gill125.model
  s = _session(m)
  p = _pack(s)
  assert p.total_new == len(CU.HISTORIES) * sum(CU.COUNTS) and p.plen == [n - 1 for n in CU.HISTORIES for _ in CU.COUNTS]
  kv_bytes = N.lib().gill_opt_kv_bytes(s.handle)
  flags = torch.zeros(p.n_candidates, dtype=torch.int32, device=cuda)
  rank = torch.full((p.total_new,), -7, dtype=torch.int32, device=cuda)
  hidden = torch.zeros((p.total_new, m.opt_cfg.hidden_size), dtype=torch.float32, device=cuda)
  out = _score(m, p, cuda, token_rank=rank, hidden_all=hidden, flags=flags)
  assert not bool(flags.any()), "a candidate was clamped or emptied"
  assert N.lib().gill_opt_kv_bytes(s.handle) == kv_bytes and s.epoch == m._cache_epoch
  tg = torch.tensor(p.targets)
  assert bool((rank.cpu()[tg == -100] == -1).all()) and bool((rank.cpu()[tg != -100] >= 0).all())
  assert torch.isfinite(hidden).all() and float(hidden.abs().max()) > 0
  got = _split(p, out)
  _check_against("score_candidates", p, got, CU.oracle_all(), tol)
  again = _score(m, p, cuda)
  assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "the same call twice gives different bits"
  # the other GPU path: the whole concatenation through gill_opt_forward_loss, one sequence per call
  worst = 0.0
  for c, (k, j, _, n) in enumerate(p.own):
    hist, cand = CU.history_ids(k), CU.all_candidates()[k][j]
    ids = torch.tensor([hist + cand])
    labels = torch.tensor([[-100] * len(hist) + cand])
    fl = m.lm_forward_loss(ids, labels)
    want = -fl.token_loss[0, len(hist) - 1:].cpu()
    d = float((got[c][0] - want).abs().max())
    worst = max(worst, d)
    assert d < 2 * tol["token_bar"], (k, j, d)
  print(f"[score_candidates vs forward_loss] worst token distance {worst:.3e} (bar {2 * tol['token_bar']:.3e})")
  assert s.epoch == m._cache_epoch, "lm_forward_loss is not a cache entry"


def _decode_step_rows(m, s, cuda):
  """One raw decode step of every row at its cached length, on fixed embeddings -> hidden rows (B, D) fp32."""
  from gill_amd import _native as N
  B, D = s.B, m.opt_cfg.hidden_size
  x = m.input_embeddings(torch.tensor([[11, 12, 13, 14][:B]], device=cuda))[0].to(torch.bfloat16).contiguous()
  lens = torch.tensor([bk.cached for bk in s.books], dtype=torch.int32, device=cuda)
  out = torch.zeros((B, D), dtype=torch.float32, device=cuda)
  N.check(N.lib().gill_opt_decode_step(s.handle, N.ptr(x), N.ptr(lens), B, max(CU.HISTORIES) + 1, N.ptr(out), N.current_stream()))
  torch.cuda.synchronize()
  return out.cpu()


def test_scoring_leaves_the_cache_as_it_was(cuda, gill125):
  from gill_amd import _native as N
  m = gill125.model
  s = _session(m)
  plain = _decode_step_rows(m, s, cuda)
  s = _session(m)                                   # the same rows again, this time scored before the step
  kv_bytes = N.lib().gill_opt_kv_bytes(s.handle)
  _score(m, _pack(s), cuda)
  assert N.lib().gill_opt_kv_bytes(s.handle) == kv_bytes
  scored = _decode_step_rows(m, s, cuda)
  assert torch.equal(plain.view(torch.int32), scored.view(torch.int32)), "a decode step after the scoring call differs: the call touched the cache"


def test_an_empty_candidate_scores_nothing(cuda, gill125):
  m = gill125.model
  s = _session(m)
  cands = [[], [[], [5, 6, 7]], [], [[9]]]
  p = _pack(s, cands)
  got = _split(p, _score(m, p, cuda))
  assert [g[3] for g in got] == [0, 3, 1]
  assert math.isnan(got[0][2]) and got[0][1] == 0.0 and got[0][0].numel() == 0
  assert math.isfinite(got[1][2]) and math.isfinite(got[2][2])
  sc = s.score([1, 3], [cands[1], cands[3]])
  assert math.isnan(float(sc[0][0])) and abs(float(sc[0][1]) - got[1][2]) == 0.0 and abs(float(sc[1][0]) - got[2][2]) == 0.0


def test_refusals_before_anything_runs(cuda, gill125):
  from gill_amd import _native as N
  m = gill125.model
  s = _session(m)
  p = _pack(s, [[[5, 6]], [], [], []])
  p.len_bound = m.opt_cfg.max_positions + 1
  with pytest.raises(N.GillNativeError, match="position table"):
    m._lm_score_candidates(p)
  try:
    m.quantize_kv("fp8")                            # drops the handle: the new one has no cache yet
    h = m._opt_native(len(CU.HISTORIES), CAPACITY)
    assert N.lib().gill_opt_kv_bytes(h) == 0
    p = _pack(s, [[[5, 6]], [], [], []])
    with pytest.raises(N.GillNativeError, match="e4m3"):
      m._lm_score_candidates(p)
    s8 = _session(m)
    with pytest.raises(N.GillNativeError, match="e4m3"):
      s8.score([0], [[[5, 6]]])
  finally:
    m.quantize_kv("bf16")
  h = m._opt_native(len(CU.HISTORIES), CAPACITY)
  assert N.lib().gill_opt_kv_bytes(h) == 0
  with pytest.raises(N.GillNativeError, match="no KV cache"):
    m._lm_score_candidates(p)
  torch.cuda.synchronize()


def test_w8_handle_meets_the_same_bars(cuda, gill125, tol):
  import w8_util as W
  m = gill125.model
  cfg, sd = R.gen_model()
  sd8 = W.w8_state_dict(sd, cfg)
  with torch.no_grad():
    oracle = [[CU.oracle_candidate(sd8, cfg, CU.history_ids(i), c) for c in cands] for i, cands in enumerate(CU.all_candidates())]
  try:
    m.quantize_lm("fp8")
    s = _session(m)
    p = _pack(s)
    _check_against("score_candidates w8", p, _split(p, _score(m, p, cuda)), oracle, tol)
  finally:
    m.quantize_lm("bf16")
