"""Branch decode end to end on the MI355X: DialogueSession.sample (n replies per dialogue from one cached history, gill_opt_decode_step_branch
over csrc/attention_branch.hip) and DialogueSession.adopt, on the OPT-125m rig of the session tests (B = 4 rows, capacity 128, 5 decisions).

  greedy    sample(n = 1, temperature = 0) on the first turn of the session test's plan "two" returns the tokens generate returns on a twin session
            (19 tokens: three free decisions, then two forced [IMG] blocks, which the branch path walks too);
  seeded    n = 4 on two rows of 33 and 70 tokens (branch_decode_util): branch j's tokens are those of a from-scratch
            generate_batch(ids = history, seed =, row_ids = [key_j]);
  untouched after sample the session's books and hidden_last are equal and a score call returns the bits it returned before;
  adopt     history(row) ends with the kept tokens; an extend with no new ids followed by generate agrees with a session that was fed history +
            reply from scratch (the session test's hidden-state bar and near-tie bar);
  propose   d.propose returns n truncated replies per active dialogue with the scores session.score gives them, ordered; d.choose adopts one
            and the dialogue goes on;
  refusals  an e4m3 handle raises, naming the format; a stale session raises StaleSessionError; a stale BranchSet raises on adopt.

A token disagreement is excused only when the reference's own logits put the two tokens' decision values within the recorded bar (greedy: the
session test's m on the logits; seeded: tests/golden/branch_decode_tolerance.json's m on the decision keys, 10 x the bf16 emulation's distance
from the oracle, measured by tools/branch_decode_tolerance.py), and the excused branches are capped at 10 % of the comparison's branches;
test_branch_host.py asserts on the CPU that the oracle's own run excuses none."""
import pytest
import torch

import branch_decode_util as Bd
import dialogue_session_util as S
import kv_cache_util as U
import ragged_decode_util as R
from gill_amd.dialogue import StaleSessionError
from test_generate_batch_gpu import _rel, rig   # noqa: F401  (rig: the module fixture of the batch-API test)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gill125(cuda):
  return R.gill125_rig(cuda)


def _book_state(s):
  return [(list(bk.ids), bk.n_extra, bk.cached, bk.turn_start, bk.ready) for bk in s.books]


def _reference_logits(m, ids, cuda):
  """The one-sequence reference's logits of the decision that follows `ids`."""
  _, _, logits = m.generate(m.input_embeddings(torch.tensor(ids, dtype=torch.int64)[None].to(cuda)), 1)
  return logits[0][0].float().cpu()


def test_greedy_single_branch_equals_generate_on_a_twin_session(cuda, gill125):
  m = gill125.model
  seeds = S.load_seeds()["two"]
  plan = sorted(S.PLANS["two"][0][1].items())
  prompts = [S.new_ids(0, r, n, first=True, seed=seeds[(0, r)]) for r, n in plan]
  rows = [r for r, _ in plan]
  s = m.open_session(S.B, S.CAPACITY)
  s.extend(rows, ids=prompts)
  bs = s.sample(rows, 1, max_len=S.MAX_LEN, **S.GEN_KW)
  assert bs.row == rows and bs.index == [0] * len(rows) and tuple(bs.tokens.shape) == (len(rows), 40)
  assert bs.n_tokens.tolist() == [S.N_TOK] * len(rows)
  twin = m.open_session(S.B, S.CAPACITY)
  twin.extend(rows, ids=prompts)
  tokens, n_tok, _, _ = twin.generate(rows, max_len=S.MAX_LEN, **S.GEN_KW)
  tol, excused = S.load_tolerance(), 0
  for k, r in enumerate(rows):
    got, want = bs.reply(r, 0), tokens[r, :int(n_tok[r])].tolist()
    if got != want:
      col = next(j for j in range(min(len(got), len(want))) if got[j] != want[j])
      assert col < 3, (r, got, want)                  # only a free decision can differ
      logits = _reference_logits(m, prompts[k] + want[:col], cuda)
      margin = abs(float(logits[got[col]] - logits[want[col]]))
      print(f"[branch decode greedy] row {r} decision {col}: branch picked {got[col]}, generate {want[col]}; the reference's logits are "
            f"{margin:.3e} apart (m = {tol:.3e})")
      assert margin <= tol, (r, col, margin)
      excused += 1
  assert excused <= Bd.EXCUSED_SHARE * len(rows), excused


def test_seeded_branches_equal_from_scratch_rows_and_adopt(cuda, gill125):
  m = gill125.model
  gold = Bd.golden()
  T, seed = float(gold["temperature"]), int(gold["sample_seed"])
  rows = list(Bd.ROWS)
  pseeds = Bd.prompt_seeds(gold)
  hist = {r: Bd.prompt_ids(r, n, pseeds[r]) for r, n in zip(Bd.ROWS, Bd.LENGTHS)}
  s = m.open_session(Bd.B, Bd.CAPACITY)
  s.extend(rows, ids=[hist[r] for r in rows])
  cands = [[[5, 6, 7], [8, 9]], [[10, 11, 12, 13]]]
  books0, hl0, epoch0, sc0 = _book_state(s), s.hidden_last.clone(), s.epoch, s.score(rows, cands)
  kw = dict(max_len=Bd.MAX_LEN, temperature=T, top_p=1.0, seed=seed)
  bs = s.sample(rows, Bd.N, **kw)
  assert bs.row == [r for r in rows for _ in range(Bd.N)] and bs.index == list(range(Bd.N)) * len(rows)
  assert tuple(bs.tokens.shape) == (len(rows) * Bd.N, Bd.MAX_LEN * 8) and bs.n_tokens.tolist() == [Bd.MAX_LEN] * (len(rows) * Bd.N)
  # the session is untouched
  assert _book_state(s) == books0 and torch.equal(s.hidden_last, hl0) and s.epoch == epoch0 == m._cache_epoch
  sc1 = s.score(rows, cands)
  for a, b in zip(sc0, sc1):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "score changed its bits after sample"
  assert gold["distinct_rows"]
  for r in gold["distinct_rows"]:       # the rows whose oracle run draws more than one reply (the synthetic model's logits are peaked)
    assert len({tuple(bs.reply(r, j)) for j in range(Bd.N)}) > 1, f"row {r}: every branch drew the same reply"
  # adopt: the row's last turn is the reply; one adopt per row
  kept = {}
  for r, j, keep in Bd.ADOPT:
    s.adopt(bs, r, j, keep)
    kept[r] = bs.reply(r, j)[:keep]
    assert s.history(r)[0].tolist() == hist[r] + kept[r]
    assert s.books[r].cached == len(hist[r]) + len(kept[r]) - 1 and s.books[r].turn_start == len(hist[r]) and not s.books[r].ready
  with pytest.raises(RuntimeError, match="no longer current"):
    s.adopt(bs, rows[0], 0)
  with pytest.raises(ValueError):
    s.adopt(bs, 1, 0)                                       # row 1 has no branch in the set
  s.extend(rows, ids=[[] for _ in rows])                    # the pending token alone
  ta, na, ha, nha = s.generate(rows, max_len=S.MAX_LEN, **S.GEN_KW)
  with pytest.raises(RuntimeError, match="no longer current"):
    s.adopt(bs, rows[1], 0)                                 # a cache-writing call since the set was drawn
  # a session fed history + reply from scratch
  s2 = m.open_session(Bd.B, Bd.CAPACITY)
  with pytest.raises(StaleSessionError):
    s.sample(rows, Bd.N, **kw)
  s2.extend(rows, ids=[hist[r] + kept[r] for r in rows])
  tb, nb, hb, nhb = s2.generate(rows, max_len=S.MAX_LEN, **S.GEN_KW)
  tol_s, excused = S.load_tolerance(), 0
  for r in rows:
    got, want = ta[r, :int(na[r])].tolist(), tb[r, :int(nb[r])].tolist()
    assert int(nb[r]) == S.N_TOK and int(nhb[r]) == S.N_HID
    if got != want:
      col = next(j for j in range(min(len(got), len(want))) if got[j] != want[j])
      assert col < 3, (r, got, want)
      logits = _reference_logits(m, hist[r] + kept[r] + want[:col], cuda)
      margin = abs(float(logits[got[col]] - logits[want[col]]))
      print(f"[branch decode adopt] row {r} decision {col}: after adopt {got[col]}, from scratch {want[col]}; the reference's logits are "
            f"{margin:.3e} apart (m = {tol_s:.3e})")
      assert margin <= tol_s, (r, col, margin)
      excused += 1
      continue
    rel = _rel(ha[r, :S.N_HID], hb[r, :S.N_HID])
    print(f"[branch decode adopt] row {r} (history {len(hist[r])} + reply {len(kept[r])}): hidden rows rel_l2 {rel:.3e}")
    assert rel < U.REL_BAR, (r, rel)
  assert excused <= Bd.EXCUSED_SHARE * len(rows), excused
  # every branch against a from-scratch generate_batch of its history with its key (the calls take the cache over)
  excused = 0
  for r in rows:
    ids = torch.tensor(hist[r], dtype=torch.int64)[None].to(cuda)
    for j in range(Bd.N):
      key = r * Bd.N + j
      tokens, n_tok, _, _ = m.generate_batch(ids=ids, lengths=[len(hist[r])], row_ids=[key], **kw)
      got, want = bs.reply(r, j), tokens[0, :int(n_tok[0])].tolist()
      if got != want:
        col = next(c for c in range(min(len(got), len(want))) if got[c] != want[c])
        keys = Bd.decision_keys(_reference_logits(m, hist[r] + want[:col], cuda), seed, key, col, T)
        margin = abs(float(keys[got[col]] - keys[want[col]]))
        print(f"[branch decode seeded] row {r} branch {j} decision {col}: branch drew {got[col]}, from scratch {want[col]}; the reference's "
              f"decision keys are {margin:.3e} apart (m = {gold['m']:.3e})")
        assert margin <= gold["m"], (r, j, col, margin)
        excused += 1
  assert excused <= Bd.EXCUSED_SHARE * len(rows) * Bd.N, excused
  with pytest.raises(StaleSessionError):
    s2.sample(rows, 1)


def test_sample_refusals(cuda, gill125):
  from gill_amd import _native as N
  m = gill125.model
  s = m.open_session(Bd.B, Bd.CAPACITY)
  with pytest.raises(RuntimeError, match="extend"):
    s.sample([0], 2, temperature=1.0, seed=3)
  s.extend([0], ids=[[2, 5, 6, 7]])
  with pytest.raises(ValueError, match="equal"):
    s.sample([0], 2)
  with pytest.raises(ValueError, match="seed"):
    s.sample([0], 2, temperature=1.0)
  with pytest.raises(ValueError, match="position table"):
    s.sample([0], 2, max_len=m.opt_cfg.max_positions, temperature=1.0, seed=3)
  with pytest.raises(ValueError, match="keys"):
    s.sample([0], 2, temperature=1.0, seed=3, keys=[1])
  try:
    m.quantize_kv("fp8")
    s8 = m.open_session(Bd.B, Bd.CAPACITY)
    s8.extend([0], ids=[[2, 5, 6, 7]])
    with pytest.raises(N.GillNativeError, match="e4m3"):
      s8.sample([0], 2, max_len=2, temperature=1.0, seed=3)
  finally:
    m.quantize_kv("bf16")


def test_propose_ranks_sampled_replies_and_choose_adopts_one(rig):   # noqa: F811
  g = rig.m
  d = g.open_dialogues(2, capacity=256)
  with pytest.raises(RuntimeError, match="propose"):
    d.choose(0, 0)
  out = d.propose([["a photo of", "a small red kite"], None], n=3, num_words=4, temperature=1.5, top_p=0.95, seed=5)
  assert out[1] is None and d.history(1)[0].numel() == 0
  o = out[0]
  assert len(o["texts"]) == len(o["tokens"]) == 3 and tuple(o["scores"].shape) == (3,) and sorted(o["order"]) == [0, 1, 2]
  assert all(isinstance(t, str) for t in o["texts"]) and all(1 <= len(t) <= 4 * 8 for t in o["tokens"])
  sc = o["scores"].tolist()
  assert all(sc[a] >= sc[b] for a, b in zip(o["order"], o["order"][1:])) and o["best"] == o["order"][0]
  hist0 = d.history(0)[0].tolist()
  again = d.session.score([0], [o["tokens"]])[0]           # nothing was adopted: the dialogue still ends with the turn
  assert torch.equal(again.view(torch.int32), o["scores"].view(torch.int32))
  j = o["order"][-1]
  d.choose(0, j)
  assert d.history(0)[0].tolist() == hist0 + o["tokens"][j]
  with pytest.raises(RuntimeError, match="no longer current"):
    d.choose(0, o["best"])                                  # one choice per dialogue and proposal
  with pytest.raises(ValueError):
    d.choose(1, 0)                                          # dialogue 1 was idle
  got = d.say([["and next to it"], None], num_words=2, min_word_tokens=0, gen_scale_factor=1e5)      # the dialogue goes on
  assert got[1] is None and got[0][0].endswith("[IMG7]")
  assert d.history(0)[0].tolist()[:len(hist0) + len(o["tokens"][j])] == hist0 + o["tokens"][j]
