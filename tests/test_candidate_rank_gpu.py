"""Candidate ranking end to end on the MI355X: DialogueSession.score, GillDialogues.rank and GILL.rank_candidates, on the rigs of the dialogue
tests.  Inputs, oracle and bars: candidate_rank_util (tests/golden/candidate_rank_tolerance.json, tools/candidate_rank_tolerance.py).

  ranking       per dialogue the order of the ten candidates' mean scores equals the oracle's for every pair whose oracle gap exceeds twice
                the mean bar (at most 10 % of a dialogue's pairs are left out), and every mean is within the bar;
  twin sessions one session scores between two turns, its twin does not: the second turn's tokens and hidden_last are bit-equal, and the
                scoring session is not stale;
  pending       a row after generate (its newest token pending) scores within the bars of the oracle on its history, as a fresh row does;
  chunked       a call split into several packs equals the unsplit one within the bars;
  one-shot      GILL.rank_candidates with an image in the context agrees with the session route on the same prompt within the bars;
  rank()        GillDialogues.rank returns the scores of the tokenised strings, ordered."""
import math

import pytest
import torch

import candidate_rank_util as CU
import dialogue_session_util as S
import ragged_decode_util as R
from gill_amd.dialogue import segment_turn
from test_generate_batch_gpu import rig   # noqa: F401  (the module fixture of the batch-API test: a GILL with a tiny CLIP tower)

pytestmark = pytest.mark.gpu

CAPACITY = 128
ROWS = list(range(len(CU.HISTORIES)))


@pytest.fixture(scope="module")
def gill125(cuda):
  return R.gill125_rig(cuda)


@pytest.fixture(scope="module")
def tol():
  return CU.load_tolerance()


def _session(m, capacity=CAPACITY):
  s = m.open_session(len(ROWS), capacity)
  s.extend(ROWS, ids=[CU.history_ids(i) for i in ROWS])
  return s


def test_session_scores_rank_as_the_oracle_and_chunking_changes_nothing_beyond_the_bars(cuda, gill125, tol):
  m = gill125.model
  s = _session(m)
  epoch, books = s.epoch, [(list(bk.ids), bk.cached, bk.ready) for bk in s.books]
  hidden = s.hidden_last.clone()
  scores, tokens = s.score(ROWS, CU.all_candidates(), return_tokens=True)
  sums = s.score(ROWS, CU.all_candidates(), reduce='sum')
  oracle = CU.oracle_all()
  for i in ROWS:
    want = [float(o.mean()) for o in oracle[i]]
    assert scores[i].shape == (len(CU.COUNTS),) and scores[i].dtype == torch.float32 and not scores[i].is_cuda
    worst = max(abs(float(scores[i][j]) - want[j]) for j in range(len(want)))
    assert worst < tol["mean_bar"], (i, worst)
    for j, n in enumerate(CU.COUNTS):
      assert tokens[i][j].shape == (n,) and float((tokens[i][j] - oracle[i][j]).abs().max()) < tol["token_bar"]
      assert abs(float(sums[i][j]) - float(scores[i][j]) * n) <= 1e-4 * abs(float(sums[i][j])) + 1e-4
    share = CU.check_order(f"dialogue {i}", scores[i].tolist(), want, tol["mean_bar"])
    print(f"[candidate rank] dialogue {i}: worst mean distance {worst:.3e} (bar {tol['mean_bar']:.3e}), {share:.1%} of the pairs left out")
  # the session is as it was
  assert s.epoch == epoch == m._cache_epoch and [(list(bk.ids), bk.cached, bk.ready) for bk in s.books] == books
  assert torch.equal(s.hidden_last, hidden)
  # several packs instead of one
  ch, ch_tok = s.score(ROWS, CU.all_candidates(), return_tokens=True, max_packed=200)
  for i in ROWS:
    assert float((ch[i] - scores[i]).abs().max()) < tol["mean_bar"]
    assert all(float((a - b).abs().max()) < tol["token_bar"] for a, b in zip(ch_tok[i], tokens[i]))


def test_a_session_that_scores_between_turns_decodes_as_its_twin(cuda, gill125, tol):
  m = gill125.model
  cfg, sd = R.gen_model()
  turn2 = [[101 + 3 * r, 205, 77 + r] for r in ROWS]
  cands = [[[400 + r, 17, 923], [31 + r]] for r in ROWS]

  def run(score):
    s = _session(m, 192)         # two turns of 19 tokens behind the longest history
    s.generate(ROWS, max_len=S.MAX_LEN, **S.GEN_KW)
    got = s.score(ROWS, cands, return_tokens=True) if score else None      # every row carries a pending token here
    hist = [s.history(r)[0].tolist() for r in ROWS]
    s.extend(ROWS, ids=turn2)
    tokens, n_tok, _, _ = s.generate(ROWS, max_len=S.MAX_LEN, **S.GEN_KW)
    return tokens.cpu(), n_tok.cpu(), s.hidden_last.cpu().clone(), got, hist

  t0, n0, h0, _, _ = run(False)
  t1, n1, h1, (scores, tokens), hist = run(True)
  assert torch.equal(t0, t1) and torch.equal(n0, n1), "the second turn's tokens differ after a scoring call"
  assert torch.equal(h0.view(torch.int32), h1.view(torch.int32)), "hidden_last differs after a scoring call"
  # pending rows score like fresh ones: against the oracle on the history as the session holds it (rows 1 and 2: the shortest)
  with torch.no_grad():
    for r in (1, 2):
      for j, c in enumerate(cands[r]):
        want = CU.oracle_candidate(sd, cfg, hist[r], c)
        assert float((tokens[r][j] - want).abs().max()) < tol["token_bar"], (r, j)
        assert abs(float(scores[r][j]) - float(want.mean())) < tol["mean_bar"], (r, j)


def test_score_argument_errors(cuda, gill125):
  from gill_amd.dialogue import StaleSessionError
  m = gill125.model
  s = _session(m)
  with pytest.raises(NotImplementedError):
    s.score([0], [[[5, -1]]])
  with pytest.raises(ValueError, match="reduce"):
    s.score([0], [[[5]]], reduce="max")
  with pytest.raises(ValueError):
    s.score([0, 1], [[[5]]])
  with pytest.raises(ValueError, match="workspace"):
    s.score([0], [[list(range(3, 40))]], max_packed=8)
  m.open_session(1, 64)
  with pytest.raises(StaleSessionError):
    s.score([0], [[[5]]])


def test_one_shot_rank_candidates_agrees_with_the_session_route_and_rank_orders(rig, tol):   # noqa: F811
  g = rig.m
  m = g.model
  prompt = [rig.img, rig.text]
  strings = ["a small red kite", "two brown dogs on a beach", "kite", "and next to it a very long reply about nothing in particular at all"]
  one = g.rank_candidates(prompt, strings)
  assert sorted(one["order"]) == list(range(len(strings))) and one["best"] == one["order"][0]
  sc = one["scores"].tolist()
  assert all(math.isfinite(v) for v in sc) and all(sc[a] >= sc[b] for a, b in zip(one["order"], one["order"][1:]))
  # the session route on the same prompt
  ids, images, done = segment_turn(m.tokenizer, prompt, m.args.n_visual_tokens, False, False, g._is_image)
  s = m.open_session(1, len(ids) + 1)
  s.extend([0], ids=[ids], extra_rows=[g._visual_rows(images)])
  cand = [[int(v) for v in m.tokenizer(c, add_special_tokens=not done, return_tensors="pt").input_ids[0].tolist()] for c in strings]
  want = {reduce: s.score([0], [cand], reduce=reduce)[0] for reduce in ("mean", "sum")}
  assert float((one["scores"] - want["mean"]).abs().max()) < tol["mean_bar"]
  got_sum = g.rank_candidates(prompt, strings, reduce="sum")["scores"]             # (a new session: s is stale from here on)
  assert float((got_sum - want["sum"]).abs().max()) < tol["mean_bar"] * max(len(c) for c in cand)
  # GillDialogues.rank: the strings tokenised without <bos> once the dialogue has one, None for an idle dialogue, the dialogue untouched
  d = g.open_dialogues(2, capacity=CAPACITY)
  d.say([prompt, ["a photo of"]], num_words=2, min_word_tokens=0, gen_scale_factor=1e5)
  before = [d.history(b)[0].tolist() for b in range(2)]
  got = d.rank([strings, None])
  assert got[1] is None and [d.history(b)[0].tolist() for b in range(2)] == before
  direct = d.session.score([0], [[[int(v) for v in m.tokenizer(c, add_special_tokens=False, return_tensors="pt").input_ids[0].tolist()]
                                  for c in strings]])[0]
  assert torch.equal(got[0]["scores"], direct) and got[0]["best"] == got[0]["order"][0] == int(direct.argmax())
  d.say([["and next to it"], None], num_words=2, min_word_tokens=0, gen_scale_factor=1e5)      # ranking left the session usable
