"""Candidate ranking, the parts that run without a GPU: the packing of DialogueSession.score (dialogue.pack_candidates), rank_order, the
argument errors, and the tolerance file of the GPU tests (tests/golden/candidate_rank_tolerance.json) with its recorded oracle check."""
import math

import pytest
import torch

import candidate_rank_util as CU
import ragged_decode_util as R
from gill_amd.dialogue import RowBook, pack_candidates, rank_order


def test_fresh_row_reruns_its_last_history_token():
  # fresh from extend: every history token is cached; the last one is fed again as the predictor of cand[0]
  (p,) = pack_candidates([(0, [2, 10, 11, 12], 4, 0)], [[[20, 21, 22], [30]]])
  assert p.plen == [3, 3] and p.parent == [0, 0] and p.cu == [0, 3, 4]
  assert p.ids == [12, 20, 21, 12] and p.targets == [20, 21, 22, 30]
  assert p.own == [(0, 0, 0, 3), (0, 1, 3, 1)] and p.max_new == 3 and p.len_bound == 6 and p.total_new == 4 and p.n_candidates == 2


def test_pending_token_and_unfed_tokens_are_fed_with_ignored_targets():
  bk = RowBook()
  bk.append([2, 10, 11])
  bk.fed()
  bk.generated([40, 41])                 # 41 is pending: cached = 4 of 5
  (p,) = pack_candidates([(3, bk.ids, bk.cached, 0)], [[[20, 21]]])
  assert p.plen == [4] and p.parent == [3] and p.ids == [41, 20] and p.targets == [20, 21] and p.own == [(0, 0, 0, 2)]
  bk.append([50, 51])                    # two more tokens no extend has fed: history tail [41, 50, 51]
  (p,) = pack_candidates([(3, bk.ids, bk.cached, 0)], [[[20, 21]]])
  assert p.plen == [4] and p.ids == [41, 50, 51, 20] and p.targets == [-100, -100, 20, 21] and p.own == [(0, 0, 2, 2)] and p.len_bound == 8


def test_empty_history_one_token_candidate_and_empty_candidate():
  (p,) = pack_candidates([(1, [], 0, 0)], [[[20, 21, 22], [30], []]])
  # cand[0] has no predictor and is unscored; a one-token candidate and an empty one bring no rows
  assert p.plen == [0, 0, 0] and p.cu == [0, 2, 2, 2] and p.ids == [20, 21] and p.targets == [21, 22]
  assert p.own == [(0, 0, 0, 2), (0, 1, 2, 0), (0, 2, 2, 0)] and p.max_new == 2
  (p,) = pack_candidates([(0, [2], 1, 0)], [[[30], []]])          # a one-token history: plen 0, the <bos> is re-run
  assert p.plen == [0, 0] and p.ids == [2] and p.targets == [30] and p.cu == [0, 1, 1] and p.own == [(0, 0, 0, 1), (0, 1, 1, 0)]


def test_grouping_by_parent_negative_ids_and_chunking():
  rows = [(2, [-1, -2, 5], 2, 4), (0, [2, 7, 8, 9], 4, 0)]      # row 2: its visual rows start at row 4 of the call's table; tail [5]
  cands = [[[11, 12], [13]], [[14, 15, 16]]]
  (p,) = pack_candidates(rows, cands)
  assert p.parent == [2, 2, 0] and p.plen == [2, 2, 3] and p.ids == [5, 11, 5, 9, 14, 15] and p.cu == [0, 2, 3, 6]
  rows[0] = (2, [-1, -2], 0, 4)                                  # nothing cached: the visual ids themselves are fed, moved by the offset
  (p,) = pack_candidates(rows, cands)
  assert p.ids[:3] == [-5, -6, 11] and p.targets[:3] == [-100, 11, 12] and p.plen[:2] == [0, 0] and p.own[0] == (0, 0, 1, 2)
  # chunking: no candidate is split, the order stands, every pack within the limit
  packs = pack_candidates(rows, cands, limit=4)
  assert [q.cu for q in packs] == [[0, 3], [0, 2], [0, 3]] and [q.parent for q in packs] == [[2], [2], [0]]
  assert [q.own for q in packs] == [[(0, 0, 1, 2)], [(0, 1, 1, 1)], [(1, 0, 0, 3)]]
  assert sum(q.total_new for q in packs) == p.total_new and all(q.total_new <= 4 for q in packs)
  packs = pack_candidates(rows, cands, limit=5)
  assert [q.cu for q in packs] == [[0, 3, 5], [0, 3]]


def test_argument_errors():
  with pytest.raises(NotImplementedError, match="text only"):
    pack_candidates([(0, [2, 3], 2, 0)], [[[5, -1]]])
  with pytest.raises(ValueError, match="one candidate list per named row"):
    pack_candidates([(0, [2, 3], 2, 0)], [[[5]], [[6]]])
  with pytest.raises(ValueError, match="workspace"):
    pack_candidates([(0, [2, 3], 2, 0)], [[[5, 6, 7, 8]]], limit=3)


def test_rank_order_puts_nan_last_and_breaks_ties_by_index():
  r = rank_order(torch.tensor([-3.0, float("nan"), -1.0, -3.0]))
  assert r["order"] == [2, 0, 3, 1] and r["best"] == 2
  assert rank_order(torch.tensor([float("nan")]))["best"] is None and rank_order(torch.zeros(0))["order"] == []


def test_tolerance_file_and_its_recorded_oracle_check():
  t = CU.load_tolerance()
  assert t["histories"] == list(CU.HISTORIES) and t["counts"] == list(CU.COUNTS) and t["margin"] == CU.MARGIN
  assert t["token_bar"] == CU.MARGIN * t["token_distance"] and t["mean_bar"] == CU.MARGIN * t["mean_distance"]
  assert 0 < t["mean_distance"] <= t["token_distance"] < 1.0
  # what the ranking test leaves out, from the recorded oracle means: within the cap, and as recorded
  for i, means in enumerate(t["oracle_means"]):
    assert len(means) == len(CU.COUNTS)
    share = len(CU.left_out_pairs(means, t["mean_bar"])) / 45
    assert share == pytest.approx(t["left_out_share"][i]) and share <= CU.LEFT_OUT_CAP
  # the recorded oracle means are the oracle's: the shortest dialogue (a one-token history) recomputed here
  cfg, sd = R.gen_model()
  i = CU.HISTORIES.index(min(CU.HISTORIES))
  with torch.no_grad():
    for j in (0, 3, 9):
      got = float(CU.oracle_candidate(sd, cfg, CU.history_ids(i), CU.candidate_ids(i, j)).mean())
      assert math.isclose(got, t["oracle_means"][i][j], rel_tol=1e-4, abs_tol=1e-3), (j, got, t["oracle_means"][i][j])
