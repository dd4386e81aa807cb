"""The host side of branch decode, on the CPU: pack_branches (order, the cut at 32, the default keys), the books after an adopt with keep, the
argument errors of DialogueSession.sample (raised before the engine is touched), the new C symbols in the header and in the library with their
ctypes signatures and host-side argument errors, and the proof that the seeded run of test_branch_decode_gpu.py needs no excusal by itself: the
fp32 oracle's own run of it (branch_decode_util.oracle_run) has no decision whose two largest decision keys are within the recorded bar m, m is
MARGIN x the bf16-operand emulation's key distance from the oracle measured on that very run (tools/branch_decode_tolerance.py), no branch picks
an [IMG] token and the rows recorded as such draw more than one reply."""
import ctypes as C
import os

import pytest
import torch

import branch_decode_util as Bd
import dialogue_session_util as S
from gill_amd import dialogue as Dg
from test_dialogue_session_host import _StubModel


def test_pack_branches_orders_by_dialogue_and_cuts_groups_at_32():
  gstart, gparent, gplen, own = Dg.pack_branches([2, 0], 4, [33, 70])
  assert gstart == [0, 4, 8] and gparent == [2, 0] and gplen == [33, 70]
  assert own == [(2, j) for j in range(4)] + [(0, j) for j in range(4)]
  gstart, gparent, gplen, own = Dg.pack_branches([3, 1, 0], 33, [5, 9, 0])
  assert gstart == [0, 32, 33, 65, 66, 98, 99] and gparent == [3, 3, 1, 1, 0, 0] and gplen == [5, 5, 9, 9, 0, 0]
  assert own[31:34] == [(3, 31), (3, 32), (1, 0)] and len(own) == 99
  assert max(b - a for a, b in zip(gstart, gstart[1:])) == Dg.BRANCH_GROUP
  gstart, gparent, _, own = Dg.pack_branches([1], 64, [7])
  assert gstart == [0, 32, 64] and gparent == [1, 1] and own[32] == (1, 32)
  assert Dg.pack_branches([], 3, []) == ([0], [], [], [])
  with pytest.raises(ValueError):
    Dg.pack_branches([0], 0, [4])
  with pytest.raises(ValueError):
    Dg.pack_branches([0, 1], 2, [4])
  # the default Philox keys of sample: row * n + j, the branch's place in generate_batch's row_ids numbering
  assert [r * 4 + j for r, j in Dg.pack_branches([2, 0], 4, [1, 1])[3]] == [8, 9, 10, 11, 0, 1, 2, 3]


def test_branch_set_lookup_and_the_books_after_adopt_with_keep():
  tokens = torch.tensor([[11, 12, 13, -1], [21, 22, -1, -1], [31, 32, 33, 34]])
  bs = Dg.BranchSet(tokens, torch.tensor([3, 2, 4]), [0, 0, 2], [0, 1, 0], [5, 5, 9], serial=1)
  assert bs.find(0, 1) == 1 and bs.find(2, 0) == 2 and bs.reply(0, 0) == [11, 12, 13] and bs.reply(2, 0) == [31, 32, 33, 34]
  with pytest.raises(ValueError):
    bs.find(1, 0)
  # what adopt does to the row's book: the kept tokens join the history, the newest stays pending (count = keep - 1 slots were copied)
  bk = Dg.RowBook()
  bk.append([2, 10, 11, 12, 13])
  bk.fed()
  bk.generated(bs.reply(0, 0)[:2])
  assert bk.ids == [2, 10, 11, 12, 13, 11, 12] and bk.cached == 6 and bk.turn_start == 5 and not bk.ready and bk.feed() == [12]
  bk.rollback(1)                                          # as after a generate that had emitted those tokens
  assert bk.ids[-1] == 11 and bk.cached == 5 and bk.feed() == [11]
  bk2 = Dg.RowBook()
  bk2.append([2, 10])
  bk2.fed()
  bk2.generated([])                                       # keep = 0: nothing joins, nothing is pending
  assert bk2.ids == [2, 10] and bk2.cached == 2 and not bk2.ready


class _Stub(_StubModel):
  retrieval_token_idx = list(range(8))


def test_sample_argument_errors_come_before_the_engine():
  m = _Stub()
  s = Dg.DialogueSession(m, 3, 64)
  with pytest.raises(RuntimeError, match="extend"):
    s.sample([0], 2, temperature=1.0, seed=1)             # not ready
  s.extend([0, 2], ids=[[2, 10, 11], [2, 12]])
  with pytest.raises(ValueError, match="equal"):
    s.sample([0], 2)                                      # n > 1 greedy: all branches would be equal
  with pytest.raises(ValueError, match="top_p"):
    s.sample([0], 1, top_p=0.9)
  with pytest.raises(ValueError, match="seed"):
    s.sample([0], 2, temperature=0.7)
  with pytest.raises(ValueError, match="seed"):
    s.sample([0], 2, temperature=0.7, seed=-1)
  with pytest.raises(ValueError, match="n >= 1"):
    s.sample([0], 0, temperature=0.7, seed=1)
  with pytest.raises(ValueError, match="n >= 1"):
    s.sample([], 2, temperature=0.7, seed=1)
  with pytest.raises(ValueError):
    s.sample([0, 0], 2, temperature=0.7, seed=1)
  with pytest.raises(RuntimeError, match="extend"):
    s.sample([0, 1], 2, temperature=0.7, seed=1)          # row 1 is empty
  with pytest.raises(ValueError, match="position table"):
    s.sample([0], 2, max_len=32, temperature=0.7, seed=1)     # 3 + 32 * 8 > 256
  with pytest.raises(ValueError, match="keys"):
    s.sample([0, 2], 2, max_len=2, temperature=0.7, seed=1, keys=[0, 1, 2])
  with pytest.raises(ValueError, match="keys"):
    s.sample([0], 2, max_len=2, temperature=0.7, seed=1, keys=[0, -1])
  m._cache_epoch += 1
  with pytest.raises(Dg.StaleSessionError):
    s.sample([0], 2, temperature=0.7, seed=1)
  with pytest.raises(Dg.StaleSessionError):
    s.adopt(Dg.BranchSet(torch.zeros((1, 1)), torch.tensor([1]), [0], [0], [3], serial=0), 0, 0)


def test_new_symbols_are_in_the_header_and_load_with_their_signatures():
  from gill_amd import _native as N
  lib = N.lib()
  vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
  want = {
    "gill_attention_branch": (i, [vp] * 3 + [i] + [vp] * 9 + [i] * 8 + [vp, vp]),
    "gill_kv_branch_adopt": (i, [vp] * 4 + [i] * 10 + [vp]),
    "gill_opt_branch_reserve": (i, [vp, i, i]),
    "gill_opt_branch_bytes": (i64, [vp]),
    "gill_opt_decode_step_branch": (i, [vp] * 6 + [i, i, i, vp, vp]),
    "gill_opt_next_token_branch": (i, [vp, vp, i, C.POINTER(N.gill_decode_rule), i, C.POINTER(N.gill_decode_sampler), vp, vp, vp, i, vp, vp]),
    "gill_opt_branch_adopt": (i, [vp, i, i, i, i, vp]),
  }
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gill_amd.h")).read()
  for name, (res, args) in want.items():
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args, name
    assert f" {name}(" in header, f"{name} is not declared in include/gill_amd.h"
  # argument errors come back as codes with a message, without a GPU
  assert lib.gill_attention_branch(None, None, None, 0, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 12, 64, 96, 32, None,
                                   None) != 0
  assert b"branch attention" in lib.gill_last_error()
  assert lib.gill_kv_branch_adopt(None, None, None, None, 1, 1, 12, 64, 96, 32, 0, 0, 0, 1, None) != 0
  assert b"branch adopt" in lib.gill_last_error()
  assert lib.gill_opt_branch_reserve(None, 4, 33) != 0
  assert lib.gill_opt_branch_bytes(None) == 0
  assert lib.gill_opt_decode_step_branch(None, None, None, None, None, None, 1, 1, 1, None, None) != 0
  assert lib.gill_opt_branch_adopt(None, 0, 0, 0, 1, None) != 0


def test_oracle_seeded_run_of_the_branches_has_no_near_tie():
  gold = Bd.golden()
  assert gold["margin_factor"] == Bd.MARGIN and gold["temperature"] == Bd.TEMPERATURE and gold["excused_share_cap"] == Bd.EXCUSED_SHARE
  run = Bd.oracle_run(Bd.prompt_seeds(gold), int(gold["sample_seed"]))
  print(f"[branch decode] {len(run['branches']) * Bd.MAX_LEN} seeded decisions, bf16 emulation vs oracle key distance {run['dist']:.3e}, m = "
        f"{gold['m']:.3e}; smallest oracle top-2 key margin {run['margin']:.3e}; greedy after adopt: smallest margin {run['greedy_margin']:.3e}")
  assert abs(gold["m"] - Bd.MARGIN * run["dist"]) <= 1e-3 * gold["m"]
  assert run["margin"] >= gold["m"], "a decision of the oracle's own run is a near tie: the reference alone would need an excusal"
  assert not run["img"] and gold["distinct_rows"]
  for r in gold["distinct_rows"]:
    assert len({tuple(run["branches"][(r, j)][0]) for j in range(Bd.N)}) > 1
  assert run["greedy_margin"] >= max(S.load_tolerance(), Bd.MARGIN * run["greedy_dist"])
