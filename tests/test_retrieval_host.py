"""CPU checks of the retrieval surface: the tests' own yardstick (tests/retrieval_util.py) agrees with torch.topk and rejects seeded mistakes,
the gill_ret_index_* symbols are bound, bad arguments come back as errors before anything touches a device, and GILL.retrieve_images refuses
to run without an index."""
import ctypes as C
import math
import os

import pytest
import torch

import retrieval_util as U

NAMES = ("gill_ret_index_create", "gill_ret_index_destroy", "gill_ret_index_add", "gill_ret_index_size", "gill_ret_index_rows",
         "gill_ret_index_search", "gill_ret_index_slabs")


def test_restatement_is_topk_on_tie_free_data():
  g = torch.Generator().manual_seed(5)
  rows = torch.randn((501, 40), generator=g, dtype=torch.float64)
  queries = torch.randn((7, 40), generator=g, dtype=torch.float64)
  S, mag = U.penalised_scores(rows, queries)
  assert torch.equal(S, queries @ rows.T) and bool((mag >= S.abs()).all())
  for k in (1, 3, 32):
    ws, wi = U.topk_ref(S, k)
    ts, ti = torch.topk(S, k, dim=1)
    assert torch.equal(ws, ts) and torch.equal(wi, ti)
    assert U.accept(ws, wi, S, 0.0)[0] and U.exact_equal(ws, wi, S, k)
  # the seen penalty: scores[idx] -= penalty, once per listed row, -1 slots ignored
  ex = [[3, 3, -1], [], [500], [-1], [0, 1, 2], [7], [9]]
  Sp, _ = U.penalised_scores(rows, queries, ex, 1000.0)
  want = S.clone()
  for q, r in ((0, 3), (2, 500), (4, 0), (4, 1), (4, 2), (5, 7), (6, 9)):
    want[q, r] -= 1000.0
  assert torch.equal(Sp, want)
  # k > N pads with (-inf, -1)
  ws, wi = U.topk_ref(S[:, :2], 3)
  assert wi[:, 2].tolist() == [-1] * 7 and bool((ws[:, 2] == -math.inf).all()) and U.accept(ws, wi, S[:, :2], 0.0)[0]


def test_ties_go_to_the_lower_index_and_the_rule_sees_mistakes():
  rows, queries = U.exact_inputs(300, 8, 3, seed=1)
  S, _ = U.penalised_scores(rows, queries)
  ws, wi = U.topk_ref(S, 16)
  for q in range(3):
    for j in range(15):
      assert ws[q, j] > ws[q, j + 1] or (ws[q, j] == ws[q, j + 1] and wi[q, j] < wi[q, j + 1])
  assert len(set(ws[0].tolist())) < 16            # the data does tie
  assert U.exact_equal(ws, wi, S, 16) and U.accept(ws, wi, S, 0.0)[0]
  # a swapped pair of equals passes the set rule but not the order pin; a missing best row, a repeated index, a wrong score, a rising pair fail
  j = next(j for j in range(15) if ws[0, j] == ws[0, j + 1])
  sw = wi.clone()
  sw[0, j], sw[0, j + 1] = wi[0, j + 1], wi[0, j]
  assert U.accept(ws, sw, S, 0.0)[0] and not U.exact_equal(ws, sw, S, 16)
  worst = int(S[0].argmax())
  Sx = S.clone()
  Sx[0, worst] += 1.0                                # now strictly the best row of query 0
  xs, xi = U.topk_ref(Sx, 17)
  assert not U.accept(xs[:, 1:], xi[:, 1:], Sx, 0.0)[0]
  rep = wi.clone()
  rep[1, 5] = rep[1, 4]
  assert not U.accept(ws, rep, S, 0.0)[0]
  bad = ws.clone()
  bad[2, 0] += 0.5
  assert not U.accept(bad, wi, S, 0.0)[0]
  assert ws[0, 0] > ws[0, -1] and not U.accept(ws.flip(1), wi.flip(1), S, 0.0)[0]
  # a bound admits what it covers and nothing more
  assert U.accept(bad, wi, S, 0.5)[0] and not U.accept(bad, wi, S, 0.49)[0]


def test_bounds_are_the_documented_formulas():
  mag = torch.tensor([[2.0, 4.0]], dtype=torch.float64)
  assert torch.equal(U.bound(mag, 256, False), 256 * 2.0 ** -24 * mag)
  assert torch.equal(U.bound(mag, 256, True), 256 * 2.0 ** -24 * mag + 2.0 ** -8 * mag)
  raw = torch.tensor([[3.0, 4.0], [0.0, 0.0]])
  assert torch.equal(U.normalized_rows(raw, 10.0), torch.tensor([[6.0, 8.0], [0.0, 0.0]], dtype=torch.float64))


def test_symbols_are_bound():
  from gill_amd import _native as N
  lib = N.lib()
  for n in NAMES:
    assert n in N.SYMBOLS and hasattr(lib, n), n
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gill_amd.h")).read()
  for n in NAMES:
    assert n + "(" in header
  from gill_amd.retrieval import GillRetrievalIndex      # noqa: F401


def test_bad_arguments_return_errors_not_crashes():
  from gill_amd import _native as N
  lib = N.lib()
  h = C.c_void_p()
  for dim, cap, word in ((12, 10, b"multiple of 8"), (1032, 10, b"1024"), (0, 10, b"multiple of 8"), (64, 0, b"capacity"), (64, 2 ** 31, b"capacity")):
    assert lib.gill_ret_index_create(C.byref(h), dim, cap) != 0 and not h.value, (dim, cap)
    assert word in lib.gill_last_error(), lib.gill_last_error()
  assert lib.gill_ret_index_create(None, 64, 10) != 0
  # a null handle
  assert lib.gill_ret_index_add(None, None, 1, 1, 0, 1.0, None) != 0 and b"null handle" in lib.gill_last_error()
  assert lib.gill_ret_index_rows(None, 0, 1, None, None) != 0 and b"null handle" in lib.gill_last_error()
  assert lib.gill_ret_index_search(None, None, 1, 1, 3, None, 0, 1000.0, None, None, None) != 0 and b"null handle" in lib.gill_last_error()
  assert lib.gill_ret_index_slabs(None, None, None, None) != 0 and b"null handle" in lib.gill_last_error()
  assert lib.gill_ret_index_size(None) == -1
  lib.gill_ret_index_destroy(None)
  # a real (still host-only) handle: every refusal comes before the first device call
  assert lib.gill_ret_index_create(C.byref(h), 64, 10) == 0 and h.value
  try:
    assert lib.gill_ret_index_size(h) == 0
    assert lib.gill_ret_index_add(h, None, 1, 11, 0, 1.0, None) != 0 and b"capacity" in lib.gill_last_error()      # past the capacity
    assert lib.gill_ret_index_add(h, None, 7, 1, 0, 1.0, None) != 0 and b"dtype" in lib.gill_last_error()
    assert lib.gill_ret_index_add(h, None, 1, -1, 0, 1.0, None) != 0
    assert lib.gill_ret_index_add(h, None, 1, 1, 0, 1.0, None) != 0 and b"aligned" in lib.gill_last_error()        # null rows
    assert lib.gill_ret_index_add(h, None, 1, 0, 0, 1.0, None) == 0                                                # nothing to add
    assert lib.gill_ret_index_size(h) == 0
    for k in (0, -1, 33):
      assert lib.gill_ret_index_search(h, None, 1, 1, k, None, 0, 1000.0, None, None, None) != 0 and b"k <= 32" in lib.gill_last_error()
    assert lib.gill_ret_index_search(h, None, 1, 1, 3, None, 65, 1000.0, None, None, None) != 0 and b"E <= 64" in lib.gill_last_error()
    assert lib.gill_ret_index_search(h, None, 0, 1, 3, None, 0, 1000.0, None, None, None) != 0
    assert lib.gill_ret_index_search(h, None, 1, 1, 3, None, 0, 1000.0, None, None, None) != 0 and b"aligned" in lib.gill_last_error()
    assert lib.gill_ret_index_rows(h, 0, 1, None, None) != 0 and b"inside" in lib.gill_last_error()
    assert lib.gill_ret_index_rows(h, -1, 0, None, None) != 0
    fr, nl, rp = C.c_int64(7), C.c_int(), C.c_int64()
    assert lib.gill_ret_index_slabs(h, C.byref(fr), C.byref(nl), C.byref(rp)) == 0 and (fr.value, nl.value, rp.value) == (0, 4, 16)
  finally:
    lib.gill_ret_index_destroy(h)


def test_python_index_refuses_bad_calls_without_a_device():
  from gill_amd import _native as N
  from gill_amd.retrieval import GillRetrievalIndex
  with pytest.raises(N.GillNativeError):
    GillRetrievalIndex(12, 10, "cpu")
  ix = GillRetrievalIndex(64, 10, "cpu")
  assert len(ix) == 0 and ix.slabs() == (0, 4, 16)
  with pytest.raises(ValueError):
    ix.add(torch.zeros(3, 32))
  with pytest.raises(ValueError):
    ix.add(torch.zeros(11, 64))
  with pytest.raises(ValueError):
    ix.search(torch.zeros(1, 64), 33)
  with pytest.raises(ValueError):
    ix.search(torch.zeros(1, 32), 3)
  with pytest.raises(ValueError):
    ix._exclude([[0] * 65], 1)
  with pytest.raises(ValueError):
    ix._exclude([[0], [1]], 1)
  ex = ix._exclude([[4, 5], [], [6]], 3)
  assert ex.tolist() == [[4, 5], [-1, -1], [6, -1]]
  with pytest.raises(IndexError):
    ix.rows(0, 1)


def test_retrieve_images_without_an_index_raises():
  from gill_amd.models import GILL
  m = GILL.__new__(GILL)
  torch.nn.Module.__init__(m)
  m.ret_index = None
  with pytest.raises(RuntimeError, match="build_retrieval_index"):
    m.retrieve_images(["a prompt"])
  m.emb_matrix = None
  m.model = torch.nn.Module()
  m.model.logit_scale = torch.nn.Parameter(torch.zeros(()))
  with pytest.raises(ValueError, match="emb_matrix"):
    m.build_retrieval_index()
