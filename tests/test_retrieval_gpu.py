"""gill_ret_index_* on the GPU against the fp64 restatement of tests/retrieval_util.py: exact integer data bit for bit (ties to the lower index),
maxima placed in the ragged last tile / inside one wave's slab / one per slab, the seen penalty, real-valued data under the derived bounds,
the device normalise of add(), the blocked layout's round trip, chunked adds and run-to-run determinism.  Every output sits in front of guard
words that must survive."""
import math

import pytest
import torch

import retrieval_util as U

pytestmark = pytest.mark.gpu


def _index(rows, cuda, dtype=torch.float32, normalize=False, scale=1.0, capacity=None):
  from gill_amd.retrieval import GillRetrievalIndex
  ix = GillRetrievalIndex(rows.shape[1], capacity or max(1, rows.shape[0]), cuda)
  ix.add(rows.to(dtype), normalize=normalize, scale=scale)
  assert len(ix) == rows.shape[0]
  return ix


def _search(ix, queries, k, **kw):
  """search() into guarded outputs -> (scores, idx) on the CPU; asserts the guards."""
  Q = queries.shape[0]
  sb, scores = U.guarded((Q, k), torch.float32, ix.device)
  ib, idx = U.guarded((Q, k), torch.int64, ix.device)
  s2, i2 = ix.search(queries.float(), k, _out=(scores, idx), **kw)
  torch.cuda.synchronize()
  assert s2 is scores and i2 is idx
  assert U.guard_ok(sb) and U.guard_ok(ib), "search wrote past its outputs"
  return scores.cpu(), idx.cpu()


# (N, dim, Q, k): every N of {1, 15, 16, 17, 4099, 70001}, dim of {8, 40, 64, 256} (40: zero-padded to 64), Q of {1, 3, 16, 17, 33} (17, 33: more
# than one pass), k of {1, 3, 16, 32}; k > N four times
EXACT = [(1, 8, 1, 1), (1, 40, 3, 3), (15, 40, 3, 16), (16, 64, 16, 16), (17, 8, 17, 32), (17, 256, 1, 3), (4099, 40, 33, 3), (4099, 256, 1, 32),
         (4099, 64, 16, 1), (70001, 256, 16, 3), (70001, 64, 17, 16), (70001, 8, 3, 32), (70001, 40, 1, 1)]


# every instance of the search kernel: k-steps 3 (of 4), 4, 5 (of 8), 10 (of 16), 16, 17 (of 32), 32; from 16 k-steps on the loop has another shape
EXACT += [(4099, 96, 3, 3), (4099, 128, 2, 16), (4099, 160, 3, 3), (4099, 320, 17, 3), (4099, 512, 3, 32), (4099, 520, 3, 3), (4099, 1024, 16, 16),
          (20001, 1000, 2, 3)]


@pytest.mark.parametrize("N,dim,Q,k", EXACT)
def test_exact_integer_data_bit_for_bit(cuda, N, dim, Q, k):
  rows, queries = U.exact_inputs(N, dim, Q, seed=N + dim + Q)
  ix = _index(rows, cuda)
  scores, idx = _search(ix, queries, k, normalize=False)
  S, mag = U.penalised_scores(rows, queries)
  assert mag.max().item() < 2 ** 24
  ok, why = U.accept(scores, idx, S, 0.0)
  assert ok, why
  assert U.exact_equal(scores, idx, S, k), "order among equal scores: the lower index first"


def test_exact_input_dtypes_store_the_same_rows(cuda):
  rows, queries = U.exact_inputs(333, 40, 2, seed=3)
  want = None
  for dt in (torch.float32, torch.float16, torch.bfloat16):
    ix = _index(rows, cuda, dtype=dt)
    got = ix.rows(0, 333).cpu()
    assert torch.equal(got.double(), rows), dt
    want = got if want is None else want
    assert torch.equal(got, want)
    assert torch.equal(ix.rows(17, 40).cpu(), want[17:57])


@pytest.fixture(scope="module")
def placed_base():
  rows, queries = U.exact_inputs(70001, 256, 3, seed=11)
  queries[0][queries[0] == 0] = 1.0        # |q_i| >= 1: (8 + j) q beats every row of the base data (|a_i| <= 4) for this query
  return rows, queries


def _placed(cuda, rows, queries, where, k):
  rows = rows.clone()
  for j, r in enumerate(where):
    rows[r] = (8 + j) * queries[0]          # integers of magnitude <= 39 * 4: exact in bf16
  ix = _index(rows, cuda)
  scores, idx = _search(ix, queries, k, normalize=False)
  S, mag = U.penalised_scores(rows, queries)
  assert mag.max().item() < 2 ** 24
  ok, why = U.accept(scores, idx, S, 0.0)
  assert ok, why
  assert U.exact_equal(scores, idx, S, k)
  assert idx[0].tolist() == list(reversed(where))[:k]      # the largest multiple first
  return ix


def test_placed_maxima_in_the_ragged_last_tile(cuda, placed_base):
  rows, queries = placed_base
  N = 4099                                  # 4099 = 16 * 256 + 3: the last tile holds three rows
  _placed(cuda, rows[:N], queries, [N - 3, N - 2, N - 1], 3)
  _placed(cuda, rows[:N], queries, [N - 1], 1)


def test_placed_maxima_inside_one_slab(cuda, placed_base):
  rows, queries = placed_base
  from gill_amd.retrieval import GillRetrievalIndex
  probe = GillRetrievalIndex(256, 70001, cuda)
  probe.add(rows[:1].float())
  assert probe.slabs() == (0, 4, 16)
  ix = _index(rows, cuda)
  first, nlists, per = ix.slabs()
  assert first > 32 and first + nlists * per >= 70001 and nlists >= 64 and per >= 32       # a prefix pass, then the main pass
  lo = first + (nlists // 3) * per
  _placed(cuda, rows, queries, list(range(lo, lo + 32)), 32)                        # one list of the main pass supplies all 32
  _placed(cuda, rows, queries, list(range(lo + per - 16, lo + per + 16)), 32)       # ... or two neighbours, half each
  _placed(cuda, rows, queries, list(range(first - 32, first)), 32)                  # ... or the prefix alone: nothing behind it passes its floor
  _placed(cuda, rows, queries, list(range(first - 16, first + 16)), 32)             # ... or both sides of the seam
  small = _index(rows[:4099], cuda)
  assert small.slabs()[0] == 0                                                      # no prefix below 16384 rows
  _, nl, pr = small.slabs()
  _placed(cuda, rows[:4099], queries, list(range(5 * pr, 5 * pr + 32)), 32)


def test_placed_maxima_one_per_slab(cuda, placed_base):
  rows, queries = placed_base
  ix = _index(rows, cuda)
  first, nlists, per = ix.slabs()
  step = nlists // 32
  where = [first + (j * step) * per + (5 * j) % per for j in range(32)]
  assert max(where) < 70001 and len(set((w - first) // per for w in where)) == 32
  _placed(cuda, rows, queries, where, 32)
  _placed(cuda, rows, queries, where[:10], 3)
  _placed(cuda, rows, queries, [7] + where[:31], 32)                                 # one of them in the prefix


def test_exclusions_are_a_penalty_not_a_removal(cuda):
  rows, queries = U.exact_inputs(4099, 64, 3, seed=21)
  ix = _index(rows, cuda)
  S, _ = U.penalised_scores(rows, queries)
  s0, i0 = _search(ix, queries, 3, normalize=False)
  assert U.exact_equal(s0, i0, S, 3)
  # the current top 3 of every query, as a tensor
  ex = i0.clone()
  s1, i1 = _search(ix, queries, 3, normalize=False, exclude=ex.to(cuda), penalty=1000.0)
  S1, _ = U.penalised_scores(rows, queries, ex.tolist(), 1000.0)
  assert U.exact_equal(s1, i1, S1, 3) and not bool((i1 == i0).all())
  # lists that differ per query, with empty slots; one query with none
  lists = [[int(i0[0, 0]), int(i0[0, 2])], [], [int(i0[2, 1]), 4098, 0]]
  s2, i2 = _search(ix, queries, 16, normalize=False, exclude=lists, penalty=1000.0)
  S2, _ = U.penalised_scores(rows, queries, lists, 1000.0)
  assert U.exact_equal(s2, i2, S2, 16)
  assert torch.equal(i2[1, :3], i0[1]) and int(i0[0, 0]) not in i2[0].tolist()
  # a small penalty keeps the row in the list, behind the rows that tied with it, reported with the penalty
  s3, i3 = _search(ix, queries[:1], 32, normalize=False, exclude=[[int(i0[0, 0])]], penalty=0.5)
  S3, _ = U.penalised_scores(rows, queries[:1], [[int(i0[0, 0])]], 0.5)
  assert U.exact_equal(s3, i3, S3, 32) and int(i0[0, 0]) in i3[0].tolist()
  # k = N over a tiny index: the penalised rows go last
  tiny = _index(rows[:5], cuda)
  s4, i4 = _search(tiny, queries, 8, normalize=False, exclude=[[0], [1, 2], [-1]], penalty=1000.0)
  S4, _ = U.penalised_scores(rows[:5], queries, [[0], [1, 2], [-1]], 1000.0)
  assert U.exact_equal(s4, i4, S4, 8) and i4[0, 4].item() == 0 and i4[:, 5:].eq(-1).all()
  # penalty 0 and all-empty lists change nothing
  s5, i5 = _search(ix, queries, 3, normalize=False, exclude=ex.to(cuda), penalty=0.0)
  s6, i6 = _search(ix, queries, 3, normalize=False, exclude=torch.full((3, 64), -1, dtype=torch.int64))
  assert torch.equal(s5, s0) and torch.equal(i5, i0) and torch.equal(s6, s0) and torch.equal(i6, i0)


@pytest.fixture(scope="module")
def real_rig():
  g = torch.Generator().manual_seed(77)
  raw = torch.randn((70001, 256), generator=g)
  raw[123] = 0.0                                         # a zero row stays zero
  queries = torch.randn((5, 256), generator=g)
  scale = math.exp(2.5)
  return raw, queries, scale, U.normalized_rows(raw, scale)


def test_add_normalises_within_one_bf16_ulp_and_rows_round_trip(cuda, real_rig):
  raw, queries, scale, want = real_rig
  ix = _index(raw, cuda, normalize=True, scale=scale)
  got = ix.rows(0, 70001).cpu().double()
  err = (got - want).abs()
  worst = (err / want.abs().clamp_min(1e-300)).max().item()
  print(f"[add] worst |stored - fp64| / |fp64| = {worst:.3e} (bar 2^-8 = {2.0 ** -8:.3e})")
  assert bool((err <= 2.0 ** -8 * want.abs()).all()), worst
  assert bool((got[123] == 0).all()) and bool(torch.isfinite(got).all())
  norms = got.norm(dim=1)
  assert abs(norms[0].item() - scale) < 0.02 * scale
  # pieces of the layout: any window reads back what the whole read gave
  for first, n in ((0, 1), (15, 2), (16, 16), (69990, 11), (4097, 333)):
    assert torch.equal(ix.rows(first, n).cpu().double(), got[first:first + n]), (first, n)
  # fp16 input of representable values: the same arithmetic
  ix16 = _index(raw[:64].half().float(), cuda, normalize=True, scale=scale)
  ixh = _index(raw[:64].half(), cuda, dtype=torch.float16, normalize=True, scale=scale)
  assert torch.equal(ix16.rows(0, 64), ixh.rows(0, 64))


def test_real_valued_search_under_the_derived_bound(cuda, real_rig):
  raw, queries, scale, want = real_rig
  ix = _index(raw, cuda, normalize=True, scale=scale)
  stored = ix.rows(0, 70001).cpu().double()
  for normalize, qs in ((True, U.normalized_queries(queries)), (False, U.bf16_round(queries))):
    for k in (10, 32):
      scores, idx = _search(ix, queries, k, normalize=normalize)
      S, mag = U.penalised_scores(stored, qs)
      b = U.bound(mag, 256, normalize)
      ok, why = U.accept(scores, idx, S, b)
      ii = idx.clamp_min(0)
      rel = ((scores.double() - torch.gather(S, 1, ii)).abs() / torch.gather(b, 1, ii).clamp_min(1e-300)).max().item()
      print(f"[search] normalize={normalize} k={k}: worst |score - fp64| / bound = {rel:.3e}")
      assert ok, why
  # two searches on one handle: the same bits
  a = _search(ix, queries, 10, normalize=True)
  b2 = _search(ix, queries, 10, normalize=True)
  assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1])
  # a zero query under normalize: every score 0, the lowest indices
  z = _search(ix, torch.zeros(1, 256), 3, normalize=True)
  assert z[1].tolist() == [[0, 1, 2]] and z[0].tolist() == [[0.0, 0.0, 0.0]]


def test_chunked_adds_equal_one_add(cuda, real_rig):
  raw, queries, scale, want = real_rig
  from gill_amd.retrieval import GillRetrievalIndex
  whole = _index(raw[:4099], cuda, normalize=True, scale=scale, capacity=5000)
  parts = GillRetrievalIndex(256, 5000, cuda)
  lo = 0
  for n in (7, 16, 4076):
    parts.add(raw[lo:lo + n].to(cuda), normalize=True, scale=scale)      # device input
    lo += n
  assert len(parts) == 4099 == len(whole)
  assert torch.equal(parts.rows(0, 4099), whole.rows(0, 4099))
  a, b = _search(whole, queries, 16, normalize=True), _search(parts, queries, 16, normalize=True)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  with pytest.raises(ValueError):
    parts.add(raw[:902], normalize=True)
  # numpy input, and the classmethod
  fe = GillRetrievalIndex.from_embeddings(raw[:4099].numpy(), scale=scale, normalize=True, device=cuda)
  assert torch.equal(fe.rows(0, 4099), whole.rows(0, 4099))
