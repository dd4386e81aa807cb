"""Dialogue sessions: every row of a batch is one multi-turn dialogue whose KV cache stays in the OPT handle across turns.

generate_batch starts from nothing at every call: the caller sends the whole history again, every image goes through the CLIP tower again and
every history token through all decoder layers again.  A session keeps, per row, the history (token ids, negative ids for visual rows, and the
row's bf16 visual rows), the number of tokens whose keys / values the cache holds, and feeds only what is new: gill_opt_extend runs the layers
over the packed new tokens of all rows at per-row cache lengths (csrc/attention_extend.hip), the ragged loop of generate_batch then decodes.

Invariant (include/gill_amd.h, the ragged decode state): after a decode loop a row's state len is the position of its newest token, whose key /
value may or may not have been stored.  So the cache counts as valid on [0, len(history) - 1) and the newest token is PENDING: the next extend
feeds [pending token | new tokens] at that length.  Slots beyond a row's cached length are never selected, whatever they hold: a rollback only
lowers the length, and an idle row's slot `cached` may be scribbled on by the other rows' decode steps without harm (which is why a row
may fill at most capacity - 1 slots).

The bookkeeping (RowBook, pack_feed, check_epoch) is plain host code that runs without a GPU; DialogueSession puts it on a GILLModel."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import _native as N


class StaleSessionError(RuntimeError):
  """The handle's KV cache was written or rebuilt by another entry since the session last used it."""


def check_epoch(session_epoch: int, model_epoch: int) -> None:
  if session_epoch != model_epoch:
    raise StaleSessionError(f'dialogue session is stale: the OPT handle\'s KV cache was written or rebuilt by another entry (generate, '
                            f'generate_batch, a cached forward, a handle rebuild, quantize_lm or quantize_kv) since the session used it '
                            f'(epoch {model_epoch}, the session holds {session_epoch}); open a new session.')


class RowBook:
  """One dialogue's host-side state.  ids: the history, an id < 0 selecting row -(id + 1) of the row's own visual rows (n_extra of them);
  cached: the tokens [0, cached) have their keys / values in the cache; ids[cached:] are pending (fed by the next extend); turn_start: where
  the last generate's tokens begin; ready: the row's hidden_last is that of ids[-1] (an extend ran and nothing changed since)."""

  def __init__(self):
    self.reset()

  def reset(self) -> None:
    self.ids: List[int] = []
    self.n_extra = 0
    self.cached = 0
    self.turn_start = 0
    self.ready = False

  def append(self, new_ids: Sequence[int], n_new_extra: int = 0) -> None:
    """A turn's new tokens; their negative ids count from the turn's own first visual row: -(j + 1) is its j-th, j < n_new_extra."""
    new_ids = [int(v) for v in new_ids]
    for v in new_ids:
      if v < -n_new_extra:
        raise ValueError(f'id {v} selects visual row {-(v + 1)} of {n_new_extra}')
    self.ids += [v - self.n_extra if v < 0 else v for v in new_ids]
    self.n_extra += int(n_new_extra)
    self.turn_start = len(self.ids)
    self.ready = False

  def feed(self) -> List[int]:
    """What the next extend runs through the layers: [pending token(s) | new tokens]."""
    return self.ids[self.cached:]

  def fed(self) -> None:
    self.cached = len(self.ids)
    self.ready = True

  def generated(self, tokens: Sequence[int]) -> None:
    """The tokens a decode loop emitted: the newest one stays pending (its key / value may not have been stored)."""
    tokens = [int(v) for v in tokens]
    self.turn_start = len(self.ids)
    self.ids += tokens
    if tokens:
      self.cached = len(self.ids) - 1
    self.ready = False

  def rollback(self, keep: int) -> None:
    """Keep only the first `keep` tokens of the last generate.  Lowers the length and the history, nothing else; the newest kept token becomes
    pending again, so that a following extend (even without new tokens) has a row to run."""
    n_gen = len(self.ids) - self.turn_start
    if not 0 <= keep <= n_gen:
      raise ValueError(f'rollback keeps 0 .. {n_gen} tokens of the last turn, got {keep}')
    del self.ids[self.turn_start + keep:]
    self.cached = min(self.cached, max(len(self.ids) - 1, 0))
    self.ready = False


def pack_feed(feeds: Sequence[Sequence[int]], extra_offsets: Sequence[int]) -> Tuple[List[int], List[int], int]:
  """The rows' feeds (one list per row of the batch, empty for a row that brings nothing) -> (packed ids, cu_new (B + 1 prefix sums), max_new).
  A negative id of row b is moved by extra_offsets[b]: row -(id + 1) of the row's own visual rows is row extra_offsets[b] - (id + 1) of the
  call's table."""
  packed: List[int] = []
  cu = [0]
  for f, off in zip(feeds, extra_offsets):
    packed += [int(v) - off if v < 0 else int(v) for v in f]
    cu.append(len(packed))
  return packed, cu, max((b - a for a, b in zip(cu, cu[1:])), default=0)


class CandidatePack:
  """One gill_opt_score_candidates call's worth of packed candidates (pack_candidates): ids / targets (total_new), cu_new (C + 1), parent and
  plen (C), the host bounds max_new and len_bound, and per candidate `own` = (index into the caller's rows, index of the candidate in that row,
  packed row of its first own token's predictor, number of own tokens scored)."""

  def __init__(self):
    self.ids: List[int] = []
    self.targets: List[int] = []
    self.cu: List[int] = [0]
    self.parent: List[int] = []
    self.plen: List[int] = []
    self.own: List[Tuple[int, int, int, int]] = []
    self.max_new = 0
    self.len_bound = 0

  @property
  def n_candidates(self) -> int:
    return len(self.parent)

  @property
  def total_new(self) -> int:
    return len(self.ids)


def pack_candidates(rows: Sequence[Tuple[int, Sequence[int], int, int]], candidates: Sequence[Sequence[Sequence[int]]],
                    limit: Optional[int] = None) -> List[CandidatePack]:
  """The packing of DialogueSession.score, pure host code.  rows: per scored row (cache row index, history ids, cached, extra offset);
  candidates: per scored row its candidate token-id sequences (ids >= 0: text only).  For a row with history `ids` whose cache holds `cached`
  tokens, plen = max(min(cached, len(ids) - 1), 0): the last history token is always re-run, as the predictor of cand[0], whether the row is
  fresh from extend (cached == len(ids)) or carries a pending token.  A candidate's feed is ids[plen:] + cand[:-1]; its targets are -100 for
  all but the last history position of the feed, then cand.  With an empty history cand[0] has no predictor: the feed is cand[:-1] and the
  targets are cand[1:] (a one-token candidate then scores nothing).  An empty candidate brings no rows and scores nothing.  A negative history
  id is moved by the row's extra offset, as in pack_feed.  Candidates stay grouped by row, in the order given.  limit: the most packed rows one
  call may carry (the handle's workspace); the candidates are split into as many packs as that takes, none of them split itself."""
  if len(rows) != len(candidates):
    raise ValueError(f'score needs one candidate list per named row ({len(rows)}), got {len(candidates)}')
  packs = [CandidatePack()]
  for k, ((parent, ids, cached, off), cands) in enumerate(zip(rows, candidates)):
    ids = [int(v) for v in ids]
    plen = max(min(int(cached), len(ids) - 1), 0)
    tail = [v - off if v < 0 else v for v in ids[plen:]]
    for j, cand in enumerate(cands):
      cand = [int(v) for v in cand]
      if any(v < 0 for v in cand):
        raise NotImplementedError(f'row {parent} candidate {j}: candidates are text only (ids >= 0); images inside a candidate are not scored')
      if not cand:
        feed, tgt, first, n_own = [], [], 0, 0
      elif tail:
        feed, tgt, first, n_own = tail + cand[:-1], [-100] * (len(tail) - 1) + cand, len(tail) - 1, len(cand)
      else:
        feed, tgt, first, n_own = cand[:-1], cand[1:], 0, len(cand) - 1
      if limit is not None and len(feed) > limit:
        raise ValueError(f'row {parent} candidate {j}: {len(feed)} packed tokens exceed the handle\'s workspace ({limit})')
      p = packs[-1]
      if limit is not None and p.total_new + len(feed) > limit:
        p = CandidatePack()
        packs.append(p)
      p.own.append((k, j, p.total_new + first, n_own))
      p.ids += feed
      p.targets += tgt
      p.cu.append(len(p.ids))
      p.parent.append(int(parent))
      p.plen.append(plen)
      p.max_new = max(p.max_new, len(feed))
      p.len_bound = max(p.len_bound, plen + len(feed))
  return [p for p in packs if p.n_candidates]


BRANCH_GROUP = 32      # siblings per group of gill_attention_branch: the query lanes of one MFMA tile


def pack_branches(rows: Sequence[int], n: int, lengths: Sequence[int]):
  """The packing of DialogueSession.sample, pure host code.  rows: the cache rows of the sampled dialogues; n: branches per dialogue; lengths:
  per dialogue the visible length of its cache row (len(history)).  Branches are ordered by dialogue (branch k * n + j is number j of rows[k])
  and a dialogue's branches are cut into groups of at most BRANCH_GROUP.  -> (gstart (G + 1), gparent (G), gplen (G), [(row, index)] per
  branch)."""
  n = int(n)
  if n < 1:
    raise ValueError(f'n should be at least 1, got {n}')
  if len(rows) != len(lengths):
    raise ValueError(f'pack_branches needs one length per row ({len(rows)}), got {len(lengths)}')
  gstart, gparent, gplen, own = [0], [], [], []
  for r, ln in zip(rows, lengths):
    for j0 in range(0, n, BRANCH_GROUP):
      cnt = min(BRANCH_GROUP, n - j0)
      own += [(int(r), j0 + j) for j in range(cnt)]
      gstart.append(len(own))
      gparent.append(int(r))
      gplen.append(int(ln))
  return gstart, gparent, gplen, own


class BranchSet:
  """What DialogueSession.sample returns: tokens (S, L) int64 on the device, padded with -1; n_tokens (S,) on the host; row (S,) the dialogue
  each branch belongs to and index (S,) its number within that dialogue.  The branches' keys / values live in the handle's branch cache until
  the next sample: adopt() is valid only while the set is current."""

  def __init__(self, tokens, n_tokens, row, index, plen, serial):
    self.tokens, self.n_tokens, self.row, self.index = tokens, n_tokens, row, index
    self._plen, self._serial = plen, serial         # per branch its dialogue's length at sample time; the session's write serial
    self._adopted = set()

  def find(self, row: int, index: int) -> int:
    for s, (r, j) in enumerate(zip(self.row, self.index)):
      if r == int(row) and j == int(index):
        return s
    raise ValueError(f'the branch set holds no branch {index} of row {row}')

  def reply(self, row: int, index: int) -> List[int]:
    s = self.find(row, index)
    return [int(v) for v in self.tokens[s, :int(self.n_tokens[s])].tolist()]


def rank_order(scores: torch.Tensor) -> dict:
  """(n,) scores -> dict(scores, order: indices from the highest score down, ties in index order, NaN last; best: order[0] or None)."""
  sc = [float(v) for v in scores.tolist()]
  order = sorted(range(len(sc)), key=lambda j: (sc[j] != sc[j], -sc[j] if sc[j] == sc[j] else 0.0, j))
  return dict(scores=scores, order=order, best=order[0] if order and sc[order[0]] == sc[order[0]] else None)


class DialogueSession:
  """GILLModel.open_session(B, capacity): B dialogues over the handle's KV cache, each of at most capacity - 1 tokens (one slot of a row is
  kept free for the decode step's store).  The handle is sized once; any other entry that writes or rebuilds its cache makes the session stale
  (StaleSessionError) instead of letting it read a cache that is no longer its own."""

  def __init__(self, model, B: int, capacity: int):
    B, capacity = int(B), int(capacity)
    if B < 1 or capacity < 2:
      raise ValueError(f'open_session needs B >= 1 and capacity >= 2, got {B}, {capacity}')
    if capacity > model.opt_cfg.max_positions:
      raise ValueError(f'capacity {capacity} exceeds the position table ({model.opt_cfg.max_positions})')
    self.model, self.B, self.capacity = model, B, capacity
    self.handle = model._opt_native(B, capacity)
    model._cache_epoch += 1       # the cache now belongs to this session: an earlier one over the same handle goes stale
    self.epoch = model._cache_epoch
    self.books = [RowBook() for _ in range(B)]
    self.extras: List[Optional[torch.Tensor]] = [None] * B      # per row (n_extra, D) bf16
    dev = model.logit_scale.device
    self.hidden_last = torch.zeros((B, 1, model.opt_cfg.hidden_size), device=dev, dtype=torch.float32)
    self._serial = 0      # counts the calls that write the cache or change a book: a BranchSet is current while it stands (sample, adopt)

  def _check(self) -> None:
    check_epoch(self.epoch, self.model._cache_epoch)

  def _rows(self, rows) -> List[int]:
    rows = list(range(self.B)) if rows is None else [int(r) for r in rows]
    if len(set(rows)) != len(rows) or any(not 0 <= r < self.B for r in rows):
      raise ValueError(f'rows should be distinct indices below {self.B}, got {rows}')
    return rows

  def extend(self, rows, ids=None, embeddings=None, extra_rows=None) -> None:
    """Appends each named row's new tokens to its history and runs [pending token | new tokens] of every named row through the layers at the
    row's cached length (gill_opt_extend, one packed call).  ids: per named row a sequence of token ids (an id < 0 selects row -(id + 1) of
    that row's entry of extra_rows, (n, D) bf16 or None: the visual rows of the turn's images).  embeddings: not kept by a session (its
    history is ids and visual rows); pass visual rows through extra_rows."""
    self._check()
    if embeddings is not None:
      raise NotImplementedError('a session keeps token ids and visual rows: pass ids (negative ids for the rows of extra_rows), not embeddings')
    rows = self._rows(rows)
    self._serial += 1
    if ids is None or len(ids) != len(rows):
      raise ValueError(f'extend needs one id sequence per named row ({len(rows)})')
    extra_rows = [None] * len(rows) if extra_rows is None else list(extra_rows)
    if len(extra_rows) != len(rows):
      raise ValueError(f'extra_rows needs one entry per named row ({len(rows)})')
    m = self.model
    dev, D = m.logit_scale.device, m.opt_cfg.hidden_size
    new = []
    for r, row_ids, ex in zip(rows, ids, extra_rows):
      row_ids = [int(v) for v in torch.as_tensor(row_ids).reshape(-1).tolist()]
      n_ex = 0
      if ex is not None:
        if ex.dim() != 2 or ex.shape[1] != D or ex.dtype != torch.bfloat16:
          raise ValueError(f'extra_rows must be (n, {D}) bfloat16, got {tuple(ex.shape)} {ex.dtype}')
        n_ex = int(ex.shape[0])
      if any(v < -n_ex for v in row_ids):
        raise ValueError(f'row {r}: id {min(row_ids)} selects visual row {-(min(row_ids) + 1)} of {n_ex}')
      bk = self.books[r]
      if len(bk.ids) + len(row_ids) > self.capacity - 1:
        raise ValueError(f'row {r}: {len(bk.ids)} + {len(row_ids)} tokens exceed the session\'s capacity - 1 = {self.capacity - 1}')
      if len(bk.ids) + len(row_ids) == 0:
        raise ValueError(f'row {r}: an empty dialogue needs at least one token')
      new.append((r, row_ids, ex, n_ex))
    for r, row_ids, ex, n_ex in new:
      self.books[r].append(row_ids, n_ex)
      if n_ex:
        ex = ex.to(dev).contiguous()
        self.extras[r] = ex if self.extras[r] is None else torch.cat([self.extras[r], ex], dim=0)
    # the call's table of visual rows: the rows of every named row whose feed selects one
    feeds, offsets, tables, n_tab = [[] for _ in range(self.B)], [0] * self.B, [], 0
    for r in rows:
      feeds[r] = self.books[r].feed()
      if any(v < 0 for v in feeds[r]):
        offsets[r] = n_tab
        tables.append(self.extras[r])
        n_tab += int(self.extras[r].shape[0])
    packed, cu, max_new = pack_feed(feeds, offsets)
    lens = [bk.cached for bk in self.books]
    len_bound = max(len(self.books[r].ids) for r in rows)
    with torch.no_grad():
      m._lm_extend(torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev), self.B, len(packed),
                   max_new, len_bound, self.hidden_last, ids=torch.tensor(packed, dtype=torch.int64, device=dev),
                   extra_rows=torch.cat(tables, dim=0) if tables else None)
    for r in rows:
      self.books[r].fed()

  def generate(self, rows=None, max_len: int = 32, temperature: float = 0.0, top_p: float = 1.0, min_word_tokens: int = 0,
               ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0, filter_value: float = -float('Inf'),
               seed: Optional[int] = None, row_ids=None):
    """Decodes the named rows (default: all) from the hidden rows their extend left, with generate_batch's loop, arguments and results
    (tokens (B, L) padded with -1, n_tokens (B,), hidden (B, L, D), n_hidden (B,), B the session's rows); the other rows are idle: no
    decision, state untouched, cache intact, n_tokens 0.  row_ids: the Philox row ids of ALL B rows (default 0 .. B - 1)."""
    self._check()
    rows = self._rows(rows)
    self._serial += 1
    m, B = self.model, self.B
    for r in rows:
      if not self.books[r].ready:
        raise RuntimeError(f'row {r} has nothing to decode from: extend it first (after a turn, a rollback or a reset)')
    if temperature == 0.0 and top_p != 1.0:
      raise ValueError('top_p cannot be set if temperature is 0 (greedy decoding).')
    if temperature != 0.0:
      if seed is None:
        raise ValueError('a session draws on the device only: temperature > 0 needs seed.')
      seed = int(seed)
      if not 0 <= seed < 2 ** 64:
        raise ValueError(f'seed should be in [0, 2**64), got {seed} instead.')
      assert top_p > 0, f'top_p should be above 0, got {top_p} instead.'
    max_len = int(max_len)
    n_ret = max(1, len(m.retrieval_token_idx))
    L = max_len * n_ret
    longest = max(len(self.books[r].ids) for r in rows) if rows else 0
    if longest + L > self.capacity:
      raise ValueError(f'{longest} tokens + max_len * {n_ret} = {longest + L} exceed the session\'s capacity ({self.capacity}).')
    keys = list(range(B)) if row_ids is None else [int(v) for v in torch.as_tensor(row_ids).reshape(-1).tolist()]
    if len(keys) != B or min(keys) < 0:
      raise ValueError(f'row_ids should be {B} integers >= 0.')
    dev = m.logit_scale.device
    D, vocab = m.opt_cfg.hidden_size, m.opt_cfg.vocab_size
    active = set(rows)
    with torch.no_grad():
      st = torch.zeros(6 * B + 1, dtype=torch.int32)
      for b, bk in enumerate(self.books):
        # an active row: its newest token's position; an idle one: its first free slot (never selected), all its decisions taken
        st[b] = len(bk.ids) - 1 if b in active else bk.cached
        st[B + b] = 0 if b in active else max_len
      st[4 * B:5 * B] = torch.tensor(keys, dtype=torch.int32)
      st[6 * B] = len(rows) if max_len > 0 else 0
      # host bounds of the decode step's lengths: the deciding rows grow by one per iteration, the idle rows stand
      len0 = max((len(self.books[b].ids) for b in active), default=1)
      len_floor = max((self.books[b].cached + 1 for b in range(B) if b not in active), default=0)
      st = st.to(dev)
      tokens = torch.full((B, max(L, 1)), -1, device=dev, dtype=torch.int64)
      hid = self.hidden_last[:, 0].contiguous()
      steps = torch.zeros((max(L, 1), B, D), device=dev, dtype=torch.float32)
      nxt = torch.zeros((B, D), device=dev, dtype=torch.bfloat16)
      logits = torch.empty((B, vocab), device=dev, dtype=torch.float32)
      rule = m._decode_rule(0, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value)
      sampler = None
      if temperature != 0.0:
        sampler = N.gill_decode_sampler()
        sampler.temperature, sampler.top_p, sampler.seed = float(temperature), min(float(top_p), 1.0), seed
      m._decode_host_waits = 0
      m._ragged_decode_loop(self.handle, B, st, hid, steps, nxt, logits, tokens, rule, sampler, max_len, L, len0, len_floor)
      n_tokens, n_hidden, hidden = m._ragged_results(B, st, tokens, steps, L, n_ret)
      toks = tokens.cpu()
      for r in rows:
        self.books[r].generated(toks[r, :int(n_tokens[r])].tolist())
    return tokens[:, :L], n_tokens.to(dev), hidden, n_hidden.to(dev)

  def score(self, rows, candidates, reduce: str = 'mean', return_tokens: bool = False, max_packed: Optional[int] = None):
    """Log-likelihood of candidate continuations of the named rows' dialogues: candidates[k] is a list of token-id sequences (text only) for
    rows[k].  The rows' cached prefixes are read where they lie and shared by all their candidates (gill_opt_score_candidates over
    csrc/attention_fork.hip): only each row's last history token (plus what is still pending) and the candidates' own tokens run through
    the layers, and nothing is appended.  Returns per named row a host fp32 tensor (n_candidates,): the sum or the mean (reduce) of the
    candidate's own tokens' log-probabilities (the mean of a candidate with nothing scored is NaN, its sum 0); with return_tokens also, per
    named row, the list of the candidates' per-token log-probabilities.  Unlike GILL.get_log_likelihood_scores the history's own tokens are
    not part of the score.  One device-to-host copy per call of the engine (one call unless the packed rows exceed the handle's workspace, or
    max_packed).  The session is untouched: books, hidden_last, cache and epoch stay as they are."""
    self._check()
    if reduce not in ('mean', 'sum'):
      raise ValueError(f"reduce should be 'mean' or 'sum', got {reduce!r}")
    rows = self._rows(rows)
    if candidates is None or len(candidates) != len(rows):
      raise ValueError(f'score needs one candidate list per named row ({len(rows)})')
    m = self.model
    dev = m.logit_scale.device
    offsets, tables, n_tab = [0] * len(rows), [], 0
    for k, r in enumerate(rows):
      bk = self.books[r]
      if any(v < 0 for v in bk.ids[max(min(bk.cached, len(bk.ids) - 1), 0):]):
        offsets[k] = n_tab
        tables.append(self.extras[r])
        n_tab += int(self.extras[r].shape[0])
    cb, ct = m._opt_cap
    limit = cb * ct if max_packed is None else min(int(max_packed), cb * ct)
    packs = pack_candidates([(r, self.books[r].ids, self.books[r].cached, offsets[k]) for k, r in enumerate(rows)], candidates, limit)
    for p in packs:
      if p.len_bound > m.opt_cfg.max_positions:
        raise ValueError(f'a history plus its candidate holds {p.len_bound} tokens: beyond the position table ({m.opt_cfg.max_positions})')
    scores = [torch.full((len(c),), float('nan') if reduce == 'mean' else 0.0, dtype=torch.float32) for c in candidates]
    tokens = [[torch.zeros(0)] * len(c) for c in candidates]
    extra = torch.cat(tables, dim=0) if tables else None
    with torch.no_grad():
      for p in packs:
        if p.total_new == 0:
          continue
        out = m._lm_score_candidates(p, extra_rows=extra).cpu()      # the one copy of this call
        T, C = p.total_new, p.n_candidates
        pick = out[T:T + C] if reduce == 'sum' else out[T + C:T + 2 * C]
        for c, (k, j, first, n_own) in enumerate(p.own):
          scores[k][j] = pick[c]
          tokens[k][j] = out[first:first + n_own].clone()
    return (scores, tokens) if return_tokens else scores

  def sample(self, rows, n: int, max_len: int = 32, temperature: float = 0.0, top_p: float = 1.0, seed: Optional[int] = None,
             min_word_tokens: int = 0, ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0, filter_value: float = -float('Inf'),
             keys=None) -> BranchSet:
    """Draws n replies per named row from the row's cached history: S = len(rows) * n branches decode together, the siblings of a row sharing
    its prefix where it lies (gill_opt_decode_step_branch over csrc/attention_branch.hip: the prefix is read once per group of up to 32
    siblings, head and step; every branch keeps its own tokens in the handle's branch cache, reserved here for S branches of
    max_len * len(retrieval_token_idx) + 1 tokens).  Every named row must be ready (extend ran); the first decision of all n branches of a row
    reads that row's hidden_last.  temperature > 0 needs seed; branch j of row r draws with the Philox key (seed, keys[k * n + j], its decision
    count), keys defaulting to r * n + j, so it draws what generate_batch(row_ids=[key]) draws from the same history.  n > 1 with
    temperature == 0 is refused: all branches would be equal.  Returns a BranchSet.  The session is untouched: books, hidden_last, main cache
    and epoch stay as they are; an e4m3 handle raises, naming the format."""
    self._check()
    rows = self._rows(rows)
    m = self.model
    n = int(n)
    if n < 1 or not rows:
      raise ValueError(f'sample needs at least one row and n >= 1, got {len(rows)} rows, n = {n}')
    for r in rows:
      if not self.books[r].ready:
        raise RuntimeError(f'row {r} has nothing to decode from: extend it first (after a turn, a rollback or a reset)')
    if temperature == 0.0 and top_p != 1.0:
      raise ValueError('top_p cannot be set if temperature is 0 (greedy decoding).')
    if temperature == 0.0 and n > 1:
      raise ValueError(f'n = {n} branches with temperature 0 would all be equal: sample with temperature > 0 and a seed.')
    if temperature != 0.0:
      if seed is None:
        raise ValueError('a session draws on the device only: temperature > 0 needs seed.')
      seed = int(seed)
      if not 0 <= seed < 2 ** 64:
        raise ValueError(f'seed should be in [0, 2**64), got {seed} instead.')
      assert top_p > 0, f'top_p should be above 0, got {top_p} instead.'
    max_len = int(max_len)
    n_ret = max(1, len(m.retrieval_token_idx))
    L = max_len * n_ret
    lengths = [len(self.books[r].ids) for r in rows]
    if max(lengths) + L > m.opt_cfg.max_positions:
      raise ValueError(f'{max(lengths)} tokens + max_len * {n_ret} = {max(lengths) + L} exceed the position table ({m.opt_cfg.max_positions}).')
    S = len(rows) * n
    keys = [r * n + j for r in rows for j in range(n)] if keys is None else [int(v) for v in torch.as_tensor(keys).reshape(-1).tolist()]
    if len(keys) != S or min(keys) < 0:
      raise ValueError(f'keys should be {S} integers >= 0 (one per branch, ordered by row).')
    gstart, gparent, gplen, own = pack_branches(rows, n, lengths)
    G = len(gparent)
    dev = m.logit_scale.device
    D, vocab = m.opt_cfg.hidden_size, m.opt_cfg.vocab_size
    with torch.no_grad(), torch.cuda.device(dev):
      N.check(N.lib().gill_opt_branch_reserve(self.handle, S, L + 1))      # an e4m3 handle: the engine's error names the format
      self._serial += 1           # the branch cache is about to be rewritten: an earlier BranchSet is no longer current
      st = torch.zeros(6 * S + 1, dtype=torch.int32)
      st[:S] = torch.tensor([lengths[k] - 1 for k in range(len(rows)) for _ in range(n)], dtype=torch.int32)     # the newest token's position
      st[4 * S:5 * S] = torch.tensor(keys, dtype=torch.int32)
      st[6 * S] = S if max_len > 0 else 0
      st = st.to(dev)
      groups = torch.tensor(gstart + gparent + gplen, dtype=torch.int32).to(dev)
      tokens = torch.full((S, max(L, 1)), -1, device=dev, dtype=torch.int64)
      hid = self.hidden_last[rows, 0].repeat_interleave(n, dim=0).contiguous()        # a copy: hidden_last itself is never written
      steps = torch.zeros((max(L, 1), S, D), device=dev, dtype=torch.float32)
      nxt = torch.zeros((S, D), device=dev, dtype=torch.bfloat16)
      logits = torch.empty((S, vocab), device=dev, dtype=torch.float32)
      rule = m._decode_rule(0, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value)
      sampler = None
      if temperature != 0.0:
        sampler = N.gill_decode_sampler()
        sampler.temperature, sampler.top_p, sampler.seed = float(temperature), min(float(top_p), 1.0), seed
      m._decode_host_waits = 0
      m._branch_decode_loop(self.handle, S, G, groups, st, hid, steps, nxt, logits, tokens, rule, sampler, max_len, L, max(lengths))
      n_tokens, _, _ = m._ragged_results(S, st, tokens, steps, L, n_ret)
    return BranchSet(tokens[:, :L], n_tokens, [r for r, _ in own], [j for _, j in own], [lengths[rows.index(r)] for r, _ in own], self._serial)

  def adopt(self, branch_set: BranchSet, row: int, index: int, keep: Optional[int] = None) -> None:
    """Makes branch `index` of `row` the row's last turn: the first `keep` tokens of that reply (default: all) join the history, the keys /
    values of all but the newest of them are copied from the branch cache into the row (gill_opt_branch_adopt; the newest token stays pending,
    as after a generate).  rollback, extend, generate and score then behave as after a generate that had emitted those tokens.  Valid only
    while the set is current: no later sample and no extend, generate, rollback or reset since, and one adopt per row."""
    self._check()
    r = self._rows([row])[0]
    s = branch_set.find(r, index)
    bk = self.books[r]
    if branch_set._serial != self._serial or r in branch_set._adopted or len(bk.ids) != branch_set._plen[s]:
      raise RuntimeError(f'the branch set is no longer current for row {r}: a later sample, extend, generate, rollback, reset or adopt changed the '
                         f'branch cache or the row since it was drawn; sample again.')
    nt = int(branch_set.n_tokens[s])
    keep = nt if keep is None else int(keep)
    if not 0 <= keep <= nt:
      raise ValueError(f'adopt keeps 0 .. {nt} tokens of the reply, got {keep}')
    plen = len(bk.ids)
    if plen + keep > self.capacity - 1:
      raise ValueError(f'row {r}: {plen} + {keep} tokens exceed the session\'s capacity - 1 = {self.capacity - 1}')
    toks = branch_set.tokens[s, :keep].tolist()
    if keep > 1:
      with torch.cuda.device(self.model.logit_scale.device):
        N.check(N.lib().gill_opt_branch_adopt(self.handle, s, r, plen, keep - 1, N.current_stream()))
    branch_set._adopted.add(r)
    bk.generated(toks)

  def rollback(self, row: int, keep: int) -> None:
    """Keeps only the first `keep` generated tokens of the row's last turn.  Costs nothing on the device."""
    self._check()
    self._serial += 1
    self.books[self._rows([row])[0]].rollback(int(keep))

  def reset(self, rows) -> None:
    """Empties the rows: new dialogues can start in them while the others go on."""
    self._check()
    self._serial += 1
    for r in self._rows(rows):
      self.books[r].reset()
      self.extras[r] = None

  def history(self, row: int):
    """(ids (n,) int64, extra_rows (n_extra, D) bf16 or None) of the row, such that generate_batch(ids=ids[None], lengths=[n],
    extra_rows=extra_rows) from scratch reproduces it."""
    r = self._rows([row])[0]
    return torch.tensor(self.books[r].ids, dtype=torch.int64), self.extras[r]


def segment_turn(tokenizer, prompt, n_visual_tokens: int, bos_done: bool, always_add_bos: bool, is_image):
  """One turn's prompt list (images and strings) -> (ids, images, bos_done), segmented as GILL._interleaved_ids segments a prompt: strings are
  tokenised, <bos> on the dialogue's first string only (bos_done: an earlier turn already had it; always_add_bos: on every string), and the
  turn's image number j takes n_visual_tokens slots with the ids -(j * n_visual_tokens + t + 1): rows of the turn's own visual rows."""
  ids: List[int] = []
  images = []
  for seg in prompt:
    if type(seg) == str:
      add_bos = always_add_bos or not bos_done
      ids += [int(v) for v in tokenizer(seg, add_special_tokens=add_bos, return_tensors="pt").input_ids[0].tolist()]
      bos_done = True
    elif is_image(seg):
      ids += [-(len(images) * n_visual_tokens + t + 1) for t in range(n_visual_tokens)]
      images.append(seg)
    else:
      raise ValueError(f'Input prompts should be either PIL.Image.Image or str types, got {type(seg)} instead.')
  if not ids:
    raise ValueError('Input prompts should be either PIL.Image.Image or str types, got an empty prompt instead.')
  return ids, images, bos_done


class GillDialogues:
  """GILL.open_dialogues(n, capacity): n multi-turn dialogues served as one ragged batch whose KV caches are kept across turns.  Each say() sends
  only the new turn: only its images go through the CLIP tower and only its tokens (behind the pending one) through the decoder layers.
  Stated divergence from the reference's demo (demo/app_gradio.py): the history is kept as token ids and visual rows, not as the decoded text
  re-tokenised at every turn, and images in the model's reply are not fed back.  Not sharded over ranks."""

  def __init__(self, gill, n: int, capacity: Optional[int] = None):
    self.gill = gill
    m = gill.model
    self.session = m.open_session(n, m.opt_cfg.max_positions if capacity is None else capacity)
    self._bos_done = [False] * int(n)

  def _extend_turn(self, rows, turns, always_add_bos: bool) -> None:
    """Segments the named dialogues' new turns (segment_turn), runs only the turn's images through the CLIP tower and extends the session."""
    g, s = self.gill, self.session
    m = g.model
    nv = m.args.n_visual_tokens
    ids, images, done = [], [], []
    for b in rows:
      p = turns[b]
      i, im, d = segment_turn(m.tokenizer, [p] if isinstance(p, str) else list(p), nv, self._bos_done[b], always_add_bos, g._is_image)
      ids.append(i)
      images.append(im)
      done.append(d)
    flat = [im for row in images for im in row]
    extra = [None] * len(rows)
    if flat:
      m._require_vision()
      vis = g._visual_rows(flat)                       # only the new turn's images
      at = 0
      for k, row in enumerate(images):
        if row:
          extra[k] = vis[at:at + len(row) * nv]
          at += len(row) * nv
    s.extend(rows, ids=ids, extra_rows=extra)
    for b, d in zip(rows, done):
      self._bos_done[b] = d

  def say(self, turns, num_words: int = 32, min_word_tokens: int = 0, ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0,
          top_p: float = 1.0, temperature: float = 0.0, max_num_rets: int = 1, generator=None, always_add_bos: bool = False,
          guidance_scale: float = 7.5, num_inference_steps: int = 50, seed: Optional[int] = None, all_branches: bool = False,
          skip_gen_on_ret: bool = False):
    """turns[b]: None (dialogue b is idle this turn) or its new prompt list (PIL images and strings).  Keywords as
    GILL.generate_for_images_and_texts_batch.  Returns, per dialogue, what that method returns for it, or None for an idle one.  After the
    reference's newline truncation the dialogue is rolled back to the truncated ids: its history is what the caller was shown."""
    g, s = self.gill, self.session
    m = g.model
    if len(turns) != s.B:
      raise ValueError(f'say() takes one entry per dialogue ({s.B}), got {len(turns)}')
    if not all_branches and (g.emb_matrix is not None or g.decision_model is not None):
      raise NotImplementedError('say() covers the generation branch only by default: with retrieval embeddings or a decision model attached, '
                                'pass all_branches=True or call generate_for_images_and_texts per prompt list.')
    if num_words == 0:
      raise NotImplementedError('Generation not implemented for num_words=0.')
    if num_words < 0:
      raise ValueError
    s._check()
    rows = [b for b, t in enumerate(turns) if t is not None]
    if not rows:
      return [None] * s.B
    self._extend_turn(rows, turns, always_add_bos)
    tokens, n_tok, hidden, n_hid = s.generate(rows, max_len=num_words, temperature=temperature, top_p=top_p, min_word_tokens=min_word_tokens,
                                              ret_scale_factor=ret_scale_factor, gen_scale_factor=gen_scale_factor, seed=seed)
    outputs, truncs = g._batch_outputs(rows, tokens, n_tok, hidden, n_hid, max_num_rets, generator, guidance_scale, num_inference_steps,
                                       all_branches, skip_gen_on_ret)
    for b, t in zip(rows, truncs):
      if t > 0:
        s.rollback(b, t)
    out = [None] * s.B
    for b, o in zip(rows, outputs):
      out[b] = o
    return out

  def propose(self, turns, n: int = 4, num_words: int = 32, temperature: float = 0.7, top_p: float = 0.95, seed: Optional[int] = None,
              min_word_tokens: int = 0, always_add_bos: bool = False):
    """Best-of-n for a turn: segments and extends turns[b] (None: dialogue b is idle) as say() does, samples n replies per active dialogue
    from its cached history (DialogueSession.sample: the history is read once per group of siblings, not once per reply), truncates each
    reply at the newline as say() does, and scores the truncated replies as continuations of the dialogue (DialogueSession.score,
    reduce='mean').  Returns per dialogue None or dict(texts, tokens: the n truncated replies as strings and id lists, scores (n,) host fp32,
    order: the reply indices from the most to the least likely, best).  Nothing is adopted: the dialogues hold the turn and wait for
    choose(b, j), or for another propose / say.  temperature > 0 needs seed.
    Scope: replies are returned as text and ids; no images are produced for an [IMG] block inside a proposed reply; all_branches is not
    offered; nothing is sharded."""
    g, s = self.gill, self.session
    m = g.model
    if len(turns) != s.B:
      raise ValueError(f'propose() takes one entry per dialogue ({s.B}), got {len(turns)}')
    if num_words <= 0:
      raise ValueError(f'propose() needs num_words >= 1, got {num_words}')
    s._check()
    rows = [b for b, t in enumerate(turns) if t is not None]
    out = [None] * s.B
    self._proposal = None
    if not rows:
      return out
    self._extend_turn(rows, turns, always_add_bos)
    bs = s.sample(rows, n, max_len=num_words, temperature=temperature, top_p=top_p, seed=seed, min_word_tokens=min_word_tokens)
    newline_token_id = m.tokenizer('\n', add_special_tokens=False).input_ids[0]
    replies = []
    for b in rows:
      row = []
      for j in range(int(n)):
        ids = bs.reply(b, j)
        trunc = next((i for i, t in enumerate(ids) if t == newline_token_id), 0)      # say()'s rule: a newline at 0 truncates nothing
        row.append(ids[:trunc] if trunc > 0 else ids)
      replies.append(row)
    for b, row, sc in zip(rows, replies, s.score(rows, replies, reduce='mean')):
      out[b] = dict(texts=[m.tokenizer.batch_decode(torch.tensor([ids], dtype=torch.int64), skip_special_tokens=True)[0] for ids in row], tokens=row, **rank_order(sc))
    self._proposal = (bs, {b: [len(ids) for ids in row] for b, row in zip(rows, replies)})
    return out

  def choose(self, b: int, j: int) -> None:
    """Adopts reply j of the last propose() as dialogue b's turn, truncated as it was shown (DialogueSession.adopt): the dialogue then stands as
    after a say() that had produced that reply.  One choice per dialogue and proposal; valid until the next say, propose or reset."""
    if getattr(self, '_proposal', None) is None:
      raise RuntimeError('choose() follows a propose()')
    bs, keeps = self._proposal
    if b not in keeps or not 0 <= int(j) < len(keeps[b]):
      raise ValueError(f'the last propose() holds no reply {j} of dialogue {b}')
    self.session.adopt(bs, b, int(j), keep=keeps[b][int(j)])

  def rank(self, candidates, reduce: str = 'mean'):
    """candidates[b]: None, or a list of candidate reply strings for dialogue b.  Each is tokenised without <bos> (with it when the dialogue
    is still empty, as the first string of a prompt) and scored as a continuation of the dialogue as it stands (DialogueSession.score: the
    candidate's own tokens only, the dialogue untouched).  Returns per dialogue None or dict(scores=(n,) host fp32 tensor, order=the candidate
    indices from the most to the least likely (NaN scores last), best=order[0] or None)."""
    s = self.session
    if len(candidates) != s.B:
      raise ValueError(f'rank() takes one entry per dialogue ({s.B}), got {len(candidates)}')
    s._check()
    rows = [b for b, c in enumerate(candidates) if c is not None]
    tok = self.gill.model.tokenizer
    ids = []
    for b in rows:
      if any(type(c) != str for c in candidates[b]):
        raise NotImplementedError('rank() takes candidate strings: images inside a candidate are not scored')
      ids.append([[int(v) for v in tok(c, add_special_tokens=not self._bos_done[b], return_tensors="pt").input_ids[0].tolist()]
                  for c in candidates[b]])
    out = [None] * s.B
    if not rows:
      return out
    for b, sc in zip(rows, s.score(rows, ids, reduce=reduce)):
      out[b] = rank_order(sc)
    return out

  def reset(self, rows) -> None:
    self.session.reset(rows)
    for r in self.session._rows(rows):
      self._bos_done[r] = False

  def history(self, row: int):
    return self.session.history(row)
