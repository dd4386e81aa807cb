"""The yardstick of the retrieval tests: an fp64 restatement of gill_ret_index_search (gill/models.py:671-696: scores = emb_matrix @ ret_emb.T,
scores[seen] -= penalty, topk) with the documented order (score descending, then row index ascending), the acceptance rule, and the derived
error bounds.  CPU only.

Acceptance rule for a returned (scores, idx) against the fp64 scores S[q, n] (penalties applied) and a bound b[q, n] >= |returned - S|:
  (i)   indices are distinct and inside [0, size), or -1 in the trailing max(0, k - size) slots (then with score -inf);
  (ii)  returned scores are non-increasing;
  (iii) each returned score is within b of S at its index;
  (iv)  every row NOT returned has S <= (the k-th returned score) + 2 b   (its own b: one for each of the two scores compared).
With b = 0 the rule admits only an exact top-k set; `exact_equal` additionally pins the order among equals.

Bounds (derived, not measured).  The restatement takes the operands the kernel multiplies — the STORED bf16 rows and the bf16-rounded queries —
so with normalize = 0 only the fp32 accumulation order differs: |err| <= dim * 2^-24 * sum_i |a_i q_i| (dim - 1 additions and the products'
alignment inside the matrix instruction, each within 2^-24 of the running magnitude).  With normalize = 1 the device divides by an fp32 norm
whose last bit may differ from the fp64 one: a query element near a rounding boundary may then land on the neighbouring bf16 value, one ulp =
at most 2^-8 of itself: + 2^-8 * sum_i |a_i q_i|.  Rows stored by add(normalize = 1) are scale * row / ||row|| computed in fp32 (relative
error of a few 2^-24) and rounded once to bf16: within 2^-8 |want| of the fp64 value."""
import math

import torch

GUARD = 64


def bf16_round(x: torch.Tensor) -> torch.Tensor:
  return x.float().to(torch.bfloat16).double()


def exact_inputs(N, dim, Q, seed):
  """Integer rows in [-4, 4] and queries in [-2, 4] (not the same law: a kernel that swapped the operands' roles would not score alike): every
  product and partial sum is an integer below 2^24, so fp32 accumulation in any order is exact; ties are plentiful."""
  g = torch.Generator().manual_seed(seed)
  rows = torch.randint(-4, 5, (N, dim), generator=g).double()
  queries = torch.randint(-2, 5, (Q, dim), generator=g).double()
  return rows, queries


def normalized_rows(raw: torch.Tensor, scale: float) -> torch.Tensor:
  """fp64 scale * row / ||row||; a zero row stays zero (the documented divergence from the reference's NaN)."""
  raw = raw.double()
  n = raw.norm(dim=1, keepdim=True)
  return torch.where(n > 0, scale * raw / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(raw))


def normalized_queries(q: torch.Tensor) -> torch.Tensor:
  """What search(normalize = 1) multiplies, up to the last bit of the fp32 norm: bf16(q / ||q||)."""
  return bf16_round(normalized_rows(q, 1.0))


def penalised_scores(rows, queries, exclude=None, penalty=0.0):
  """rows (N, D), queries (Q, D), both already what the kernel multiplies, as doubles -> (S (Q, N) fp64, mag (Q, N) = sum |a_i q_i|).
  exclude: per query a list of rows (-1 = empty slot); a listed row loses `penalty` once."""
  S = queries @ rows.T
  mag = queries.abs() @ rows.abs().T
  if exclude is not None:
    for q, lst in enumerate(exclude):
      for r in sorted(set(int(i) for i in lst if int(i) >= 0)):
        S[q, r] -= penalty
  return S, mag


def topk_ref(S: torch.Tensor, k: int):
  """Exact top-k of S (Q, N) by (score descending, index ascending) -> (scores (Q, k) fp64, idx (Q, k) int64); slots past N: (-inf, -1)."""
  Q, N = S.shape
  order = torch.sort(-S, dim=1, stable=True).indices[:, :k]
  scores = torch.gather(S, 1, order)
  if k > N:
    scores = torch.cat([scores, torch.full((Q, k - N), -math.inf, dtype=S.dtype)], 1)
    order = torch.cat([order, torch.full((Q, k - N), -1, dtype=torch.int64)], 1)
  return scores, order


def bound(mag: torch.Tensor, dim: int, normalize: bool) -> torch.Tensor:
  b = dim * 2.0 ** -24 * mag
  if normalize:
    b = b + 2.0 ** -8 * mag
  return b


def accept(scores, idx, S, b):
  """The rule of the module docstring -> (ok, message).  scores (Q, k), idx (Q, k) as returned; S, b (Q, N) fp64 (b may be the number 0)."""
  scores, idx = scores.double().cpu(), idx.cpu()
  Q, N = S.shape
  k = idx.shape[1]
  if not torch.is_tensor(b):
    b = torch.full_like(S, float(b))
  for q in range(Q):
    real = min(k, N)
    ii, ss = idx[q, :real], scores[q, :real]
    if bool((idx[q, real:] != -1).any()) or bool((scores[q, real:] != -math.inf).any()):
      return False, f"(i) query {q}: slots past size must be (-1, -inf): {idx[q].tolist()} {scores[q].tolist()}"
    if bool(((ii < 0) | (ii >= N)).any()) or len(set(ii.tolist())) != real:
      return False, f"(i) query {q}: indices {ii.tolist()} not distinct rows of [0, {N})"
    if bool((ss[1:] > ss[:-1]).any()):
      return False, f"(ii) query {q}: scores increase: {ss.tolist()}"
    err = (ss - S[q, ii]).abs()
    if bool((err > b[q, ii]).any()):
      j = int((err - b[q, ii]).argmax())
      return False, f"(iii) query {q} slot {j}: score {ss[j].item()} vs {S[q, ii[j]].item()}, bound {b[q, ii[j]].item()}"
    if real < N:
      rest = torch.ones(N, dtype=torch.bool)
      rest[ii] = False
      over = S[q] - 2 * b[q] - ss[real - 1]
      over[~rest] = -math.inf
      if bool((over > 0).any()):
        j = int(over.argmax())
        return False, f"(iv) query {q}: row {j} with score {S[q, j].item()} left out; k-th returned {ss[real - 1].item()}, bound {b[q, j].item()}"
  return True, ""


def exact_equal(scores, idx, S, k):
  """Bit for bit: the returned pair equals topk_ref (order among equals included).  For data on which fp32 accumulation is exact."""
  ws, wi = topk_ref(S, k)
  return bool(torch.equal(idx.cpu(), wi)) and bool(torch.equal(scores.double().cpu(), ws))


def guarded(shape, dtype, device):
  """An output tensor with GUARD sentinel words behind it in the same allocation -> (buffer, view)."""
  n = 1
  for d in shape:
    n *= int(d)
  fill, guard = (float("nan"), -12352.0) if dtype.is_floating_point else (-7777777, -12352)
  buf = torch.full((n + GUARD,), fill, device=device, dtype=dtype)
  buf[n:] = guard
  return buf, buf[:n].view(*shape)


def guard_ok(buf) -> bool:
  return bool((buf[-GUARD:] == -12352).all())
