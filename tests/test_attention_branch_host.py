"""Branch decode attention (csrc/attention_branch.hip) on the CPU: what the GPU test's accuracy bar can and cannot see.

`emulate` restates the kernel's arithmetic in fp32: the prefix tiles of 32 slots dealt to four waves by tile index, each wave's online softmax
in the log2 domain with the scale applied in fp32 and the probabilities rounded to bf16 for P.V, the branch's own slots and its new token as one
fp32 pass, then the merge of the four partials in wave order and the own part, a wave without a tile selected away.  Against fp64 on the same
bf16 operands it must pass test_attention_branch_gpu's bar (kv_cache_util.ATTN_BAR, report_rows' figure) on every case; with each of DEFECTS
switched on it must miss that bar by a factor of at least 3 on at least one case, so the GPU test would catch a kernel that has the defect.

Cases: the shapes' head dims, prefix lengths on both sides of a tile and of the four-wave deal, own counts 0, 1 and 33.  Slot n of the prefix row
and slot m of the branch row (the first ones a branch must not see) hold a key that leans towards the query as its own new key does; a sibling
brings 33 own keys.  One case more shifts every score far below zero (keys pointing away from the query): attention does not change under a
shift of the scores, but an empty partial that enters the merge as zeros (maximum 0, sum 0) is harmless EXCEPT there, where the false maximum
flushes every true weight to zero."""
import math

import pytest
import torch

import kv_cache_util as U

DEFECTS = ("prefix_slot_beyond_n_visible", "own_slot_beyond_m_visible", "new_key_hidden", "sibling_own_keys_visible", "merge_drops_a_wave",
           "empty_partial_as_zeros")
LOG2E = 1.4426950408889634
# (H, d, n, m, deep): deep = every score shifted far below zero
CASES = ([(2, d, n, m, False) for d in (64, 80, 128) for n, m in ((0, 0), (1, 33), (33, 1), (129, 0), (160, 33))] +
         [(2, 64, 33, 1, True), (2, 128, 0, 1, True)])


def _inputs(H, d, n, m, deep, seed):
  """q (H,d); prefix K / V (H, n + 1, d) (slot n stale); own k / v (H, m + 2, d): slots 0 .. m - 1 cached, m the new token, m + 1 what slot m of
  the branch row held before (stale); sibling own keys / values (H, 33, d).  bf16-valued floats."""
  _, kp, vp = U.decode_attn_inputs(1, H, 1, n + 1, d, seed=seed)
  q, ko, vo = U.decode_attn_inputs(1, H, 1, m + 1, d, seed=seed + 1)
  _, ks, vs = U.decode_attn_inputs(1, H, 1, 33, d, seed=seed + 2)
  heads = lambda t: t[0].view(-1, H, d).transpose(0, 1)     # noqa: E731
  q, kp, vp, ko, vo, ks, vs = (heads(t) for t in (q, kp, vp, ko, vo, ks, vs))
  q = q[:, 0]
  lean = U.bf(q / 3.0 * (2.0 / math.sqrt(d)))[:, None]      # + ~6 on the score, as the new key has
  g = torch.Generator().manual_seed(seed + 3)
  kp = torch.cat([kp[:, :n], lean], 1)
  ko = torch.cat([ko, lean], 1)
  vo = torch.cat([vo, U.bf(torch.randn((H, 1, d), generator=g))], 1)
  if deep:      # every key the branch sees points away from the query: scores around -250 in the log2 domain
    away = U.bf(-q * (60.0 / math.sqrt(d)))[:, None]
    kp[:, :n] += away
    ko[:, :m + 1] += away
    kp, ko = U.bf(kp), U.bf(ko)
  return q, kp, vp, ko, vo, ks, vs


def _ref(q, kp, vp, ko, vo, n, m):
  d = q.shape[-1]
  k = torch.cat([kp[:, :n], ko[:, :m + 1]], 1).double()
  v = torch.cat([vp[:, :n], vo[:, :m + 1]], 1).double()
  s = (k @ q.double()[:, :, None])[..., 0] * d ** -0.5
  return (s.softmax(-1)[:, None] @ v)[:, 0].float()


def emulate(q, kp, vp, ko, vo, ks, vs, n, m, defect=None):
  """(H, d) fp32: the kernel's tile order and merge.  Everything is per head; q (H,d)."""
  H, d = q.shape
  qscale = torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
  ninf = float("-inf")
  nvis = n + 1 if defect == "prefix_slot_beyond_n_visible" else n
  parts = []
  for w in range(4):
    mr, lr, o = torch.full((H,), ninf), torch.zeros(H), torch.zeros(H, d)
    met = False
    for kv0 in range(w * 32, n, 128):          # the deal is a function of n alone
      met = True
      hi = min(kv0 + 32, kp.shape[1])
      s = (kp[:, kv0:hi] @ q[:, :, None])[..., 0] * qscale
      vis = torch.arange(kv0, hi) < nvis
      s = torch.where(vis[None], s, torch.full_like(s, ninf))
      m_new = torch.maximum(mr, s.amax(-1))
      alpha = torch.exp2(mr - m_new)
      p = torch.exp2(s - m_new[:, None])
      lr = lr * alpha + p.sum(-1)
      vt = torch.where(vis[None, :, None], vp[:, kv0:hi], torch.zeros(()))
      o = o * alpha[:, None] + (U.bf(p)[:, None] @ vt)[:, 0]
      mr = m_new
    parts.append((met, mr, lr, o))
  # own part: the cached slots 0 .. m - 1 and the new token (ko[:, m]); ko[:, m + 1] is what slot m of the row held
  idx = list(range(m + 1))
  if defect == "own_slot_beyond_m_visible":
    idx.append(m + 1)
  if defect == "new_key_hidden":
    idx.remove(m)
  k, v = ko[:, idx], vo[:, idx]
  if defect == "sibling_own_keys_visible":
    k, v = torch.cat([ks, k], 1), torch.cat([vs, v], 1)
  if k.shape[1]:
    s = (k @ q[:, :, None])[..., 0] * qscale
    mo = s.amax(-1)
    p = torch.exp2(s - mo[:, None])
    lo, oo = p.sum(-1), (p[:, None] @ v)[:, 0]
  else:
    mo, lo, oo = torch.full((H,), ninf), torch.zeros(H), torch.zeros(H, d)
  # merge
  M = mo.clone()
  for w, (met, mr, lr, o) in enumerate(parts):
    if not met and defect == "empty_partial_as_zeros":
      parts[w] = (True, torch.zeros(H), torch.zeros(H), torch.zeros(H, d))
    if defect == "merge_drops_a_wave" and w == 1:
      parts[w] = (False, mr, lr, o)
    if parts[w][0]:
      M = torch.maximum(M, parts[w][1])
  L, O = torch.zeros(H), torch.zeros(H, d)
  for met, mr, lr, o in parts:
    if met:
      f = torch.exp2(mr - M)
      L, O = L + f * lr, O + f[:, None] * o
  f = torch.exp2(mo - M)
  L, O = L + f * lo, O + f[:, None] * oo
  return O / L[:, None]


def _figure(tag, got, ref):
  return U.report_rows(tag, got.reshape(1, 1, -1), ref.reshape(1, 1, -1))


def _applies(defect, n, m):
  return {"prefix_slot_beyond_n_visible": True, "own_slot_beyond_m_visible": True, "new_key_hidden": n + m > 0, "sibling_own_keys_visible": True,
          "merge_drops_a_wave": n > 32, "empty_partial_as_zeros": n <= 96}[defect]


def test_emulation_passes_the_bar_on_every_case():
  worst = 0.0
  for i, (H, d, n, m, deep) in enumerate(CASES):
    ins = _inputs(H, d, n, m, deep, seed=900 + 7 * i)
    q, kp, vp, ko, vo, ks, vs = ins
    rel = _figure(f"branch emulation d{d} n{n} m{m} deep={deep}", emulate(*ins, n, m), _ref(q, kp, vp, ko, vo, n, m))
    worst = max(worst, rel)
    assert rel < U.ATTN_BAR, (H, d, n, m, deep, rel)
  print(f"[branch emulation] worst figure {worst:.3e} = {worst / U.ATTN_BAR:.3f} of the bar {U.ATTN_BAR}")


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_misses_the_bar_by_3x(defect):
  best, where = 0.0, None
  for i, (H, d, n, m, deep) in enumerate(CASES):
    if not _applies(defect, n, m):
      continue
    ins = _inputs(H, d, n, m, deep, seed=900 + 7 * i)
    q, kp, vp, ko, vo, ks, vs = ins
    rel = _figure(f"branch {defect} d{d} n{n} m{m} deep={deep}", emulate(*ins, n, m, defect=defect), _ref(q, kp, vp, ko, vo, n, m))
    print(f"[branch {defect}] d{d} n{n} m{m} deep={deep}: misses the bar by a factor of {rel / U.ATTN_BAR:.2f}")
    if rel > best:
      best, where = rel, (d, n, m, deep)
  print(f"[branch {defect}] largest factor {best / U.ATTN_BAR:.2f} at (d, n, m, deep) = {where}")
  assert best >= 3 * U.ATTN_BAR, f"{defect} stays within 3x of the bar on every case: largest factor {best / U.ATTN_BAR:.2f} at {where}"
