"""Level-0 attention (d = 40, attention_dma_kernel) with P.V on 16x16x32 MFMAs over 48 head rows.

The P fragments are regrouped between lane rows (v_permlane16_swap_b32), V^T is read as the A operand in the matching key order,
the ones row that carries the row sum is fetched into LDS row 40, and in the rare running-max jump every accumulator block takes its
rescale factor from another lane row.  Random operands average over most of these; the two tests here do not:

  routing  an (almost exactly) one-hot softmax with integer V: every output row must BE one V row, so a wrong key group, query block,
           d row, row sum or tile mask shows as a whole-number error in that row;
  rescale  the two 16-query blocks of every wave jump their running max in different tiles (or by different amounts), and earlier keys
           keep a visible share of the row, so a rescale factor taken from the wrong block misses the bar (shown on the host below).
"""
import functools
import math

import pytest
import torch

D = 40
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
SCALE = D ** -0.5
KVT = 64              # keys per tile of the kernel

# (B, H, nq, nkv).  128 queries of 2 heads run the 256-thread form: one tile, both ring stages, an odd tile count, ragged last tiles
# (77 keys pad to 96, which the LDS-DMA kernel does not take: that case runs the register-staged kernel; 100 keys pad to 128 and stay
# on the LDS-DMA kernel).  cdiv(2048, 256) * 4 * 8 = 256 workgroups reach the 512-thread form, with a rotated tile walk per query tile.
SMALL = [(1, 2, 128, n) for n in (64, 128, 192, 77, 100)]
BIG = (4, 8, 2048, 192)
ROUTING_SHAPES = SMALL + [BIG]
RESCALE_SHAPES = [s for s in SMALL if s[3] > KVT] + [BIG]      # a jump needs an earlier tile
ROUTING_BAR = 2.0 ** -5
ATTN_BAR = 2e-2       # test_ops_gpu.test_attention


def _bf(x):
  return x.to(torch.bfloat16)


def _heads(x, H):      # (B, n, H * d) -> (B, H, n, d) fp32
  B, n, _ = x.shape
  return x.float().view(B, n, H, D).transpose(1, 2)


def _prescaled(q):
  """What pack_heads / the QKV epilogue hand the kernel: Q times scale * log2(e), rounded to bf16."""
  return _bf(q.float() * (SCALE * LOG2E))


def _scores2(q, k, H):
  """Scores in the exp2 domain on the kernel's own operands, (B, H, nq, nkv) fp32."""
  return _heads(_prescaled(q), H) @ _heads(k, H).transpose(-1, -2)


def _oracle(q, k, v, H):
  p = (_scores2(q, k, H) * LN2).softmax(-1)
  return p @ _heads(v, H)            # (B, H, nq, d)


def _rows(out, H):     # kernel output (B, nq, H * d) -> (B, H, nq, d) fp32 on the CPU
  return _heads(out.float().cpu(), H)


def _row_rel(got, ref):
  """test_attention's figure (max abs error over max |ref|) for every (batch, head, query) row."""
  return (got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-6)


# ------------------------------------------------------------------------------------------------ routing
@functools.lru_cache(maxsize=None)
def _routing_case(B, H, nq, nkv):
  g = torch.Generator().manual_seed(1000 + nkv + nq)
  k = torch.randint(0, 2, (B, nkv, H, D), generator=g).float() * 2 - 1          # +-1: |k|^2 = 40 for every key
  pi = (5 * torch.arange(nq) + 3) % nkv
  kk = k.transpose(1, 2)                                                        # (B, H, nkv, d)
  raw = kk[:, :, pi] @ kk.transpose(-1, -2)                                     # k_pi(i) . k_j
  other = raw.masked_fill(torch.nn.functional.one_hot(pi, nkv).bool(), -math.inf).amax(-1)
  gap = (D - other).min().item()
  assert gap > 0, "two equal keys"
  c = _bf(torch.tensor(1.25 * 30.0 / (SCALE * LOG2E * gap))).float().item()     # a bf16 value: q = +-c is exact
  q = (c * k[:, pi]).reshape(B, nq, H * D)
  kd = torch.arange(nkv).view(1, nkv, 1, 1)
  v = ((7 * kd + 3 * torch.arange(D).view(1, 1, 1, D) + 5 * torch.arange(H).view(1, 1, H, 1)) % 17 - 8).float()
  v = v.expand(B, nkv, H, D).reshape(B, nkv, H * D)
  q, k, v = _bf(q), _bf(k.reshape(B, nkv, H * D)), _bf(v)
  assert torch.equal(v.float(), v.float().round())                              # small integers are exact in bf16
  want = _heads(v, H)[:, :, pi]                                                 # (B, H, nq, d): V[pi(i)]
  # on the CPU: the aligned score leads every other score of its row by >= 30 in the exp2 domain, and the fp32 oracle of the
  # same operands meets the bar
  s2 = _scores2(q, k, H)
  onehot = torch.nn.functional.one_hot(pi, nkv).bool()
  lead = (s2.masked_fill(~onehot, -math.inf).amax(-1) - s2.masked_fill(onehot, -math.inf).amax(-1)).min().item()
  assert lead >= 30.0, lead
  oracle_err = (_oracle(q, k, v, H) - want).abs().amax(-1).max().item()
  assert oracle_err <= ROUTING_BAR, oracle_err
  return q, k, v, want, lead, oracle_err


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,nq,nkv", ROUTING_SHAPES)
def test_pv48_routing_one_hot_rows_equal_their_v_row(cuda, B, H, nq, nkv):
  """Query i is aligned with key pi(i) = (5 i + 3) mod nkv by a lead of >= 30 in the exp2 domain; V holds small integers, distinct per
  (key, d, head).  Every output row must equal V[pi(i)] to 2^-5."""
  from gill_amd import ops
  q, k, v, want, lead, oracle_err = _routing_case(B, H, nq, nkv)
  out = _rows(ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H), H)
  assert torch.isfinite(out).all()
  err = (out - want).abs().amax(-1)                                             # per (batch, head, query) row
  w = int(err.argmax())
  print(f"[pv48 routing B{B} H{H} {nq}x{nkv}] lead {lead:.1f}, oracle err {oracle_err:.2e}, worst row (flat {w}) err {err.max().item():.4e}, "
        f"rows over the bar {(err > ROUTING_BAR).sum().item()} of {err.numel()}")
  assert err.max().item() <= ROUTING_BAR


# ------------------------------------------------------------------------------------------------ rescale
@functools.lru_cache(maxsize=None)
def _rescale_case(B, H, nq, nkv):
  """Queries with (i mod 32) < 16 have one aligned key in the last tile, the others one in the second tile.  Its score leads the
  maximum of every OTHER tile by 9..14 in the exp2 domain (so it leads the row's earlier maximum by that much whatever the order in
  which a workgroup walks the tiles), which is past the lazy threshold of 8: the slow path runs, and the earlier keys keep a visible
  share of the row.  The keys of tile t are +-1 on head dims 13 t .. 13 t + 12 and zero elsewhere: pulling a query towards its aligned
  key then leaves its scores against the other tiles alone (with dense random keys k_a . k_j moves them by a sixth of the lead, one
  standard deviation, and no window five wide holds every row)."""
  g = torch.Generator().manual_seed(2000 + nkv + nq)
  ntiles = (nkv + KVT - 1) // KVT
  dims = (torch.arange(D).view(1, D) // 13 == (torch.arange(nkv) // KVT).view(nkv, 1)).view(1, nkv, 1, D)
  k = _bf((torch.randint(0, 2, (B, nkv, H, D), generator=g).float() * 2 - 1) * dims)
  v = _bf(torch.randn((B, nkv, H * D), generator=g))
  base = torch.randn((B, nq, H, D), generator=g)                                # scores of std ~0.8 in the exp2 domain
  i = torch.arange(nq)
  tile = torch.where(i % 32 < 16, torch.full_like(i, ntiles - 1), torch.ones_like(i))
  a = tile * KVT + (5 * i + 3) % torch.clamp(nkv - tile * KVT, max=KVT)         # the aligned key of query i
  ka = k.float()[:, a]                                                          # (B, nq, H, d)
  onehot = torch.nn.functional.one_hot(a, nkv).bool()
  own_tile = torch.nn.functional.one_hot(tile, ntiles).bool()                   # (nq, ntiles)
  kflat = k.reshape(B, nkv, H * D)

  def leads(c):
    """bf16 operands of q = base + c k_a, and per row the smallest and the largest lead of the aligned score over the maximum of
    another tile: on the scores the kernel sees."""
    qb = _bf((base + c.permute(0, 2, 1).unsqueeze(-1) * ka).reshape(B, nq, H * D))
    s2 = _scores2(qb, kflat, H)
    top = s2.masked_fill(~onehot, -math.inf).amax(-1)
    rest = torch.nn.functional.pad(s2.masked_fill(onehot, -math.inf), (0, ntiles * KVT - nkv), value=-math.inf)
    tmax = rest.view(B, H, nq, ntiles, KVT).amax(-1)
    lo = top - tmax.masked_fill(own_tile, -math.inf).amax(-1)
    hi = top - tmax.masked_fill(own_tile, math.inf).amin(-1)
    return qb, s2, lo, hi

  c = torch.zeros(B, H, nq)
  for it in range(3):                                                           # (linear in c but for the bf16 rounding of q)
    _, _, lo, hi = leads(c)
    c = c + (9.5 - lo) / (13 * SCALE * LOG2E)
  q, s2, lo, hi = leads(c)
  lo, hi = lo.min().item(), hi.max().item()
  assert 9.0 <= lo and hi <= 14.0, (lo, hi)
  p = (s2 * LN2).softmax(-1)
  elsewhere = (torch.arange(nkv) // KVT).view(1, nkv) != tile.view(nq, 1)
  rest = p.masked_fill(~elsewhere, 0.0).sum(-1)                                 # the weight that the keys of the other tiles keep
  k = kflat
  return q, k, v, _oracle(q, k, v, H), (lo, hi), (rest.min().item(), rest.max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,nq,nkv", RESCALE_SHAPES)
def test_pv48_rescale_per_query_block(cuda, B, H, nq, nkv):
  """The running-max jump, with the two 16-query blocks of every wave jumping in different tiles: test_attention's bar, per row,
  against the fp32 oracle on the kernel's own pre-scaled bf16 operands."""
  from gill_amd import ops
  q, k, v, ref, lead, rest = _rescale_case(B, H, nq, nkv)
  out = _rows(ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H), H)
  assert torch.isfinite(out).all()
  rel = _row_rel(out, ref)
  print(f"[pv48 rescale B{B} H{H} {nq}x{nkv}] lead {lead[0]:.2f}..{lead[1]:.2f}, other keys keep {100 * rest[0]:.1f}..{100 * rest[1]:.1f} %, "
        f"worst row {rel.max().item():.4e}, rows over the bar {(rel >= ATTN_BAR).sum().item()} of {rel.numel()}")
  assert rel.max().item() < ATTN_BAR


def _online_softmax(q, k, v, H, swap_blocks):
  """The kernel's online softmax in fp32 (64-key tiles in natural order, 32 queries per wave, lazy running max with the wave-wide
  `any`, P rounded to bf16, the row sum accumulated from the rounded P).  swap_blocks: in the slow path the two 16-query blocks of
  a wave take each other's rescale factor — the mistake the per-block exchange of the kernel could make."""
  s2 = _scores2(q, k, H)
  vh = _heads(v, H)
  B, _, nq, nkv = s2.shape
  o = torch.zeros(B, H, nq, D)
  l = torch.zeros(B, H, nq)
  m = torch.zeros(B, H, nq)
  for t in range((nkv + KVT - 1) // KVT):
    s = s2[..., t * KVT:(t + 1) * KVT] - m.unsqueeze(-1)
    mx = s.amax(-1)
    if t == 0:
      delta = mx
    else:
      jump = (mx > 8.0).view(B, H, nq // 32, 32).any(-1, keepdim=True).expand(B, H, nq // 32, 32).reshape(B, H, nq)
      delta = torch.where(jump, mx.clamp_min(0.0), torch.zeros_like(mx))
      alpha = torch.exp2(-delta)
      if swap_blocks:
        alpha = alpha.view(B, H, nq // 32, 2, 16).flip(-2).reshape(B, H, nq)
      o, l = o * alpha.unsqueeze(-1), l * alpha
    m = m + delta
    p = _bf(torch.exp2(s - delta.unsqueeze(-1))).float()
    o = o + p @ vh[:, :, t * KVT:(t + 1) * KVT]
    l = l + p.sum(-1)
  return _bf(o / l.unsqueeze(-1)).float()


def test_pv48_rescale_check_sees_swapped_block_factors():
  """Host only: on the rescale operands an emulation of the kernel's online softmax meets the bar, and the same emulation with the two
  16-query blocks' rescale factors exchanged misses it by more than 10 x."""
  B, H, nq, nkv = 1, 2, 128, 192
  q, k, v, ref, _, _ = _rescale_case(B, H, nq, nkv)
  good = _row_rel(_online_softmax(q, k, v, H, False), ref).max().item()
  bad = _row_rel(_online_softmax(q, k, v, H, True), ref).max().item()
  print(f"[pv48 rescale emulation] worst row: as built {good:.4e}, block factors swapped {bad:.4e}")
  assert good < ATTN_BAR
  assert bad >= 10 * ATTN_BAR
