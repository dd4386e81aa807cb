"""Shared by test_attention_inst_host.py and test_attention_inst_gpu.py (not a test module): the register-staged attention_kernel<DP, NTHR>
(csrc/attention.hip) at every instantiation, on operands that do not average a mistake away.

  * the case table: (B, H, nq, nkv, d, causal) -> the (family, DP, NTHR) the launcher's plan (csrc/attention_plan.h, ops.attention_plan) must give;
  * four deterministic operand builders, each asserting its own premises on the CPU:
      routing   an (almost exactly) one-hot softmax over +-1 keys with integer V: every output row must BE V[pi(i)], so a key in the wrong slot of
                the permuted V^T image, a wrong tile of the rotated walk, a wrong d row, row sum or mask shows as a whole-number error in that row;
      rescale   the two 16-row halves of every wave jump their running max (lazy threshold 8) in different tiles while the other keys keep a
                visible share of the row, whatever the order in which a query tile walks the key tiles;
      shift     test_attention's random operands with every real score moved to about -40 in the exp2 domain: the softmax over the real keys
                does not change, and a zero padding key that the kernel saw would score 0 and own the row;
      large     test_attention_d40_large_scores' construction (spike in the last tile, q times mag) off the LDS-DMA kernel;
  * `emulate`: the kernel's online softmax in fp32 on the host (rotated tile walk per query tile, 32-row waves, lazy running max with the
    wave-wide `any` and per-row delta, P rounded to bf16, row sum from the rounded P on the ones-row kernels and from the fp32 P on the
    others) with a `defect=` switch that breaks it in one of the ways the real kernel could be broken (DEFECTS).

Scores are stated on the kernel's own operands: Q times scale * log2(e) in fp32, rounded to bf16 (pack_heads / the QKV epilogue)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from kv_cache_util import ATTN_BAR, DECODE_SHAPES                                # 2e-2: test_attention
from test_attention_pv48_gpu import ROUTING_BAR, ROUTING_SHAPES as PV48_SHAPES   # 2^-5

REG, DMA = 0, 1       # family: attention_kernel | attention_dma_kernel (include/gill_amd.h gill_attention_plan)
KVT = 64              # keys per tile of the kernel
LN2 = 0.6931471805599453
DIMS = (40, 64, 80, 128, 160)


def padded(d):
  return next(dp for dp in (48, 64, 80, 128, 160) if d <= dp)


# ------------------------------------------------------------------------------------------------ the case table
# 256-thread form, non-causal.  Three (sample, head) pairs leave XCDs 3-7 without work; three 128-query tiles start their walk at tiles 0,
# 5 % nt and 10 % nt; the last wave is ragged (300 = 2 * 128 + 32 + 12).  200 keys: four tiles, 8 keys in the last (d = 40: nkv_pad = 224 is
# not a multiple of 64, so the LDS-DMA kernel does not take it); 77 keys: two tiles, 13 in the last; 257: CLIP ViT-L's shape class, five
# tiles, one key in the last; one key: one tile, two waves with one live query in the second.
NC256 = ([(1, 3, 300, 200, d, False) for d in DIMS] + [(1, 3, 300, 77, d, False) for d in (40, 64, 160)] + [(1, 16, 257, 257, 64, False)] +
         [(1, 2, 33, 1, d, False) for d in (64, 80)])
# 512-thread form, non-causal: 129 pairs, cdiv(300, 256) * 129 = 258 >= 256 workgroups.  The last XCD round holds one pair (surplus workgroups
# exit), the two query tiles walk the four key tiles from tiles 0 and 1, waves 2-7 of the second query tile are idle.
NC512 = [(43, 3, 300, 200, d, False) for d in DIMS]
# Causal: d 64 and 128 only (OPT-125m / OPT-6.7b and CLIP text are the engines that run causal attention).  B H >= 256 takes the 512 form.
CAUSAL512 = [(8, 32, 40, 40, 128, True), (8, 32, 8, 72, 128, True), (22, 12, 40, 40, 64, True)]
CAUSAL256 = [(B, H, nq, nkv, d, True) for B, H, nq, nkv, d in DECODE_SHAPES if (B, H, nq, nkv, d) in ((1, 32, 33, 97, 128), (3, 12, 33, 64, 64))]
assert len(CAUSAL256) == 2
LARGE = [(1, 2, 256, 256, d, False) for d in (64, 80)]
LARGE_MAGS = (64.0, 4096.0)

EXPECTED = {}
for _c in NC256 + CAUSAL256 + LARGE:
  EXPECTED[_c] = (REG, padded(_c[4]), 256)
for _c in NC512 + CAUSAL512:
  EXPECTED[_c] = (REG, padded(_c[4]), 512)
# test_attention_pv48_gpu's shapes: the LDS-DMA kernel, 256 threads but for BIG (512); 77 keys pad to 96 and stay register-staged
PV48_EXPECTED = {(B, H, nq, nkv, 40, False): ((REG if nkv == 77 else DMA), 48, (512 if nq == 2048 else 256)) for B, H, nq, nkv in PV48_SHAPES}

NONCAUSAL = NC256 + NC512
ROUTING_CASES = NC256 + NC512 + CAUSAL512 + CAUSAL256
RESCALE_CASES = [c for c in NONCAUSAL if c[3] > 2 * KVT]            # three key tiles or more
SHIFT_CASES = NONCAUSAL                                             # every one has a ragged last key tile
INDEPENDENCE_CASES = [(1, 3, 300, 200, d, False) for d in DIMS] + [(43, 3, 300, 200, 80, False)]


def case_id(c):
  B, H, nq, nkv, d, causal = c
  return f"B{B}-H{H}-{nq}x{nkv}-d{d}" + ("-causal" if causal else "")


# ------------------------------------------------------------------------------------------------ operands as the kernel sees them
def bf(x):
  return x.to(torch.bfloat16)


def qmul(d):
  """gill_op_attention's multiplier of Q: float(scale) * 1.4426950408889634f in fp32."""
  return float(np.float32(d ** -0.5) * np.float32(1.4426950408889634))


def heads(x, H):      # (B, n, H * d) -> (B, H, n, d) fp32
  B, n, hd = x.shape
  return x.float().view(B, n, H, hd // H).transpose(1, 2)


def prescaled(q, d):
  """What pack_heads hands the kernel: Q times scale * log2(e), rounded to bf16."""
  return bf(q.float() * qmul(d))


def scores2(q, k, H):
  """Scores in the exp2 domain on the kernel's own operands, (B, H, nq, nkv) fp32."""
  d = q.shape[-1] // H
  return heads(prescaled(q, d), H) @ heads(k, H).transpose(-1, -2)


def hidden_keys(nq, nkv, causal):
  """(nq, nkv) bool: key j is masked for query i (causal: j > i + nkv - nq)."""
  if not causal:
    return torch.zeros(nq, nkv, dtype=torch.bool)
  return torch.arange(nkv).view(1, nkv) > (torch.arange(nq) + (nkv - nq)).view(nq, 1)


def oracle(q, k, v, H, causal=False):
  s2 = scores2(q, k, H).masked_fill(hidden_keys(q.shape[1], k.shape[1], causal), -math.inf)
  return (s2 * LN2).softmax(-1) @ heads(v, H)            # (B, H, nq, d)


def row_rel(got, ref):
  """test_attention's figure (max abs error over max |ref|) for every (batch, head, query) row; a non-finite row counts as infinitely wrong."""
  rel = (got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-6)
  return torch.where(torch.isfinite(rel), rel, torch.full_like(rel, math.inf))


def row_abs(got, want):
  err = (got - want).abs().amax(-1)
  return torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))


def whole_rel(got, ref):
  """test_ops_gpu._report's figure."""
  err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
  return err if math.isfinite(err) else math.inf


def _rnd(shape, seed):      # test_ops_gpu._rnd
  return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ routing
@functools.lru_cache(maxsize=None)
def routing_case(B, H, nq, nkv, d, causal):
  """q_i = c k_pi(i) over +-1 keys, pi(i) = (5 i + 3) mod (the number of keys row i may see); V small integers, distinct per (key, d, head,
  sample).  Returns q, k, v (B, n, H d) bf16, want (B, H, nq, d) = V[pi(i)], the smallest lead and the fp32 oracle's error."""
  g = torch.Generator().manual_seed(1000 + nkv + nq + d)
  k = torch.randint(0, 2, (B, nkv, H, d), generator=g).float() * 2 - 1          # +-1: |k|^2 = d for every key
  i = torch.arange(nq)
  visible = i + (nkv - nq) + 1 if causal else torch.full_like(i, nkv)
  pi = (5 * i + 3) % visible
  kk = k.transpose(1, 2)                                                        # (B, H, nkv, d)
  raw = kk[:, :, pi] @ kk.transpose(-1, -2)                                     # k_pi(i) . k_j
  onehot = F.one_hot(pi, nkv).bool()
  hidden = hidden_keys(nq, nkv, causal)
  other = raw.masked_fill(onehot | hidden, -math.inf).amax(-1)                  # (-inf: a row that sees one key)
  gap = min((d - other).min().item(), float(d))
  assert gap > 0, "two equal keys"
  mul = qmul(d)
  c = bf(torch.tensor(1.25 * 30.0 / (mul * gap))).float().item()                # a bf16 value: q = +-c is exact
  q = (c * k[:, pi]).reshape(B, nq, H * d)
  ar = lambda n, *shape: torch.arange(n).view(*shape)
  v = ((7 * ar(nkv, 1, nkv, 1, 1) + 3 * ar(d, 1, 1, 1, d) + 5 * ar(H, 1, 1, H, 1) + 11 * ar(B, B, 1, 1, 1)) % 17 - 8).float()
  q, k, v = bf(q), bf(k.reshape(B, nkv, H * d)), bf(v.reshape(B, nkv, H * d))
  assert torch.equal(v.float(), v.float().round())                              # small integers are exact in bf16
  want = heads(v, H)[:, :, pi]                                                  # (B, H, nq, d): V[pi(i)]
  # premises: the aligned score leads every other visible score of its row by >= 30 in the exp2 domain on the kernel's operands, and the
  # fp32 oracle of the same operands meets the bar
  s2 = scores2(q, k, H)
  lead = (s2.masked_fill(~onehot, -math.inf).amax(-1) - s2.masked_fill(onehot | hidden, -math.inf).amax(-1)).min().item()
  assert lead >= 30.0, lead
  oracle_err = row_abs(oracle(q, k, v, H, causal), want).max().item()
  assert oracle_err <= ROUTING_BAR, oracle_err
  return q, k, v, want, lead, oracle_err


# ------------------------------------------------------------------------------------------------ rescale
RESCALE_BASE = 0.6      # std of the random part of a query: the scores against the other tiles spread by ~2.5 in the exp2 domain over a row


@functools.lru_cache(maxsize=None)
def rescale_case(B, H, nq, nkv, d, alt=False):
  """Queries with (i mod 32) < 16 have one aligned key in the last tile, the others one in the second tile (alt: in the third).  Its score
  leads the maximum of every OTHER tile by 9..14 in the exp2 domain — past the kernel's lazy threshold of 8 whatever the walk order — and the
  other keys keep a visible share of the row.  The keys of tile t are +-1 on their own block of d // ntiles head dims and zero elsewhere, so
  that pulling a query towards its aligned key leaves its scores against the other tiles alone.  At every jump half the rows of a wave
  take delta = 0.  Returns q, k, v, the fp32 oracle (B, H, nq, d), the lead range and the range of the weight the other tiles keep."""
  g = torch.Generator().manual_seed(2000 + nkv + nq + d)
  ntiles = (nkv + KVT - 1) // KVT
  assert ntiles >= 3
  w = d // ntiles
  dims = (torch.arange(d).view(1, d) // w == (torch.arange(nkv) // KVT).view(nkv, 1)).view(1, nkv, 1, d)
  k = bf((torch.randint(0, 2, (B, nkv, H, d), generator=g).float() * 2 - 1) * dims)
  v = bf(torch.randn((B, nkv, H * d), generator=g))
  base = torch.randn((B, nq, H, d), generator=g) * RESCALE_BASE
  i = torch.arange(nq)
  tile = torch.where(i % 32 < 16, torch.full_like(i, ntiles - 1), torch.full_like(i, 2 if alt else 1))
  a = tile * KVT + (5 * i + 3) % torch.clamp(nkv - tile * KVT, max=KVT)         # the aligned key of query i
  ka = k.float()[:, a]                                                          # (B, nq, H, d)
  onehot = F.one_hot(a, nkv).bool()
  own_tile = F.one_hot(tile, ntiles).bool()                                     # (nq, ntiles)
  kflat = k.reshape(B, nkv, H * d)

  def leads(c):
    """bf16 operands of q = base + c k_a, and per row the smallest and the largest lead of the aligned score over the maximum of
    another tile: on the scores the kernel sees."""
    qb = bf((base + c.permute(0, 2, 1).unsqueeze(-1) * ka).reshape(B, nq, H * d))
    s2 = scores2(qb, kflat, H)
    top = s2.masked_fill(~onehot, -math.inf).amax(-1)
    rest = F.pad(s2.masked_fill(onehot, -math.inf), (0, ntiles * KVT - nkv), value=-math.inf)
    tmax = rest.view(B, H, nq, ntiles, KVT).amax(-1)
    lo = top - tmax.masked_fill(own_tile, -math.inf).amax(-1)
    hi = top - tmax.masked_fill(own_tile, math.inf).amin(-1)
    return qb, s2, lo, hi

  c = torch.zeros(B, H, nq)
  for it in range(3):                                                           # (linear in c but for the bf16 rounding of q)
    _, _, lo, hi = leads(c)
    c = c + (9.5 - lo) / (w * qmul(d))
  q, s2, lo, hi = leads(c)
  lo, hi = lo.min().item(), hi.max().item()
  assert 9.0 <= lo and hi <= 14.0, (lo, hi)
  p = (s2 * LN2).softmax(-1)
  elsewhere = (torch.arange(nkv) // KVT).view(1, nkv) != tile.view(nq, 1)
  rest = p.masked_fill(~elsewhere, 0.0).sum(-1)                                 # the weight that the keys of the other tiles keep
  rest = (rest.min().item(), rest.max().item())
  assert rest[0] >= 0.02, rest                                                  # visible: the bar is 2e-2 of the row
  return q, kflat, v, oracle(q, kflat, v, H), (lo, hi), rest


def independence_pair(B, H, nq, nkv, d):
  """The rescale operands, and the same with every query of (i mod 32) >= 16 replaced by one that jumps in another tile."""
  q, k, v = rescale_case(B, H, nq, nkv, d)[:3]
  q2 = rescale_case(B, H, nq, nkv, d, alt=True)[0].clone()
  kept = torch.arange(nq) % 32 < 16
  q2[:, kept] = q[:, kept]
  assert not torch.equal(q2[:, ~kept], q[:, ~kept])
  return q, q2, k, v, kept


# ------------------------------------------------------------------------------------------------ shift
@functools.lru_cache(maxsize=None)
def shift_case(B, H, nq, nkv, d):
  """test_attention's operands; head dim 0 of every key is 1 and head dim 0 of every query moves all its scores by about -40 (exp2
  domain).  Returns q, k, v, the fp32 oracle over the real keys, and the largest real score."""
  q, k, v = (bf(_rnd((B, n, H * d), s)) for n, s in ((nq, 30), (nkv, 31), (nkv, 32)))
  q, k = q.view(B, nq, H, d).clone(), k.view(B, nkv, H, d).clone()
  k[..., 0] = 1.0
  q[..., 0] = bf(torch.tensor(-40.0 / qmul(d)))
  q, k = q.reshape(B, nq, H * d), k.reshape(B, nkv, H * d)
  top = scores2(q, k, H).max().item()
  assert top <= -20.0, top                                                      # a zero padding key (score 0) would own any row by 2^20
  return q, k, v, oracle(q, k, v, H), top


# ------------------------------------------------------------------------------------------------ large scores
@functools.lru_cache(maxsize=None)
def large_case(B, H, nq, nkv, d, mag):
  """test_attention_d40_large_scores' construction at head dim d: key 200 (the last tile) is aligned with query 7, q times mag; the reference
  is taken on the pre-scaled bf16 Q, whose rounding moves scores by whole units at these magnitudes."""
  assert nq == nkv and nkv > 200
  q, k, v = _rnd((B, nq, H * d), 36), _rnd((B, nkv, H * d), 37), _rnd((B, nkv, H * d), 38)
  k[:, 200] = q[:, 7] * 3.0
  q, k, v = bf(q * mag), bf(k), bf(v)
  return q, k, v, oracle(q, k, v, H)


# ------------------------------------------------------------------------------------------------ the kernel's online softmax on the host
DEFECTS = ("v_blocks_exchanged",       # (a) two 4-key blocks of every 16-key group of V exchanged: keys [0-3][8-11][4-7][12-15]
           "walk_wraps_wrong",         # (b) query tile 1 wraps to tile 1, not 0: one key tile's data used twice, tile 0 never
           "row_sum_wrong_row",        # (c) ones-row kernels (DP 48 / 80): the row sum picked from O^T row DP - 16, not row DP
           "l_not_rescaled",           # (d) explicit-sum kernels (DP 64 / 128 / 160): a jump rescales O but not l_run
           "wave_max_delta",           # (e) a jump rescales every row of the wave by the wave's largest delta; the scores lose their own
           "padding_visible")          # (f) the padding keys of the last tile are not masked


def _waves(x, fn):
  """x (..., R) per row -> fn over each 32-row wave, broadcast back to the rows."""
  R = x.shape[-1]
  pad = (-R) % 32
  y = F.pad(x.float(), (0, pad), value=0.0).view(*x.shape[:-1], (R + pad) // 32, 32)
  return fn(y).unsqueeze(-1).expand_as(y).reshape(*x.shape[:-1], R + pad)[..., :R]


def emulate(q, k, v, H, nthr, causal=False, defect=None):
  """attention_kernel<padded(d), nthr> in fp32 on (B, n, H d) bf16 operands -> (B, H, nq, d) fp32 holding bf16 values."""
  assert defect is None or defect in DEFECTS
  d = q.shape[-1] // H
  dp = padded(d)
  has_ones = dp % 32 != 0
  qb = nthr // 2                                                                # queries per workgroup
  kh, vh = heads(k, H), heads(v, H)
  B, _, nkv, _ = kh.shape
  nq = q.shape[1]
  npad = (nkv + KVT - 1) // KVT * KVT
  kh, vh = F.pad(kh, (0, 0, 0, npad - nkv)), F.pad(vh, (0, 0, 0, npad - nkv))   # padding K rows / V^T columns are zeros
  if defect == "v_blocks_exchanged":
    vh = vh.view(B, H, npad // 16, 4, 4, d)[:, :, :, [0, 2, 1, 3]].reshape(B, H, npad, d)
  s_all = heads(prescaled(q, d), H) @ kh.transpose(-1, -2)                      # (B, H, nq, npad)
  masked = F.pad(hidden_keys(nq, nkv, causal), (0, npad - nkv), value=(defect != "padding_visible"))
  coff = nkv - nq
  out = torch.zeros(B, H, nq, d)
  for qt in range((nq + qb - 1) // qb):
    r0, r1 = qt * qb, min(nq, (qt + 1) * qb)
    kv_end = max(1, min(nkv, qt * qb + qb + coff)) if causal else nkv
    nt = (kv_end + KVT - 1) // KVT
    rot = 0 if causal else (qt * 5) % nt
    m = torch.zeros(B, H, r1 - r0)
    l, lo, o = torch.zeros_like(m), torch.zeros_like(m), torch.zeros(B, H, r1 - r0, d)
    data = rot                                                                  # the tile whose K / V^T the iteration holds
    for it in range(nt):
      tile = (it + rot) % nt
      s = s_all[:, :, r0:r1, data * KVT:(data + 1) * KVT] - m.unsqueeze(-1)     # (the accumulator starts at -m_run)
      s = s.masked_fill(masked[r0:r1, tile * KVT:(tile + 1) * KVT], -math.inf)
      mx = s.amax(-1)
      if it == 0:
        delta = torch.where(mx > -math.inf, mx, torch.zeros_like(mx))
        m = delta
      else:
        grow = mx > 8.0
        delta = torch.where(grow, mx, torch.zeros_like(mx))                     # a row that did not ask keeps its max
        scale_by = _waves(delta, lambda y: y.amax(-1)) if defect == "wave_max_delta" else delta
        alpha = torch.exp2(-scale_by)
        m = m + delta
        o, lo = o * alpha.unsqueeze(-1), lo * alpha
        if defect != "l_not_rescaled":
          l = l * alpha
      p = torch.exp2(s - delta.unsqueeze(-1))
      pb = bf(p).float()
      l = l + p.sum(-1)                                                         # explicit sum: of the fp32 P
      lo = lo + pb.sum(-1)                                                      # ones row of V^T: of the rounded P, through the MFMA
      o = o + pb @ vh[:, :, data * KVT:(data + 1) * KVT]
      nxt = tile + 1 if tile + 1 < nt else 0
      if defect == "walk_wraps_wrong" and qt == 1 and tile + 1 >= nt:
        nxt = min(1, nt - 1)
      data = nxt
    rowsum = lo if has_ones else l
    if defect == "row_sum_wrong_row":
      rowsum = o[..., dp - 16]
    out[:, :, r0:r1] = o / rowsum.unsqueeze(-1)
  return bf(out).float()


def defect_applies(defect, case):
  B, H, nq, nkv, d, causal = case
  dp, qb = padded(d), EXPECTED[case][2] // 2
  return {"v_blocks_exchanged": True,
          "walk_wraps_wrong": not causal and nq > qb and 5 % ((nkv + KVT - 1) // KVT) != 0,      # query tile 1 exists and starts off tile 0
          "row_sum_wrong_row": dp % 32 != 0,
          "l_not_rescaled": dp % 32 == 0,
          "wave_max_delta": True,
          "padding_visible": nkv % KVT != 0}[defect]


# ------------------------------------------------------------------------------------------------ the GPU side
def run(q, k, v, H, causal, device):
  """ops.attention on the device -> (B, H, nq, d) fp32 on the CPU."""
  from gill_amd import ops
  d = q.shape[-1] // H
  out = ops.attention(q.to(device), k.to(device), v.to(device), H, d ** -0.5, causal)
  return heads(out.float().cpu(), H)
