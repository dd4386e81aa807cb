"""ops.attention_decode (gill_attention_decode: one new token per row against that row's own cache length, with append) on the MI355X.

Per (B, H, d) and cache pitch, the rows of a batch take different lengths from LENGTHS (every length below the pitch, plus pitch - 1), in
groups of B until every length has been a row; inputs are built like kv_cache_util.decode_attn_inputs (peaked scores, the newest key
leaning to its query), one sequence per row, and the cache beyond each length is filled with finite LARGE stale values (+-1e30) in K and
V^T.  Checked per group:

  accuracy            against fp64 on the same bf16 operands, kv_cache_util.report_rows' figure per batch row, at ATTN_BAR = 2e-2;
  append              slot n of K and V^T holds the new key / value bit for bit, and no other slot of either cache changed (where the
                      V^T rows are padded, d = 80, the entry [d][n] of the ones-row the flash kernel reads is 1.0);
  batch independence  every row run alone at B = 1 gives the bits of its row in the batch;
  clamp               a length >= pitch (or < 0) sets the row's flag, guard words around both caches and the output stay untouched,
                      and the unclamped rows of the same launch keep their bits."""
import pytest
import torch

import kv_cache_util as U

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 128), (3, 12, 64), (2, 32, 80), (9, 12, 64)]
PITCHES = (96, 320)
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
STALE = 1e30          # finite in bf16; 0 * STALE is still 0, but STALE * anything that is not selected out would drown a row
GUARD = 256           # elements in front of and behind every guarded buffer


def _lengths(pitch):
  return [n for n in LENGTHS if n < pitch - 1] + [pitch - 1]


def _groups(B, pitch, rot):
  """Groups of B lengths covering every candidate, neighbours in the list landing in one batch; `rot` rotates the start."""
  ls = _lengths(pitch)
  ls = ls[rot % len(ls):] + ls[:rot % len(ls)]
  ls = ls + ls[:(-len(ls)) % B]
  return [ls[i:i + B] for i in range(0, len(ls), B)]


def _guarded(shape, fill, dev):
  n = 1
  for s in shape:
    n *= s
  big = torch.full((n + 2 * GUARD,), fill, dtype=torch.bfloat16, device=dev)
  return big, big[GUARD:GUARD + n].view(shape)


def _guards_intact(big, fill):
  g = torch.cat([big[:GUARD], big[-GUARD:]]).float()
  return bool((g == fill).all())


def _case(B, H, d, pitch, lens, seed, dev):
  """Host tensors of one batch: q, k_new, v_new (B, H*d); K (B,H,pitch,d), Vt (B,H,dpv,pitch) with stale values beyond each length;
  the fp64 reference (B, H*d)."""
  dpv = (d + 31) // 32 * 32
  g = torch.Generator().manual_seed(seed)
  sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -STALE, STALE)   # noqa: E731
  K, Vt = U.bf(sign((B, H, pitch, d))), U.bf(sign((B, H, dpv, pitch)))
  q, kn, vn, ref = (torch.empty(B, H * d) for _ in range(4))
  for b, n in enumerate(lens):
    qb, kb, vb = U.decode_attn_inputs(1, H, 1, n + 1, d, seed=seed * 131 + b)
    q[b], kn[b], vn[b] = qb[0, 0], kb[0, n], vb[0, n]
    kh = kb[0].view(n + 1, H, d).transpose(0, 1)          # (H, n + 1, d)
    vh = vb[0].view(n + 1, H, d).transpose(0, 1)
    K[b, :, :n] = kh[:, :n]
    Vt[b, :, :d, :n] = vh[:, :n].transpose(1, 2)
    s = (qb[0, 0].view(H, 1, d).double() @ kh.double().transpose(1, 2)) * d ** -0.5
    ref[b] = (s.softmax(-1) @ vh.double()).reshape(H * d).float()
  return q, kn, vn, K, Vt, ref


def _run(q, kn, vn, K, Vt, lens, dev, flags=None):
  from gill_amd import ops
  Kd, Vd = K.to(dev, torch.bfloat16).contiguous(), Vt.to(dev, torch.bfloat16).contiguous()
  o = ops.attention_decode(q.to(dev, torch.bfloat16), kn.to(dev, torch.bfloat16), vn.to(dev, torch.bfloat16), Kd, Vd,
                           torch.tensor(lens, dtype=torch.int32, device=dev), flags)
  torch.cuda.synchronize()
  return o.float().cpu(), Kd.float().cpu(), Vd.float().cpu()


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("B,H,d", SHAPES)
def test_attention_decode_accuracy_append_and_batch_independence(cuda, B, H, d, pitch):
  worst = 0.0
  for gi, lens in enumerate(_groups(B, pitch, rot=SHAPES.index((B, H, d)) * 5)):
    q, kn, vn, K, Vt, ref = _case(B, H, d, pitch, lens, seed=50 + gi, dev=cuda)
    o, K2, Vt2 = _run(q, kn, vn, K, Vt, lens, cuda)
    assert torch.isfinite(o).all(), f"lens {lens}: non-finite output (a stale slot was read as data)"
    # report_rows takes (B, rows, C) and reports per row: here one row per batch entry
    rel = U.report_rows(f"attention_decode B{B} H{H} d{d} pitch {pitch} lens {lens}", o[None], ref[None])
    worst = max(worst, rel)
    assert rel < U.ATTN_BAR, (lens, rel)
    # append: the new slot bit for bit, nothing else moved
    wantK, wantV = K.clone(), Vt.clone()
    for b, n in enumerate(lens):
      wantK[b, :, n] = kn[b].view(H, d)
      wantV[b, :, :d, n] = vn[b].view(H, d)
      if Vt.shape[2] > d:
        wantV[b, :, d, n] = 1.0
    assert torch.equal(K2, wantK), f"lens {lens}: K changed outside the appended slot, or the slot differs from the input"
    assert torch.equal(Vt2, wantV), f"lens {lens}: V^T changed outside the appended slot, or the slot differs from the input"
    # every row alone
    if B > 1:
      for b, n in enumerate(lens):
        ob, _, _ = _run(q[b:b + 1], kn[b:b + 1], vn[b:b + 1], K[b:b + 1], Vt[b:b + 1], [n], cuda)
        assert torch.equal(ob[0], o[b]), f"lens {lens}: row {b} alone differs from its row in the batch by {(ob[0] - o[b]).abs().max().item():.3e}"
  print(f"[attention_decode B{B} H{H} d{d} pitch {pitch}] worst row figure {worst:.3e} (bar {U.ATTN_BAR})")


@pytest.mark.parametrize("B,H,d,pitch", [(5, 12, 64, 96), (5, 32, 80, 96), (5, 32, 128, 320)])
def test_attention_decode_clamps_lengths_beyond_the_cache(cuda, B, H, d, pitch):
  from gill_amd import ops
  dpv = (d + 31) // 32 * 32
  good = [3, 33]
  lens = [pitch, good[0], pitch + 1000, -5, good[1]]
  inside = [min(max(n, 0), pitch - 1) for n in lens]
  q, kn, vn, K, Vt, _ = _case(B, H, d, pitch, inside, seed=90, dev=cuda)
  fill = 7.0
  bigK, Kd = _guarded((B, H, pitch, d), fill, cuda)
  bigV, Vd = _guarded((B, H, dpv, pitch), fill, cuda)
  Kd.copy_(K)
  Vd.copy_(Vt)
  flags = torch.zeros(B, dtype=torch.int32, device=cuda)
  o = ops.attention_decode(q.to(cuda, torch.bfloat16), kn.to(cuda, torch.bfloat16), vn.to(cuda, torch.bfloat16), Kd, Vd,
                           torch.tensor(lens, dtype=torch.int32, device=cuda), flags)
  torch.cuda.synchronize()
  assert flags.cpu().tolist() == [1, 0, 1, 1, 0]
  assert _guards_intact(bigK, fill) and _guards_intact(bigV, fill), "a clamped row wrote outside the caches"
  assert torch.isfinite(o.float()).all()
  # the clamped rows wrote the slot they were clamped to, nothing else; the unclamped rows are what they are alone
  wantK, wantV = K.clone(), Vt.clone()
  for b, n in enumerate(inside):
    wantK[b, :, n] = kn[b].view(H, d)
    wantV[b, :, :d, n] = vn[b].view(H, d)
    if dpv > d:
      wantV[b, :, d, n] = 1.0
  assert torch.equal(Kd.float().cpu(), wantK) and torch.equal(Vd.float().cpu(), wantV)
  for b in (1, 4):
    ob, _, _ = _run(q[b:b + 1], kn[b:b + 1], vn[b:b + 1], K[b:b + 1], Vt[b:b + 1], [lens[b]], cuda)
    assert torch.equal(ob[0], o[b].float().cpu())
