"""ops.attention_extend (gill_attention_extend: a ragged number of consecutive new tokens per row, packed, against that row's own cache length,
with append) on the MI355X.

Inputs are built as test_attention_append_gpu._case builds them: kv_cache_util.decode_attn_inputs (peaked scores, every new key leaning to its
query), one sequence per row, the cache beyond each length filled with finite LARGE stale values (+-1e30) in K and V^T.  Per (B, H, d) and pitch
the rows are (count, length) pairs: every count of COUNTS with lengths walked through LENGTHS (kept to n + count <= pitch, else the exact fit
n = pitch - count), plus exact fits; counts and lengths sit on both sides of the 16-, 32- and 64-wide edges (the kernel's key tile is 32, a wave
takes 32 queries, the store kernel 64 tokens, a workgroup 128 queries).  The pairs are dealt into calls of B rows, so one call mixes counts
(a row with no new tokens among them).  Checked per call:

  accuracy       against fp64 on the same bf16 operands, kv_cache_util.report_rows' figure per packed row, below ATTN_BAR = 2e-2;
  append         slots n .. n + count - 1 of K and V^T hold the inputs bit for bit (d = 80: the ones-row entry Vt[b][h][d][n + i] is 1.0) and
                 nothing else in either cache moved;
  independence   every row alone at B = 1, and the same rows packed in the reverse order, give the same output and cache bits;
  handover       ops.attention_decode on the resulting cache at n + count (one further token) meets the same bar;
  clamp          lengths pitch, pitch - count + 1 and -5 set the row's flag, guard words around both caches and the output stay intact, the
                 unclamped rows keep their bits;
  bad arguments  an unsupported d, a misaligned pointer and max_new = 0 are errors that launch nothing."""
import pytest
import torch

import kv_cache_util as U
from test_attention_decode_gpu import STALE, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 128), (3, 12, 64), (2, 32, 80)]
PITCHES = (96, 320)
COUNTS = (0, 1, 15, 16, 17, 33, 64)
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127)


def _pairs(pitch, rot):
  """(count, length) rows: two lengths per count, walking LENGTHS so that each is used, then the exact fits of three counts."""
  out = []
  for i, c in enumerate(COUNTS):
    for k in range(2):
      n = LENGTHS[(2 * i + k + rot) % len(LENGTHS)]
      out.append((c, n if n + c <= pitch else pitch - c))
  return out + [(c, pitch - c) for c in (1, 17, 64)]


def _calls(B, pitch, rot):
  ps = _pairs(pitch, rot)
  # neighbours in the list have the same count: deal them with a stride so that a call mixes counts
  stride = 5
  ps = [ps[(j * stride) % len(ps)] for j in range(len(ps))]       # len(ps) = 17: 5 is coprime, a permutation
  ps = ps + ps[:(-len(ps)) % B]
  return [ps[i:i + B] for i in range(0, len(ps), B)]


def _row(H, d, pitch, cnt, n, seed):
  """One sequence on the host: q, k_new, v_new (cnt, H*d), the handover token's (1, H*d) each, K (H,pitch,d) / Vt (H,dpv,pitch) with stale values
  from slot n on, the fp64 references (cnt, H*d) and (1, H*d)."""
  dpv = (d + 31) // 32 * 32
  g = torch.Generator().manual_seed(seed)
  sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -STALE, STALE)   # noqa: E731
  K, Vt = U.bf(sign((H, pitch, d))), U.bf(sign((H, dpv, pitch)))
  nq, nkv = cnt + 1, n + cnt + 1
  qb, kb, vb = U.decode_attn_inputs(1, H, nq, nkv, d, seed=seed * 131 + 7)
  kh = kb[0].view(nkv, H, d).transpose(0, 1)          # (H, nkv, d)
  vh = vb[0].view(nkv, H, d).transpose(0, 1)
  K[:, :n] = kh[:, :n]
  Vt[:, :d, :n] = vh[:, :n].transpose(1, 2)
  s = (qb[0].view(nq, H, d).transpose(0, 1).double() @ kh.double().transpose(1, 2)) * d ** -0.5      # (H, nq, nkv)
  vis = torch.arange(nkv)[None, :] <= (torch.arange(nq)[:, None] + n)
  ref = (s.masked_fill(~vis, float("-inf")).softmax(-1) @ vh.double()).transpose(0, 1).reshape(nq, H * d).float()
  return dict(cnt=cnt, n=n, q=qb[0, :cnt], k=kb[0, n:n + cnt], v=vb[0, n:n + cnt], K=K, Vt=Vt, ref=ref[:cnt],
              q1=qb[0, cnt:], k1=kb[0, n + cnt:], v1=vb[0, n + cnt:], ref1=ref[cnt:])


def _dev(t, dev):
  return t.to(dev, torch.bfloat16).contiguous()


def _extend(rows, dev, lens=None, flags=None):
  """One call over `rows` in the given order -> per-row outputs, K (B,H,pitch,d) and Vt as host floats, and the device caches."""
  from gill_amd import ops
  counts = [r["cnt"] for r in rows]
  cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=dev)
  Kd, Vd = _dev(torch.stack([r["K"] for r in rows]), dev), _dev(torch.stack([r["Vt"] for r in rows]), dev)
  # the three thirds of one (total, 3 H d) projection, as the engine passes them
  qkv = _dev(torch.cat([torch.cat([r[x] for r in rows]) for x in ("q", "k", "v")], dim=1), dev)
  hd = qkv.shape[1] // 3
  lens_t = torch.tensor([r["n"] for r in rows] if lens is None else lens, dtype=torch.int32, device=dev)
  o = ops.attention_extend(qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:], Kd, Vd, lens_t, cu, max(max(counts), 1), flags)
  torch.cuda.synchronize()
  return list(o.float().cpu().split(counts)), Kd.float().cpu(), Vd.float().cpu(), Kd, Vd


def _appended(r, H, d, n=None):
  n = r["n"] if n is None else n
  c = r["cnt"]
  wantK, wantV = r["K"].clone(), r["Vt"].clone()
  wantK[:, n:n + c] = r["k"].view(c, H, d).transpose(0, 1)
  wantV[:, :d, n:n + c] = r["v"].view(c, H, d).permute(1, 2, 0)
  if wantV.shape[1] > d:
    wantV[:, d, n:n + c] = 1.0
  return wantK, wantV


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("B,H,d", SHAPES)
def test_attention_extend_accuracy_append_independence_and_handover(cuda, B, H, d, pitch):
  from gill_amd import ops
  worst = worst1 = 0.0
  for ci, call in enumerate(_calls(B, pitch, rot=SHAPES.index((B, H, d)) * 2)):
    tag = f"attention_extend B{B} H{H} d{d} pitch {pitch} (count, len) {call}"
    rows = [_row(H, d, pitch, c, n, seed=300 + 17 * ci + b) for b, (c, n) in enumerate(call)]
    outs, K2, Vt2, Kd, Vd = _extend(rows, cuda)
    for b, r in enumerate(rows):
      assert torch.isfinite(outs[b]).all(), f"{tag}: row {b}: non-finite output (a stale slot was read as data)"
      # append: the new slots bit for bit, nothing else moved (a row without new tokens: nothing at all)
      wantK, wantV = _appended(r, H, d)
      assert torch.equal(K2[b], wantK), f"{tag}: row {b}: K changed outside the appended slots, or a slot differs from the input"
      assert torch.equal(Vt2[b], wantV), f"{tag}: row {b}: V^T changed outside the appended slots, or a slot differs from the input"
    got, ref = torch.cat(outs), torch.cat([r["ref"] for r in rows])
    if got.shape[0]:
      rel = U.report_rows(tag, got[None], ref[None])
      worst = max(worst, rel)
      assert rel < U.ATTN_BAR, (call, rel)
    # every row alone, and the rows packed in the reverse order
    if B > 1:
      for b, r in enumerate(rows):
        ob, Kb, Vb, _, _ = _extend([r], cuda)
        assert torch.equal(ob[0], outs[b]), f"{tag}: row {b} alone differs from its row in the pack"
        assert torch.equal(Kb[0], K2[b]) and torch.equal(Vb[0], Vt2[b]), f"{tag}: row {b} alone leaves another cache"
      orv, Krv, Vrv, _, _ = _extend(rows[::-1], cuda)
      for b in range(B):
        assert torch.equal(orv[B - 1 - b], outs[b]), f"{tag}: row {b} differs when the pack is reversed"
        assert torch.equal(Krv[B - 1 - b], K2[b]) and torch.equal(Vrv[B - 1 - b], Vt2[b]), f"{tag}: row {b}: cache differs when the pack is reversed"
    # handover: one further token through the decode kernel on the cache the extend left (rows that still have a free slot)
    fits = [b for b, r in enumerate(rows) if r["n"] + r["cnt"] <= pitch - 1]
    o1 = ops.attention_decode(*(_dev(torch.cat([r[x] for r in rows]), cuda) for x in ("q1", "k1", "v1")), Kd, Vd,
                              torch.tensor([min(r["n"] + r["cnt"], pitch - 1) for r in rows], dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()
    o1 = o1.float().cpu()
    if fits:
      rel1 = U.report_rows(tag + " -> attention_decode", o1[fits][None], torch.cat([rows[b]["ref1"] for b in fits])[None])
      worst1 = max(worst1, rel1)
      assert rel1 < U.ATTN_BAR, (call, rel1)
  print(f"[attention_extend B{B} H{H} d{d} pitch {pitch}] worst row figure {worst:.3e}, handover {worst1:.3e} (bar {U.ATTN_BAR})")


def _raw_call(q, kn, vn, ld, Kd, Vd, lens, cu, o, B, total, max_new, H, d, pitch, flags):
  from gill_amd import _native as N
  return N.lib().gill_attention_extend(q.data_ptr(), kn.data_ptr(), vn.data_ptr(), ld, Kd.data_ptr(), Vd.data_ptr(), lens.data_ptr(),
                                       cu.data_ptr(), o.data_ptr(), B, total, max_new, H, d, pitch,
                                       None if flags is None else flags.data_ptr(), N.current_stream())


@pytest.mark.parametrize("H,d,pitch,counts", [(12, 64, 96, (17, 16, 33, 1, 15)), (32, 80, 96, (64, 0, 16, 33, 17)),
                                              (32, 128, 320, (33, 64, 17, 15, 1))])
def test_attention_extend_clamps_lengths_beyond_the_cache(cuda, H, d, pitch, counts):
  B, dpv = 5, (d + 31) // 32 * 32
  good = [3, 33]
  lens = [pitch, good[0], pitch - counts[2] + 1, -5, good[1]]
  inside = [min(max(n, 0), pitch - c) for n, c in zip(lens, counts)]
  rows = [_row(H, d, pitch, c, n, seed=390 + b) for b, (c, n) in enumerate(zip(counts, inside))]
  total, fill = sum(counts), 7.0
  bigK, Kd = _guarded((B, H, pitch, d), fill, cuda)
  bigV, Vd = _guarded((B, H, dpv, pitch), fill, cuda)
  bigO, od = _guarded((total, H * d), fill, cuda)
  Kd.copy_(torch.stack([r["K"] for r in rows]))
  Vd.copy_(torch.stack([r["Vt"] for r in rows]))
  q, kn, vn = (_dev(torch.cat([r[x] for r in rows]), cuda) for x in ("q", "k", "v"))
  cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=cuda)
  flags = torch.zeros(B, dtype=torch.int32, device=cuda)
  rc = _raw_call(q, kn, vn, H * d, Kd, Vd, torch.tensor(lens, dtype=torch.int32, device=cuda), cu, od, B, total, max(counts), H, d, pitch, flags)
  torch.cuda.synchronize()
  assert rc == 0
  assert flags.cpu().tolist() == [1, 0, 1, 1, 0]
  assert _guards_intact(bigK, fill) and _guards_intact(bigV, fill) and _guards_intact(bigO, fill), "a clamped row wrote outside a buffer"
  outs = list(od.float().cpu().split(list(counts)))
  assert all(torch.isfinite(o).all() for o in outs)
  # the clamped rows wrote the slots they were clamped to, nothing else; the unclamped rows are what they are alone
  K2, Vt2 = Kd.float().cpu(), Vd.float().cpu()
  for b, r in enumerate(rows):
    wantK, wantV = _appended(r, H, d, inside[b])
    assert torch.equal(K2[b], wantK) and torch.equal(Vt2[b], wantV), f"row {b}"
  for b in (1, 4):
    ob, _, _, _, _ = _extend([rows[b]], cuda)
    assert torch.equal(ob[0], outs[b])


def test_attention_extend_bad_arguments_launch_nothing(cuda):
  B, H, d, pitch = 2, 12, 64, 96
  mk = lambda *shape: torch.full(shape, 3.0, dtype=torch.bfloat16, device=cuda)   # noqa: E731
  total = 20
  n = total * H * d + 16
  q, kn, vn, o = mk(n), mk(n), mk(n), mk(n)
  Kd, Vd = mk(B, H, pitch, d), mk(B, H, d, pitch)
  lens = torch.tensor([5, 9], dtype=torch.int32, device=cuda)
  cu = torch.tensor([0, 3, total], dtype=torch.int32, device=cuda)
  call = lambda q=q, kn=kn, vn=vn, Kd=Kd, Vd=Vd, o=o, max_new=17, H=H, d=d, pitch=pitch, ld=H * d: _raw_call(   # noqa: E731
    q, kn, vn, ld, Kd, Vd, lens, cu, o, B, total, max_new, H, d, pitch, None)
  assert call(max_new=0) != 0, "max_new = 0 accepted"
  assert call(max_new=-1) != 0, "max_new = -1 accepted"
  assert call(max_new=pitch + 1) != 0, "max_new beyond the pitch accepted"
  assert call(q=q[1:]) != 0, "misaligned q accepted"
  assert call(kn=kn[1:]) != 0, "misaligned k_new accepted"
  assert call(vn=vn[1:]) != 0, "misaligned v_new accepted"
  assert call(Kd=Kd.view(-1)[1:]) != 0, "misaligned K accepted"
  assert call(Vd=Vd.view(-1)[1:]) != 0, "misaligned Vt accepted"
  assert call(o=o[1:]) != 0, "misaligned o accepted"
  assert call(H=16, d=48) != 0, "head dim 48 accepted"
  assert call(pitch=80) != 0, "pitch 80 accepted"
  assert call(ld=H * d + 4) != 0, "row stride that breaks the 16-byte alignment accepted"
  torch.cuda.synchronize()
  for t in (o, Kd, Vd):
    assert bool((t.float() == 3.0).all()), "a refused call wrote something"
  assert call() == 0
  torch.cuda.synchronize()
