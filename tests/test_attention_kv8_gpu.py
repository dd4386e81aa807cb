"""ops.attention_extend_kv8 and ops.attention_decode_kv8 (the ragged extend and the decode step with append on an e4m3 KV cache:
csrc/attention_extend_kv8.hip, csrc/attention_decode_kv8.hip) on the MI355X.

Shapes, pitches, counts, lengths and the dealing of (count, length) rows into calls are those of test_attention_extend_gpu.py.  Operands are
kv8_util.attn_operands (kv_cache_util.decode_attn_inputs with per-token powers of two on the key and value rows: neighbouring slots, and a slot's
key and value, have different exponents); the new tokens of heads 0 and 1 carry the quantiser's edge rows (kv8_util.EDGE_ROWS: an all-zero row,
a maximum of exactly 448 * 2^e and one bf16 step above it, a row whose other elements fall among the subnormal codes, a row with one element
2^20 times the rest).  The cached slots hold the reference quantiser's codes and exponents; every other slot of the four buffers (K8, Vt8
with its rows d .. round_up(d, 32) - 1, Kexp, Vexp) holds stale bytes of every pattern, the two NaN codes 0x7f / 0xff in every stale row, and
stale exponents of +-127.  Checked per call:

  accuracy       against fp64 on the DEQUANTISED operands, the new tokens' own quantised rows included (kv8_util.attention_ref), with
                 kv_cache_util.report_rows' figure per packed row below ATTN_BAR = 2e-2: the operand values are exact, so the arithmetic on them
                 is what that bar was set for;
  append         the slots n .. n + count - 1 hold the reference quantiser's bytes (modulo the sign bit of a zero code; the values with ==) and
                 exponents, and nothing else in the four buffers moved;
  independence   every row alone at B = 1, and the same rows packed in the reverse order, give the same output and cache bits;
  handover       ops.attention_decode_kv8 on the resulting cache at n + count (one further token; a row with no new tokens: the decode step at
                 n) meets the bar, appends the reference's codes, and gives the same bits for a row alone;
  tie            kv8_util.tie_operands, through both kernels: the inputs at which a token's own key left unquantised would show;
  clamp          lengths beyond the cache set the row's flag, guard words around all five buffers stay intact, unclamped rows keep their bits;
  bad arguments  launch nothing."""
import pytest
import torch

import kv8_util as K8
import kv_cache_util as U
from test_attention_extend_gpu import PITCHES, SHAPES, _calls

pytestmark = pytest.mark.gpu
GUARD = 256
BUFS = ("K8", "Vt8", "Kexp", "Vexp")


def _row(H, d, pitch, cnt, n, seed, tie=False):
  """One sequence on the host: the new tokens' q, k, v (cnt, H*d), the handover token's (1, H*d), the four cache buffers with slots < n
  holding the reference's codes and everything else stale, the fp64 references, and the reference's codes of every token."""
  dpv = (d + 31) // 32 * 32
  nq, nkv = cnt + 1, n + cnt + 1
  if tie:
    q, k, v = K8.tie_operands(H, d, seed)
    if cnt == 1:      # the tie is the extend's token: any further token for the handover
      q, k, v = (torch.cat([t, x]) for t, x in zip((q, k, v), K8.attn_operands(H, 1, 1, d, seed)))
  else:
    q, k, v = K8.attn_operands(H, nq, nkv, d, seed * 131 + 7)
    K8.plant_edge_rows(k, v, H, d, n, seed)
  kq, ke = K8.quantise_heads(k, H, d)
  vq, ve = K8.quantise_heads(v, H, d)
  ref = K8.attention_ref(q, kq, ke, vq, ve, H, d)
  g = torch.Generator().manual_seed(seed + 77)
  Kb = torch.randint(0, 256, (H, pitch, d), generator=g, dtype=torch.int32).to(torch.uint8)
  Vb = torch.randint(0, 256, (H, dpv, pitch), generator=g, dtype=torch.int32).to(torch.uint8)
  Kb[:, :, 0], Kb[:, :, 1] = 0x7f, 0xff                  # both NaN codes in every stale key row
  Vb[:, 0], Vb[:, 1] = 0x7f, 0xff                        # and in every stale value column
  sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -127, 127).to(torch.int8)   # noqa: E731
  Ke, Ve = sign((H, pitch)), sign((H, pitch))
  kb, vb = kq.view(torch.uint8), vq.view(torch.uint8)
  Kb[:, :n], Ke[:, :n] = kb[:, :n], ke[:, :n]
  Vb[:, :d, :n], Ve[:, :n] = vb[:, :n].transpose(1, 2), ve[:, :n]
  return dict(cnt=cnt, n=n, q=q[:cnt], k=k[n:n + cnt], v=v[n:n + cnt], K8=Kb, Vt8=Vb, Kexp=Ke, Vexp=Ve, ref=ref[:cnt],
              q1=q[cnt:], k1=k[n + cnt:], v1=v[n + cnt:], ref1=ref[cnt:], kb=kb, ke=ke, vb=vb, ve=ve)


def _bf(t, dev):
  return t.to(dev, torch.bfloat16).contiguous()


def _cache(rows, dev):
  return [torch.stack([r[x] for r in rows]).to(dev).contiguous() for x in BUFS]


def _host(bufs):
  return [b.cpu() for b in bufs]


def _extend(rows, dev, lens=None, flags=None):
  """One extend call over `rows` in the given order -> per-row outputs, the four buffers on the host, and on the device."""
  from gill_amd import ops
  counts = [r["cnt"] for r in rows]
  cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=dev)
  bufs = _cache(rows, dev)
  qkv = _bf(torch.cat([torch.cat([r[x] for r in rows]) for x in ("q", "k", "v")], dim=1), dev)      # the three thirds of one projection
  hd = qkv.shape[1] // 3
  lens_t = torch.tensor([r["n"] for r in rows] if lens is None else lens, dtype=torch.int32, device=dev)
  o = ops.attention_extend_kv8(qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:], *bufs, lens_t, cu, max(max(counts), 1), flags)
  torch.cuda.synchronize()
  return list(o.float().cpu().split(counts)), _host(bufs), bufs


def _decode(rows, bufs, lens, dev, flags=None):
  from gill_amd import ops
  o = ops.attention_decode_kv8(*(_bf(torch.cat([r[x] for r in rows]), dev) for x in ("q1", "k1", "v1")), *bufs,
                               torch.tensor(lens, dtype=torch.int32, device=dev), flags)
  torch.cuda.synchronize()
  return o.float().cpu()


def _appended(r, d, lo, hi, n=None):
  """The four buffers of row r with the reference's codes of its tokens lo .. hi - 1 (counted from r's first new token) at slots n + lo .."""
  n = r["n"] if n is None else n
  a, b = r["n"] + lo, r["n"] + hi
  want = [r[x].clone() for x in BUFS]
  want[0][:, n + lo:n + hi] = r["kb"][:, a:b]
  want[1][:, :d, n + lo:n + hi] = r["vb"][:, a:b].transpose(1, 2)
  want[2][:, n + lo:n + hi] = r["ke"][:, a:b]
  want[3][:, n + lo:n + hi] = r["ve"][:, a:b]
  return want


def _same_cache(got, want):
  """bytes modulo the sign of a zero code (and with them the values), exponents exactly"""
  norm = lambda t: torch.where(t == 0x80, torch.zeros_like(t), t)   # noqa: E731
  return all(torch.equal(norm(g), norm(w)) for g, w in zip(got[:2], want[:2])) and all(torch.equal(g, w) for g, w in zip(got[2:], want[2:]))


def _check_call(tag, rows, H, d, pitch, cuda, independence):
  outs, host, bufs = _extend(rows, cuda)
  B = len(rows)
  for b, r in enumerate(rows):
    assert torch.isfinite(outs[b]).all(), f"{tag}: row {b}: non-finite output (a stale slot was read as data)"
    assert _same_cache([h[b] for h in host], _appended(r, d, 0, r["cnt"])), \
      f"{tag}: row {b}: a new slot differs from the reference quantiser, or something outside the new slots moved"
    # the values with ==: codes x 2^e of the new slots
    n, c = r["n"], r["cnt"]
    got_k = K8.dequantise_rows(host[0][b][:, n:n + c].view(torch.float8_e4m3fn), host[2][b][:, n:n + c])
    want_k = K8.dequantise_rows(r["kb"][:, n:n + c].view(torch.float8_e4m3fn), r["ke"][:, n:n + c])
    assert bool((got_k == want_k).all()), f"{tag}: row {b}: a stored key differs in value"
  worst = worst1 = 0.0
  got, ref = torch.cat(outs), torch.cat([r["ref"] for r in rows])
  if got.shape[0]:
    worst = U.report_rows(tag, got[None], ref[None])
    assert worst < U.ATTN_BAR, (tag, worst)
  if independence and B > 1:
    for b, r in enumerate(rows):
      ob, hb, _ = _extend([r], cuda)
      assert torch.equal(ob[0], outs[b]), f"{tag}: row {b} alone differs from its row in the pack"
      assert all(torch.equal(x[0], y[b]) for x, y in zip(hb, host)), f"{tag}: row {b} alone leaves another cache"
    orv, hrv, _ = _extend(rows[::-1], cuda)
    for b in range(B):
      assert torch.equal(orv[B - 1 - b], outs[b]), f"{tag}: row {b} differs when the pack is reversed"
      assert all(torch.equal(x[B - 1 - b], y[b]) for x, y in zip(hrv, host)), f"{tag}: row {b}: cache differs when the pack is reversed"
  # handover: one further token through the decode kernel on the cache the extend left (rows that still have a free slot)
  fits = [b for b, r in enumerate(rows) if r["n"] + r["cnt"] <= pitch - 1]
  lens1 = [min(r["n"] + r["cnt"], pitch - 1) for r in rows]
  alone = {b: [x[b:b + 1].clone() for x in bufs] for b in fits[:2]} if independence else {}
  o1 = _decode(rows, bufs, lens1, cuda)
  host1 = _host(bufs)
  if fits:
    assert torch.isfinite(o1[fits]).all(), f"{tag}: decode: non-finite output"
    worst1 = U.report_rows(tag + " -> attention_decode_kv8", o1[fits][None], torch.cat([rows[b]["ref1"] for b in fits])[None])
    assert worst1 < U.ATTN_BAR, (tag, worst1)
    for b in fits:
      r = rows[b]
      assert _same_cache([h[b] for h in host1], _appended(r, d, 0, r["cnt"] + 1)), \
        f"{tag}: decode row {b}: the new slot differs from the reference quantiser, or something else moved"
    for b, bb in alone.items():
      ob = _decode([rows[b]], bb, [lens1[b]], cuda)
      assert torch.equal(ob[0], o1[b]), f"{tag}: decode row {b} alone differs from its row in the batch"
      assert all(torch.equal(x[0].cpu(), y[b]) for x, y in zip(bb, host1)), f"{tag}: decode row {b} alone leaves another cache"
  return worst, worst1


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("B,H,d", SHAPES)
def test_attention_kv8_accuracy_append_independence_and_handover(cuda, B, H, d, pitch):
  worst = worst1 = 0.0
  for ci, call in enumerate(_calls(B, pitch, rot=SHAPES.index((B, H, d)) * 2)):
    tag = f"attention_extend_kv8 B{B} H{H} d{d} pitch {pitch} (count, len) {call}"
    rows = [_row(H, d, pitch, c, n, seed=300 + 17 * ci + b) for b, (c, n) in enumerate(call)]
    w, w1 = _check_call(tag, rows, H, d, pitch, cuda, independence=True)
    worst, worst1 = max(worst, w), max(worst1, w1)
  print(f"[attention_kv8 B{B} H{H} d{d} pitch {pitch}] worst row figure {worst:.3e}, handover {worst1:.3e} (bar {U.ATTN_BAR})")


@pytest.mark.parametrize("H,d", [(12, 64), (32, 80), (32, 128)])
def test_attention_kv8_the_own_token_is_quantised_before_it_is_used(cuda, H, d):
  """tie_operands: extend of the second token (count 1 at length 1), and the same token through the decode kernel (count 0, handover at 1)."""
  ext = _row(H, d, 96, 1, 1, seed=900 + d, tie=True)
  dec = _row(H, d, 96, 0, 1, seed=900 + d, tie=True)
  w, _ = _check_call(f"attention_extend_kv8 tie H{H} d{d}", [ext], H, d, 96, cuda, independence=False)
  _, w1 = _check_call(f"attention_decode_kv8 tie H{H} d{d}", [dec], H, d, 96, cuda, independence=False)
  print(f"[attention_kv8 tie H{H} d{d}] extend {w:.3e}, decode {w1:.3e} (bar {U.ATTN_BAR})")


def _guarded(shape, fill, dev, dtype):
  n = 1
  for s in shape:
    n *= s
  big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
  return big, big[GUARD:GUARD + n].view(shape)


def _guards_intact(big, fill):
  return bool((torch.cat([big[:GUARD], big[-GUARD:]]).float() == fill).all())


def _guarded_cache(rows, B, H, d, pitch, cuda):
  dpv = (d + 31) // 32 * 32
  shapes = ((B, H, pitch, d), (B, H, dpv, pitch), (B, H, pitch), (B, H, pitch))
  bigs, views = zip(*[_guarded(s, 7, cuda, torch.uint8 if i < 2 else torch.int8) for i, s in enumerate(shapes)])
  for v, x in zip(views, BUFS):
    v.copy_(torch.stack([r[x] for r in rows]))
  return bigs, list(views)


@pytest.mark.parametrize("H,d,pitch,counts", [(12, 64, 96, (17, 16, 33, 1, 15)), (32, 80, 96, (64, 0, 16, 33, 17)),
                                              (32, 128, 320, (33, 64, 17, 15, 1))])
def test_attention_extend_kv8_clamps_lengths_beyond_the_cache(cuda, H, d, pitch, counts):
  from gill_amd import ops
  B = 5
  lens = [pitch, 3, pitch - counts[2] + 1, -5, 33]
  inside = [min(max(n, 0), pitch - c) for n, c in zip(lens, counts)]
  rows = [_row(H, d, pitch, c, n, seed=390 + b) for b, (c, n) in enumerate(zip(counts, inside))]
  total = sum(counts)
  bigs, bufs = _guarded_cache(rows, B, H, d, pitch, cuda)
  q, kn, vn = (_bf(torch.cat([r[x] for r in rows]), cuda) for x in ("q", "k", "v"))
  cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32, device=cuda)
  flags = torch.zeros(B, dtype=torch.int32, device=cuda)
  o = ops.attention_extend_kv8(q, kn, vn, *bufs, torch.tensor(lens, dtype=torch.int32, device=cuda), cu, max(counts), flags)
  torch.cuda.synchronize()
  assert flags.cpu().tolist() == [1, 0, 1, 1, 0]
  assert all(_guards_intact(b, 7) for b in bigs), "a clamped row wrote outside a buffer"
  outs = list(o.float().cpu().split(list(counts)))
  assert all(torch.isfinite(x).all() for x in outs)
  host = _host(bufs)
  for b, r in enumerate(rows):      # the clamped rows wrote the slots they were clamped to, nothing else
    assert _same_cache([h[b] for h in host], _appended(r, d, 0, r["cnt"], inside[b])), f"row {b}"
  for b in (1, 4):                  # the unclamped rows are what they are alone
    ob, _, _ = _extend([rows[b]], cuda)
    assert torch.equal(ob[0], outs[b])


@pytest.mark.parametrize("H,d,pitch", [(12, 64, 96), (32, 80, 96), (32, 128, 320)])
def test_attention_decode_kv8_clamps_lengths_beyond_the_cache(cuda, H, d, pitch):
  B = 5
  lens = [pitch, 3, pitch + 1000, -5, 33]
  inside = [min(max(n, 0), pitch - 1) for n in lens]
  rows = [_row(H, d, pitch, 0, n, seed=490 + b) for b, n in enumerate(inside)]
  bigs, bufs = _guarded_cache(rows, B, H, d, pitch, cuda)
  flags = torch.zeros(B, dtype=torch.int32, device=cuda)
  o = _decode(rows, bufs, lens, cuda, flags)
  assert flags.cpu().tolist() == [1, 0, 1, 1, 0]
  assert all(_guards_intact(b, 7) for b in bigs), "a clamped row wrote outside a buffer"
  assert torch.isfinite(o).all()
  host = _host(bufs)
  for b, r in enumerate(rows):
    assert _same_cache([h[b] for h in host], _appended(r, d, 0, 1)), f"row {b}"
  for b in (1, 4):
    ob = _decode([rows[b]], _cache([rows[b]], cuda), [lens[b]], cuda)
    assert torch.equal(ob[0], o[b])


def test_attention_kv8_bad_arguments_launch_nothing(cuda):
  from gill_amd import _native as N
  B, H, d, pitch, total = 2, 12, 64, 96, 20
  mk = lambda *shape: torch.full(shape, 3.0, dtype=torch.bfloat16, device=cuda)   # noqa: E731
  mk8 = lambda dt, *shape: torch.full(shape, 3, dtype=dt, device=cuda)   # noqa: E731
  n = total * H * d + 16
  q, kn, vn, o = mk(n), mk(n), mk(n), mk(n)
  K8b, V8b = mk8(torch.uint8, B * H * pitch * d + 16), mk8(torch.uint8, B * H * d * pitch + 16)
  Ke, Ve = mk8(torch.int8, B * H * pitch + 16), mk8(torch.int8, B * H * pitch + 16)
  lens = torch.tensor([5, 9], dtype=torch.int32, device=cuda)
  cu = torch.tensor([0, 3, total], dtype=torch.int32, device=cuda)
  p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

  def ext(q=q, kn=kn, vn=vn, K8b=K8b, V8b=V8b, Ke=Ke, Ve=Ve, o=o, max_new=17, H=H, d=d, pitch=pitch, ld=H * d):
    return N.lib().gill_attention_extend_kv8(p(q), p(kn), p(vn), ld, p(K8b), p(V8b), p(Ke), p(Ve), p(lens), p(cu), p(o), B, total, max_new, H, d,
                                             pitch, None, N.current_stream())

  def dec(q=q, kn=kn, vn=vn, K8b=K8b, V8b=V8b, Ke=Ke, Ve=Ve, o=o, H=H, d=d, pitch=pitch, ld=H * d):
    return N.lib().gill_attention_decode_kv8(p(q), p(kn), p(vn), ld, p(K8b), p(V8b), p(Ke), p(Ve), p(lens), p(o), B, H, d, pitch, None,
                                             N.current_stream())

  for name, call in (("extend", ext), ("decode", dec)):
    assert call(q=q[1:]) != 0, f"{name}: misaligned q accepted"
    assert call(kn=kn[1:]) != 0, f"{name}: misaligned k_new accepted"
    assert call(vn=vn[1:]) != 0, f"{name}: misaligned v_new accepted"
    assert call(K8b=K8b[1:]) != 0, f"{name}: misaligned K8 accepted"
    assert call(V8b=V8b[8:]) != 0, f"{name}: misaligned Vt8 accepted"
    assert call(Ke=None) != 0 and call(Ve=None) != 0, f"{name}: a null exponent buffer accepted"
    assert call(H=16, d=48) != 0, f"{name}: head dim 48 accepted"
    assert call(pitch=80) != 0, f"{name}: pitch 80 accepted"
    assert call(ld=H * d + 4) != 0, f"{name}: row stride that breaks the 16-byte alignment accepted"
  assert ext(max_new=0) != 0 and ext(max_new=-1) != 0 and ext(max_new=pitch + 1) != 0, "extend: max_new outside 1 .. pitch accepted"
  assert ext(Ke=Ke[1:]) != 0 and ext(Ve=Ve[2:]) != 0, "extend: a misaligned exponent buffer accepted"
  assert ext(o=o[1:]) != 0, "extend: misaligned o accepted"
  torch.cuda.synchronize()
  assert bool((o.float() == 3.0).all()) and all(bool((t == 3).all()) for t in (K8b, V8b, Ke, Ve)), "a refused call wrote something"
  assert ext() == 0 and dec() == 0
  torch.cuda.synchronize()
