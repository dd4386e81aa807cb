"""ops.attention_append (gill_attention_append: nq consecutive new tokens per row against that row's own cache length, with append) on the
MI355X.

Inputs are built as test_attention_decode_gpu._case builds them: kv_cache_util.decode_attn_inputs (peaked scores, every new key leaning to
its query), one sequence per row, the cache beyond each length filled with finite LARGE stale values (+-1e30) in K and V^T.  Per
(B, H, d), pitch and nq, the rows take different lengths from LENGTHS and pitch - nq (those with n + nq <= pitch), in groups of B until every
length has been a row.  Checked per group:

  sequential identity  output and both caches equal, bit for bit, nq successive ops.attention_decode calls on the same operands, the i-th at
                       lens + i (nq == 1: one call);
  accuracy             against fp64 on the same bf16 operands, kv_cache_util.report_rows' figure per row, at ATTN_BAR = 2e-2;
  append               slots n .. n + nq - 1 of K and V^T hold the inputs bit for bit and nothing else in either cache moved (d = 80: the
                       ones-row entry Vt[b][h][d][n + i] is 1.0 for each appended slot);
  batch independence   every row alone at B = 1 gives the bits it has in the batch;
  clamp                lengths pitch, pitch - nq + 1 and -5 set the row's flag, guard words around both caches and the output stay
                       intact, the unclamped rows keep their bits;
  bad arguments        nq 0 or 17, a misaligned pointer and an unsupported d are errors that launch nothing."""
import pytest
import torch

import kv_cache_util as U
from test_attention_decode_gpu import STALE, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 128), (3, 12, 64), (2, 32, 80)]
PITCHES = (96, 320)
NQS = (1, 2, 8, 16)
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128)


def _lengths(pitch, nq):
  ls = [n for n in LENGTHS if n + nq <= pitch]
  return ls if pitch - nq in ls else ls + [pitch - nq]


def _groups(B, pitch, nq, rot):
  ls = _lengths(pitch, nq)
  ls = ls[rot % len(ls):] + ls[:rot % len(ls)]
  ls = ls + ls[:(-len(ls)) % B]
  return [ls[i:i + B] for i in range(0, len(ls), B)]


def _case(B, H, d, pitch, nq, lens, seed):
  """Host tensors of one batch: q, k_new, v_new (B, nq, H*d); K (B,H,pitch,d), Vt (B,H,dpv,pitch) with stale values from each length on;
  the fp64 reference (B, nq, H*d): token i of row b sees the keys 0 .. lens[b] + i."""
  dpv = (d + 31) // 32 * 32
  g = torch.Generator().manual_seed(seed)
  sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -STALE, STALE)   # noqa: E731
  K, Vt = U.bf(sign((B, H, pitch, d))), U.bf(sign((B, H, dpv, pitch)))
  q, kn, vn, ref = (torch.empty(B, nq, H * d) for _ in range(4))
  for b, n in enumerate(lens):
    qb, kb, vb = U.decode_attn_inputs(1, H, nq, n + nq, d, seed=seed * 131 + b)
    q[b], kn[b], vn[b] = qb[0], kb[0, n:], vb[0, n:]
    kh = kb[0].view(n + nq, H, d).transpose(0, 1)          # (H, n + nq, d)
    vh = vb[0].view(n + nq, H, d).transpose(0, 1)
    K[b, :, :n] = kh[:, :n]
    Vt[b, :, :d, :n] = vh[:, :n].transpose(1, 2)
    s = (qb[0].view(nq, H, d).transpose(0, 1).double() @ kh.double().transpose(1, 2)) * d ** -0.5      # (H, nq, n + nq)
    vis = torch.arange(n + nq)[None, :] <= (torch.arange(nq)[:, None] + n)
    s = s.masked_fill(~vis, float("-inf"))
    ref[b] = (s.softmax(-1) @ vh.double()).transpose(0, 1).reshape(nq, H * d).float()
  return q, kn, vn, K, Vt, ref


def _dev(t, dev):
  return t.to(dev, torch.bfloat16).contiguous()


def _append(q, kn, vn, K, Vt, lens, dev, flags=None):
  from gill_amd import ops
  Kd, Vd = _dev(K, dev), _dev(Vt, dev)
  o = ops.attention_append(_dev(q, dev), _dev(kn, dev), _dev(vn, dev), Kd, Vd, torch.tensor(lens, dtype=torch.int32, device=dev), flags)
  torch.cuda.synchronize()
  return o.float().cpu(), Kd.float().cpu(), Vd.float().cpu()


def _sequential(q, kn, vn, K, Vt, lens, dev):
  """nq successive single-token calls on one pair of caches, the i-th at lens + i."""
  from gill_amd import ops
  Kd, Vd = _dev(K, dev), _dev(Vt, dev)
  outs = []
  for i in range(q.shape[1]):
    outs.append(ops.attention_decode(_dev(q[:, i], dev), _dev(kn[:, i], dev), _dev(vn[:, i], dev), Kd, Vd,
                                     torch.tensor([n + i for n in lens], dtype=torch.int32, device=dev)))
  torch.cuda.synchronize()
  return torch.stack(outs, 1).float().cpu(), Kd.float().cpu(), Vd.float().cpu()


def _appended(K, Vt, kn, vn, lens, H, d):
  wantK, wantV = K.clone(), Vt.clone()
  nq = kn.shape[1]
  for b, n in enumerate(lens):
    wantK[b, :, n:n + nq] = kn[b].view(nq, H, d).transpose(0, 1)
    wantV[b, :, :d, n:n + nq] = vn[b].view(nq, H, d).permute(1, 2, 0)
    if Vt.shape[2] > d:
      wantV[b, :, d, n:n + nq] = 1.0
  return wantK, wantV


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("B,H,d", SHAPES)
def test_attention_append_identity_accuracy_append_and_batch_independence(cuda, B, H, d, pitch, nq):
  worst = 0.0
  for gi, lens in enumerate(_groups(B, pitch, nq, rot=SHAPES.index((B, H, d)) * 5 + nq)):
    q, kn, vn, K, Vt, ref = _case(B, H, d, pitch, nq, lens, seed=150 + gi)
    o, K2, Vt2 = _append(q, kn, vn, K, Vt, lens, cuda)
    assert torch.isfinite(o).all(), f"lens {lens}: non-finite output (a stale slot was read as data)"
    # sequential identity
    os_, Ks, Vs = _sequential(q, kn, vn, K, Vt, lens, cuda)
    assert torch.equal(o, os_), f"lens {lens}: differs from {nq} single-token calls by {(o - os_).abs().max().item():.3e}"
    assert torch.equal(K2, Ks) and torch.equal(Vt2, Vs), f"lens {lens}: the caches differ from those of {nq} single-token calls"
    # accuracy, per row
    rel = U.report_rows(f"attention_append B{B} H{H} d{d} pitch {pitch} nq {nq} lens {lens}", o.reshape(1, B * nq, H * d),
                        ref.reshape(1, B * nq, H * d))
    worst = max(worst, rel)
    assert rel < U.ATTN_BAR, (lens, rel)
    # append: the new slots bit for bit, nothing else moved
    wantK, wantV = _appended(K, Vt, kn, vn, lens, H, d)
    assert torch.equal(K2, wantK), f"lens {lens}: K changed outside the appended slots, or a slot differs from the input"
    assert torch.equal(Vt2, wantV), f"lens {lens}: V^T changed outside the appended slots, or a slot differs from the input"
    # every row alone
    if B > 1:
      for b, n in enumerate(lens):
        ob, _, _ = _append(q[b:b + 1], kn[b:b + 1], vn[b:b + 1], K[b:b + 1], Vt[b:b + 1], [n], cuda)
        assert torch.equal(ob[0], o[b]), f"lens {lens}: row {b} alone differs from its row in the batch by {(ob[0] - o[b]).abs().max().item():.3e}"
  print(f"[attention_append B{B} H{H} d{d} pitch {pitch} nq {nq}] worst row figure {worst:.3e} (bar {U.ATTN_BAR})")


def _raw_call(q, kn, vn, Kd, Vd, lens, o, B, nq, H, d, pitch, flags):
  from gill_amd import _native as N
  return N.lib().gill_attention_append(q.data_ptr(), kn.data_ptr(), vn.data_ptr(), H * d, Kd.data_ptr(), Vd.data_ptr(), lens.data_ptr(),
                                       o.data_ptr(), B, nq, H, d, pitch, None if flags is None else flags.data_ptr(), N.current_stream())


@pytest.mark.parametrize("B,H,d,pitch,nq", [(5, 12, 64, 96, 8), (5, 32, 80, 96, 16), (5, 32, 128, 320, 2)])
def test_attention_append_clamps_lengths_beyond_the_cache(cuda, B, H, d, pitch, nq):
  dpv = (d + 31) // 32 * 32
  good = [3, 33]
  lens = [pitch, good[0], pitch - nq + 1, -5, good[1]]
  inside = [min(max(n, 0), pitch - nq) for n in lens]
  q, kn, vn, K, Vt, _ = _case(B, H, d, pitch, nq, inside, seed=190)
  fill = 7.0
  bigK, Kd = _guarded((B, H, pitch, d), fill, cuda)
  bigV, Vd = _guarded((B, H, dpv, pitch), fill, cuda)
  bigO, od = _guarded((B, nq, H * d), fill, cuda)
  Kd.copy_(K)
  Vd.copy_(Vt)
  flags = torch.zeros(B, dtype=torch.int32, device=cuda)
  rc = _raw_call(_dev(q, cuda), _dev(kn, cuda), _dev(vn, cuda), Kd, Vd, torch.tensor(lens, dtype=torch.int32, device=cuda), od, B, nq, H, d,
                 pitch, flags)
  torch.cuda.synchronize()
  assert rc == 0
  assert flags.cpu().tolist() == [1, 0, 1, 1, 0]
  assert _guards_intact(bigK, fill) and _guards_intact(bigV, fill) and _guards_intact(bigO, fill), "a clamped row wrote outside a buffer"
  o = od.float().cpu()
  assert torch.isfinite(o).all()
  # the clamped rows wrote the slots they were clamped to, nothing else; the unclamped rows are what they are alone
  wantK, wantV = _appended(K, Vt, kn, vn, inside, H, d)
  assert torch.equal(Kd.float().cpu(), wantK) and torch.equal(Vd.float().cpu(), wantV)
  for b in (1, 4):
    ob, _, _ = _append(q[b:b + 1], kn[b:b + 1], vn[b:b + 1], K[b:b + 1], Vt[b:b + 1], [lens[b]], cuda)
    assert torch.equal(ob[0], o[b])


def test_attention_append_bad_arguments_launch_nothing(cuda):
  B, H, d, pitch = 2, 12, 64, 96
  mk = lambda *shape: torch.full(shape, 3.0, dtype=torch.bfloat16, device=cuda)   # noqa: E731
  rows = 17 * B * H * d + 16
  q, kn, vn, o = mk(rows), mk(rows), mk(rows), mk(rows)
  Kd, Vd = mk(B, H, pitch, d), mk(B, H, d, pitch)
  lens = torch.tensor([5, 9], dtype=torch.int32, device=cuda)
  for nq in (0, 17, -1):
    assert _raw_call(q, kn, vn, Kd, Vd, lens, o, B, nq, H, d, pitch, None) != 0, f"nq = {nq} accepted"
  assert _raw_call(q[1:], kn, vn, Kd, Vd, lens, o, B, 2, H, d, pitch, None) != 0, "misaligned q accepted"
  assert _raw_call(q, kn[1:], vn, Kd, Vd, lens, o, B, 2, H, d, pitch, None) != 0, "misaligned k_new accepted"
  assert _raw_call(q, kn, vn, Kd.view(-1)[1:], Vd, lens, o, B, 2, H, d, pitch, None) != 0, "misaligned K accepted"
  assert _raw_call(q, kn, vn, Kd, Vd, lens, o.view(-1)[1:], B, 2, H, d, pitch, None) != 0, "misaligned o accepted"
  assert _raw_call(q, kn, vn, Kd, Vd, lens, o, B, 2, 16, 48, pitch, None) != 0, "head dim 48 accepted"
  assert _raw_call(q, kn, vn, Kd, Vd, lens, o, B, 2, H, d, 80, None) != 0, "pitch 80 accepted"
  torch.cuda.synchronize()
  for t in (o, Kd, Vd):
    assert bool((t.float() == 3.0).all()), "a refused call wrote something"
  assert _raw_call(q, kn, vn, Kd, Vd, lens, o, B, 2, H, d, pitch, None) == 0
  torch.cuda.synchronize()
