"""ops.attention_fork (gill_attention_fork: packed candidate continuations against the read-only, shared prefix of a cache row, each causal over
its own tokens, nothing appended) on the MI355X.

Inputs come from kv_cache_util.decode_attn_inputs as in test_attention_extend_gpu._row (peaked scores, every own key leaning to its query): one
draw per cache row for the prefix, one per candidate for its q / k / v.  A cache has Bc rows that candidates name plus one that none names.  Per
(Bc, H, d) and pitch the candidates are (count, plen) pairs: every count of COUNTS with two prefix lengths walked through PLENS, plus counts at
plen = pitch; both sit on both sides of the 32-wide key tile, a wave's 32 queries and a workgroup's 128.  The pairs are dealt into calls of at
most five candidates per parent, parents unsorted, so one call mixes counts (an empty candidate among them) and siblings with different plen.
Slots of a row at or beyond the LARGEST plen of its candidates hold +-1e30 in one run and bf16 NaN / Inf bit patterns in another; the slots
between a sibling's smaller plen and that hold the row's real (finite) keys, which the sibling must not see either.  Checked per call:

  accuracy       against fp64 on the same bf16 operands, kv_cache_util.report_rows' figure per packed row, below ATTN_BAR = 2e-2;
  read-only      K and Vt are bit-identical after the call; guard words around both caches, the output and the workspace are intact;
  independence   every candidate alone at C = 1, the pack reversed, a candidate beside other siblings (every second one dropped) and the same
                 prefixes at other cache row indices give the same output bits;
  agreement      a candidate's output meets the same bar against ops.attention_extend on a scratch copy of its parent row (no bit comparison);
  clamps         plen -5 and pitch + 1, parent -1 and Bc, a count above max_new: flagged, the unflagged candidates keep their bits, emptied
                 candidates store nothing, nothing outside the buffers is touched;
  bad arguments  an unsupported d, a misaligned pointer, max_new < 1 and a negative workspace size are errors that launch nothing."""
import pytest
import torch

import kv_cache_util as U
from test_attention_decode_gpu import GUARD, STALE, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 128), (3, 12, 64), (2, 32, 80)]
PITCHES = (96, 320)
COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 64, 65)
PLENS = (0, 1, 31, 32, 33, 63, 64, 65, None)        # None: the pitch
PER_PARENT = 5
NONFINITE = (0x7FC0, 0xFF80, 0x7F80, 0xFFC1, 0x7FFF)     # bf16 quiet NaN, -Inf, +Inf, NaNs with other payloads / sign
WS_SPARE = 64          # bf16 elements of workspace handed over beyond the query's answer (guarded like the rest)


def _pairs(pitch, rot):
  out = []
  for i, c in enumerate(COUNTS):
    for k in range(2):
      n = PLENS[(2 * i + k + rot) % len(PLENS)]
      out.append((c, pitch if n is None else n))
  return out + [(c, pitch) for c in (1, 33, 65)]


def _calls(Bc, pitch, rot):
  """Lists of (count, plen, parent): at most PER_PARENT candidates per parent and call, parents dealt round robin from the highest index (not
  sorted in the pack), neighbours of the pair list (same count) separated by a stride."""
  ps = _pairs(pitch, rot)
  ps = [ps[(j * 7) % len(ps)] for j in range(len(ps))]       # len(ps) = 23: 7 is coprime, a permutation
  per = PER_PARENT * Bc
  return [[(c, n, (Bc - 1 - j) % Bc) for j, (c, n) in enumerate(ps[i:i + per])] for i in range(0, len(ps), per)]


def _bits(t):
  return t.contiguous().view(torch.int16)


def _stale(shape, kind, g):
  if kind == "large":
    return U.bf(torch.where(torch.rand(shape, generator=g) < 0.5, -STALE, STALE)).bfloat16()
  pat = torch.tensor(NONFINITE, dtype=torch.int32)[torch.randint(0, len(NONFINITE), shape, generator=g)]
  return (pat - (pat >= 32768) * 65536).to(torch.int16).view(torch.bfloat16)      # the 16 bits as they are


def _case(Bc, H, d, pitch, call, seed, kind):
  """Host tensors of one call.  cache rows: parent p lives at row p + 1 of a (Bc + 1)-row cache whose row 0 no candidate names (all stale).
  -> dict(K (Bc+1,H,pitch,d) bf16, Vt, cands: [dict(cnt, n, par, q, k, v (cnt, H*d) float bf16-valued, ref (cnt, H*d))])."""
  dpv = (d + 31) // 32 * 32
  g = torch.Generator().manual_seed(seed)
  K, Vt = _stale((Bc + 1, H, pitch, d), kind, g), _stale((Bc + 1, H, dpv, pitch), kind, g)
  pre = []
  for p in range(Bc):
    top = max([n for _, n, par in call if par == p], default=0)
    _, kb, vb = U.decode_attn_inputs(1, H, 1, max(top, 1), d, seed=seed * 31 + p)
    kh = kb[0].view(-1, H, d).transpose(0, 1)[:, :top]          # (H, top, d)
    vh = vb[0].view(-1, H, d).transpose(0, 1)[:, :top]
    K[p + 1, :, :top] = kh.bfloat16()
    Vt[p + 1, :, :d, :top] = vh.transpose(1, 2).bfloat16()
    pre.append((kh, vh))
  cands = []
  for j, (cnt, n, par) in enumerate(call):
    if cnt:
      qb, kb, vb = U.decode_attn_inputs(1, H, cnt, cnt, d, seed=seed * 131 + 7 + j)
      q, k, v = qb[0], kb[0], vb[0]
      kh = torch.cat([pre[par][0][:, :n], k.view(cnt, H, d).transpose(0, 1)], 1).double()      # (H, n + cnt, d)
      vh = torch.cat([pre[par][1][:, :n], v.view(cnt, H, d).transpose(0, 1)], 1).double()
      s = (q.view(cnt, H, d).transpose(0, 1).double() @ kh.transpose(1, 2)) * d ** -0.5
      vis = torch.arange(n + cnt)[None, :] <= (torch.arange(cnt)[:, None] + n)
      ref = (s.masked_fill(~vis, float("-inf")).softmax(-1) @ vh).transpose(0, 1).reshape(cnt, H * d).float()
    else:
      q = k = v = ref = torch.zeros(0, H * d)
    cands.append(dict(cnt=cnt, n=n, par=par, q=q, k=k, v=v, ref=ref))
  return dict(K=K, Vt=Vt, cands=cands)


def _i32(v, dev):
  return torch.tensor(v, dtype=torch.int32, device=dev)


def _raw(q, kn, vn, ld, Kd, Vd, parent, plen, cu, o, C, Bc, total, max_new, H, d, pitch, flags, ws, ws_bytes):
  from gill_amd import _native as N
  return N.lib().gill_attention_fork(q.data_ptr(), kn.data_ptr(), vn.data_ptr(), ld, Kd.data_ptr(), Vd.data_ptr(), parent.data_ptr(),
                                     plen.data_ptr(), cu.data_ptr(), o.data_ptr(), C, Bc, total, max_new, H, d, pitch,
                                     None if flags is None else flags.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes,
                                     N.current_stream())


def _fork(case, cands, dev, rowmap=None, parents=None, plens=None, max_new=None, flags=None, fill=7.0):
  """One guarded raw call over `cands` in the given order.  rowmap[p]: the cache row index parent p's prefix is put at (default p + 1).
  -> per-candidate outputs (bf16 bit patterns, host), the packed device output, and whether guards and caches came through."""
  from gill_amd import _native as N
  Kh, Vh = case["K"], case["Vt"]
  R, H, pitch, d = Kh.shape
  if rowmap is not None:
    Kp, Vp = Kh.clone(), Vh.clone()
    for p, row in enumerate(rowmap):
      Kp[row], Vp[row] = Kh[p + 1], Vh[p + 1]
    spare = [r for r in range(R) if r not in rowmap]
    Kp[spare[0]], Vp[spare[0]] = Kh[0], Vh[0]
    Kh, Vh = Kp, Vp
  rowmap = rowmap or [p + 1 for p in range(R - 1)]
  counts = [c["cnt"] for c in cands]
  total, C = sum(counts), len(cands)
  mx = max(max(counts), 1) if max_new is None else max_new
  nws = int(N.lib().gill_attention_fork_ws_bytes(C, H, d, mx))
  bigK, Kd = _guarded(tuple(Kh.shape), fill, dev)
  bigV, Vd = _guarded(tuple(Vh.shape), fill, dev)
  bigO, od = _guarded((max(total, 1), H * d), fill, dev)
  bigW, wd = _guarded((nws // 2 + WS_SPARE,), fill, dev)
  Kd.copy_(Kh)
  Vd.copy_(Vh)
  qkv = torch.cat([torch.cat([c[x] for c in cands]) for x in ("q", "k", "v")], dim=1).to(dev, torch.bfloat16).contiguous()
  if total == 0:
    qkv = torch.zeros((1, 3 * H * d), dtype=torch.bfloat16, device=dev)
  hd = H * d
  cu = _i32([0] + torch.tensor(counts).cumsum(0).tolist(), dev)
  par = _i32([rowmap[c["par"]] for c in cands] if parents is None else parents, dev)
  pl = _i32([c["n"] for c in cands] if plens is None else plens, dev)
  rc = _raw(qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:], 3 * hd, Kd, Vd, par, pl, cu, od, C, R, max(total, 1), mx, H, d, pitch, flags, wd,
            wd.numel() * 2)
  torch.cuda.synchronize()
  assert rc == 0, N.lib().gill_last_error()
  ok = (_guards_intact(bigK, fill) and _guards_intact(bigV, fill) and _guards_intact(bigO, fill) and _guards_intact(bigW, fill) and
        bool((wd.float() == fill).all() if nws == 0 else True))
  same = torch.equal(_bits(Kd).cpu(), _bits(Kh)) and torch.equal(_bits(Vd).cpu(), _bits(Vh))
  outs = list(od[:total].cpu().split(counts)) if total else [od[:0].cpu() for _ in counts]
  return outs, ok, same


@pytest.mark.parametrize("kind", ["large", "nonfinite"])
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("Bc,H,d", SHAPES)
def test_attention_fork_accuracy_readonly_independence_and_agreement(cuda, Bc, H, d, pitch, kind):
  from gill_amd import ops
  worst = worst_ext = 0.0
  for ci, call in enumerate(_calls(Bc, pitch, rot=SHAPES.index((Bc, H, d)) * 2)):
    tag = f"attention_fork Bc{Bc} H{H} d{d} pitch {pitch} {kind} (count, plen, parent) {call}"
    case = _case(Bc, H, d, pitch, call, seed=500 + 19 * ci, kind=kind)
    cands = case["cands"]
    outs, ok, same = _fork(case, cands, cuda)
    assert ok, f"{tag}: a guard word around a cache, the output or the workspace changed"
    assert same, f"{tag}: the call wrote the cache"
    for j, o in enumerate(outs):
      assert torch.isfinite(o.float()).all(), f"{tag}: candidate {j}: non-finite output (a slot beyond plen was read as data)"
    got, ref = torch.cat(outs).float(), torch.cat([c["ref"] for c in cands])
    rel = U.report_rows(tag, got[None], ref[None])
    worst = max(worst, rel)
    assert rel < U.ATTN_BAR, (call, rel)
    if kind != "large":
      continue
    # the pack reversed; every second candidate dropped (other siblings); the prefixes at other cache row indices
    orv, _, _ = _fork(case, cands[::-1], cuda)
    for j in range(len(cands)):
      assert torch.equal(_bits(orv[len(cands) - 1 - j]), _bits(outs[j])), f"{tag}: candidate {j} differs when the pack is reversed"
    osub, _, _ = _fork(case, cands[::2], cuda)
    for j in range(0, len(cands), 2):
      assert torch.equal(_bits(osub[j // 2]), _bits(outs[j])), f"{tag}: candidate {j} differs beside other siblings"
    omv, _, same_mv = _fork(case, cands, cuda, rowmap=list(range(Bc)))        # parent p at row p, the unnamed row last
    assert same_mv
    for j in range(len(cands)):
      assert torch.equal(_bits(omv[j]), _bits(outs[j])), f"{tag}: candidate {j} differs when its prefix lies in another cache row"
    # every candidate alone through ops.attention_fork, and ops.attention_extend on a scratch copy of its parent row
    Kd, Vd = case["K"].to(cuda), case["Vt"].to(cuda)
    for j, c in enumerate(cands):
      if not c["cnt"]:
        continue
      q, k, v = (c[x].to(cuda, torch.bfloat16).contiguous() for x in ("q", "k", "v"))
      cu = _i32([0, c["cnt"]], cuda)
      oa = ops.attention_fork(q, k, v, Kd, Vd, _i32([c["par"] + 1], cuda), _i32([c["n"]], cuda), cu, c["cnt"])
      assert torch.equal(_bits(oa.cpu()), _bits(outs[j])), f"{tag}: candidate {j} alone differs from its rows in the pack"
      if c["n"] + c["cnt"] <= pitch:
        Ks, Vs = Kd[c["par"] + 1:c["par"] + 2].clone(), Vd[c["par"] + 1:c["par"] + 2].clone()
        oe = ops.attention_extend(q, k, v, Ks, Vs, _i32([c["n"]], cuda), cu, c["cnt"])
        torch.cuda.synchronize()
        rel_e = U.report_rows(f"{tag} candidate {j} vs attention_extend", outs[j].float()[None], oe.float().cpu()[None])
        worst_ext = max(worst_ext, rel_e)
        assert rel_e < U.ATTN_BAR, (call[j], rel_e)
    assert torch.equal(_bits(Kd.cpu()), _bits(case["K"])) and torch.equal(_bits(Vd.cpu()), _bits(case["Vt"])), f"{tag}: ops.attention_fork wrote the cache"
  print(f"[attention_fork Bc{Bc} H{H} d{d} pitch {pitch} {kind}] worst row figure {worst:.3e}, against attention_extend {worst_ext:.3e} "
        f"(bar {U.ATTN_BAR})")


@pytest.mark.parametrize("Bc,H,d,pitch", [(3, 12, 64, 96), (2, 32, 80, 96), (1, 32, 128, 320)])
def test_attention_fork_clamps_and_flags(cuda, Bc, H, d, pitch):
  counts = (17, 16, 33, 8, 15, 1, 34)
  call = [(c, n, j % Bc) for j, (c, n) in enumerate(zip(counts, (0, 33, pitch, 5, 31, 9, 3)))]
  case = _case(Bc, H, d, pitch, call, seed=590, kind="large")
  cands = case["cands"]
  R = Bc + 1
  parents = [c["par"] + 1 for c in cands]
  plens = [c["n"] for c in cands]
  plens[0], plens[2] = -5, pitch + 1            # clamped to 0 and to the pitch: the values the candidates were built for
  parents[3], parents[5] = -1, R                # emptied
  flags = torch.zeros(len(cands), dtype=torch.int32, device=cuda)
  fill = 7.0
  outs, ok, same = _fork(case, cands, cuda, parents=parents, plens=plens, max_new=33, flags=flags, fill=fill)   # candidate 6: 34 > max_new
  assert flags.cpu().tolist() == [1, 0, 1, 1, 0, 1, 1]
  assert ok, "a flagged candidate wrote outside a buffer"
  assert same, "the call wrote the cache"
  for j in (3, 5, 6):
    assert bool((outs[j].float() == fill).all()), f"emptied candidate {j} stored something"
  # the clamped candidates are what they were built for (plen 0: exact; plen pitch: every slot of the row up to the largest plen is its own)
  ref, _, _ = _fork(case, cands[:6], cuda)
  for j in (0, 1, 2, 4):
    assert torch.equal(_bits(outs[j]), _bits(ref[j])), f"candidate {j} changed beside flagged candidates"
  rel = U.report_rows("attention_fork clamps", torch.cat([outs[j] for j in (0, 1, 2, 4)]).float()[None],
                      torch.cat([cands[j]["ref"] for j in (0, 1, 2, 4)])[None])
  assert rel < U.ATTN_BAR, rel


def test_attention_fork_bad_arguments_launch_nothing(cuda):
  from gill_amd import _native as N
  Bc, H, d, pitch, C = 2, 12, 64, 96, 2
  mk = lambda *shape: torch.full(shape, 3.0, dtype=torch.bfloat16, device=cuda)   # noqa: E731
  total = 20
  n = total * H * d + 16
  q, kn, vn, o, ws = mk(n), mk(n), mk(n), mk(n), mk(64)
  Kd, Vd = mk(Bc, H, pitch, d), mk(Bc, H, d, pitch)
  parent, plen, cu = _i32([1, 0], cuda), _i32([5, 9], cuda), _i32([0, 3, total], cuda)
  call = lambda q=q, kn=kn, vn=vn, Kd=Kd, Vd=Vd, o=o, max_new=17, H=H, d=d, pitch=pitch, ld=H * d, C=C, wsb=128: _raw(   # noqa: E731
    q, kn, vn, ld, Kd, Vd, parent, plen, cu, o, C, Bc, total, max_new, H, d, pitch, None, ws, wsb)
  assert N.lib().gill_attention_fork_ws_bytes(C, H, d, 17) >= 0
  assert call(max_new=0) != 0, "max_new = 0 accepted"
  assert call(max_new=-1) != 0, "max_new = -1 accepted"
  assert call(C=0) != 0, "C = 0 accepted"
  assert call(q=q[1:]) != 0, "misaligned q accepted"
  assert call(kn=kn[1:]) != 0, "misaligned k_new accepted"
  assert call(vn=vn[1:]) != 0, "misaligned v_new accepted"
  assert call(Kd=Kd.view(-1)[1:]) != 0, "misaligned K accepted"
  assert call(Vd=Vd.view(-1)[1:]) != 0, "misaligned Vt accepted"
  assert call(o=o[1:]) != 0, "misaligned o accepted"
  assert call(H=16, d=48) != 0, "head dim 48 accepted"
  assert call(pitch=80) != 0, "pitch 80 accepted"
  assert call(ld=H * d + 4) != 0, "row stride that breaks the 16-byte alignment accepted"
  assert call(wsb=-1) != 0, "negative workspace size accepted"
  torch.cuda.synchronize()
  for t in (o, Kd, Vd, ws):
    assert bool((t.float() == 3.0).all()), "a refused call wrote something"
  assert call() == 0
  torch.cuda.synchronize()
  assert bool((Kd.float() == 3.0).all()) and bool((Vd.float() == 3.0).all()) and bool((ws.float() == 3.0).all())
