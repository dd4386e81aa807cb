"""ops.attention_branch (gill_attention_branch: sampled continuations of cached dialogues decode one token each; the siblings of a dialogue share
its prefix in the main cache, read-only, and every branch appends to its own row of a small branch cache) and ops.kv_branch_adopt on the MI355X.

Inputs come from kv_cache_util.decode_attn_inputs as in test_attention_fork_gpu: one draw per main-cache row for the prefix, one per branch for
its query and its m + 1 own keys / values (the last one is the new token and leans towards the query).  A main cache has Bc rows that groups name
plus one that none names.  Per (Bc, H, d), pitch and bpitch one call holds a dialogue per prefix length of NS (both sides of the 32-slot tile and
of the four-wave deal: 128 slots are one tile per wave, 129 start the second round, 96 or fewer leave waves without a tile), with the sibling
counts of SIZES (33 is packed as 32 + 1) and the own counts of MS walked through the branches; parents are dealt from the highest index, not
sorted, several dialogues with different n share a parent.  Slots of a main row at or beyond the LARGEST n of its dialogues, and slots of a
branch row at or beyond its m, hold +-1e30 in one run and bf16 NaN / Inf bit patterns in another; between a dialogue's smaller n and the row's
largest lie the row's real keys, which that dialogue must not see either.  Checked:

  accuracy       against fp64 on the same bf16 operands, kv_cache_util.report_rows' figure per branch, below ATTN_BAR = 2e-2;
  append         slot m of the branch row holds the bits of k_new / v_new; every other word of the branch cache, the whole main cache and the
                 guard words around the four caches and the output are bit-identical after the call;
  independence   a branch alone in a group of 1 (S = G = 1), the pack reversed (dialogues and siblings, the branch rows with them) and the
                 prefixes at other main-cache row indices give the same output bits; a branch of a 31- or 32-group is thereby compared with
                 itself alone;
  agreement      the same bar against ops.attention_decode on a scratch row holding prefix + own tokens (no bit comparison);
  clamps         n -5 and pitch + 1, m -1 and bpitch, parents -1 and Bc, a group of 33, a range beyond S: flagged, the neighbours keep their
                 bits, emptied groups store nothing, nothing outside the buffers is touched;
  bad arguments  an unsupported d, a misaligned pointer, bpitch % 32 != 0 and S < 1 are errors that launch nothing;
  adopt          the destination slots equal the source bits, the ones-row is written for d = 80, everything else is untouched; the argument
                 errors launch nothing, count = 0 is legal."""
import pytest
import torch

import kv_cache_util as U
from test_attention_decode_gpu import _guarded, _guards_intact
from test_attention_fork_gpu import _bits, _i32, _stale

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 128), (3, 12, 64), (2, 32, 80)]
PITCHES = (96, 320)
BPITCHES = (32, 64)
NS = (0, 1, 31, 32, 33, 127, 128, 129, 160, None)       # None: the pitch
MS = (0, 1, 31, 32, 33, None)                           # None: bpitch - 1
SIZES = (1, 2, 31, 32, 33)
FILL = 7.0


def _dialogues(Bc, pitch, bpitch, rot):
  """[(parent, n, [m of every sibling])]: one dialogue per prefix length, sizes and own counts walked through, parents from the highest index."""
  ns = sorted({pitch if n is None else n for n in NS if n is None or n <= pitch})
  ms = sorted({bpitch - 1 if m is None else m for m in MS if m is None or m <= bpitch - 1})
  ns = ns[rot % len(ns):] + ns[:rot % len(ns)]
  out, k = [], rot
  for i, n in enumerate(ns):
    size = SIZES[(i + rot) % len(SIZES)]
    out.append(((Bc - 1 - i) % Bc, n, [ms[(k + j) % len(ms)] for j in range(size)]))
    k += size
  assert {len(d[2]) for d in out} >= set(SIZES) or len(ns) < len(SIZES)
  return out


def _case(Bc, H, d, pitch, bpitch, dialogues, seed, kind):
  """Host tensors.  Parent p lives at row p + 1 of a (Bc + 1)-row main cache whose row 0 no group names (all stale).
  -> dict(K, Vt bf16, dial: [dict(par, n, br: [dict(m, q (H*d), k, v (m + 1, H*d) float bf16-valued, ref (H*d))])])."""
  dpv = (d + 31) // 32 * 32
  g = torch.Generator().manual_seed(seed)
  K, Vt = _stale((Bc + 1, H, pitch, d), kind, g), _stale((Bc + 1, H, dpv, pitch), kind, g)
  pre = []
  for p in range(Bc):
    top = max([n for par, n, _ in dialogues if par == p], default=0)
    _, kb, vb = U.decode_attn_inputs(1, H, 1, max(top, 1), d, seed=seed * 31 + p)
    kh = kb[0].view(-1, H, d).transpose(0, 1)[:, :top]          # (H, top, d)
    vh = vb[0].view(-1, H, d).transpose(0, 1)[:, :top]
    K[p + 1, :, :top] = kh.bfloat16()
    Vt[p + 1, :, :d, :top] = vh.transpose(1, 2).bfloat16()
    pre.append((kh, vh))
  dial, j = [], 0
  for par, n, ms in dialogues:
    br = []
    for m in ms:
      qb, kb, vb = U.decode_attn_inputs(1, H, 1, m + 1, d, seed=seed * 131 + 7 + j)
      j += 1
      q, k, v = qb[0, 0], kb[0], vb[0]
      kh = torch.cat([pre[par][0][:, :n], k.view(m + 1, H, d).transpose(0, 1)], 1).double()      # (H, n + m + 1, d)
      vh = torch.cat([pre[par][1][:, :n], v.view(m + 1, H, d).transpose(0, 1)], 1).double()
      s = (q.view(H, 1, d).double() @ kh.transpose(1, 2)) * d ** -0.5
      ref = (s.softmax(-1) @ vh).reshape(H * d).float()
      br.append(dict(m=m, q=q, k=k, v=v, ref=ref))
    dial.append(dict(par=par, n=n, br=br))
  return dict(K=K, Vt=Vt, dial=dial, kind=kind, seed=seed)


def _pack(dial):
  """gstart, group -> dialogue index, flat branches: dialogue order, groups cut at 32."""
  gstart, gd, flat = [0], [], []
  for i, dl in enumerate(dial):
    for c0 in range(0, len(dl["br"]), 32):
      chunk = dl["br"][c0:c0 + 32]
      flat += chunk
      gd.append(i)
      gstart.append(len(flat))
  return gstart, gd, flat


def _branch_cache(flat, H, d, bpitch, kind, seed, extra=1):
  """(S + extra, H, bpitch, d) / (S + extra, H, dpv, bpitch) bf16: branch s's m cached tokens in row s, everything else stale."""
  dpv = (d + 31) // 32 * 32
  g = torch.Generator().manual_seed(seed + 9)
  S = len(flat)
  Kb, Vtb = _stale((S + extra, H, bpitch, d), kind, g), _stale((S + extra, H, dpv, bpitch), kind, g)
  for s, b in enumerate(flat):
    m = b["m"]
    if m:
      Kb[s, :, :m] = b["k"][:m].view(m, H, d).transpose(0, 1).bfloat16()
      Vtb[s, :, :d, :m] = b["v"][:m].view(m, H, d).permute(1, 2, 0).bfloat16()
  return Kb, Vtb


def _raw(qkv, hd, Kd, Vd, Kbd, Vbd, gs, gp, gn, lens, od, S, G, Sb, Bc, H, d, pitch, bpitch, flags, q=None, kn=None, vn=None, ld=None):
  from gill_amd import _native as N
  q = qkv[:, :hd] if q is None else q
  kn = qkv[:, hd:2 * hd] if kn is None else kn
  vn = qkv[:, 2 * hd:] if vn is None else vn
  return N.lib().gill_attention_branch(q.data_ptr(), kn.data_ptr(), vn.data_ptr(), 3 * hd if ld is None else ld, Kd.data_ptr(), Vd.data_ptr(),
                                       Kbd.data_ptr(), Vbd.data_ptr(), gs.data_ptr(), gp.data_ptr(), gn.data_ptr(), lens.data_ptr(),
                                       od.data_ptr(), S, G, Sb, Bc, H, d, pitch, bpitch, None if flags is None else flags.data_ptr(),
                                       N.current_stream())


def _branch(case, dial, bpitch, dev, rowmap=None, gparent=None, gplen=None, lens=None, gstart=None, flags=None, emptied=()):
  """One guarded raw call over the dialogues `dial` in the given order.  rowmap[p]: the main-cache row parent p's prefix is put at (default
  p + 1).  gparent / gplen / lens / gstart override the device arrays.  emptied: flat indices of branches expected to store nothing.
  -> (S, H*d) bf16 output on the host; asserts guards, the read-only main cache and the append."""
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
  gs, gd, flat = _pack(dial)
  S, G, hd = len(flat), len(gd), H * d
  Kbh, Vbh = _branch_cache(flat, H, d, bpitch, case["kind"], case["seed"])
  bufs = [_guarded(tuple(t.shape), FILL, dev) for t in (Kh, Vh, Kbh, Vbh)] + [_guarded((S, hd), FILL, dev)]
  (_, Kd), (_, Vd), (_, Kbd), (_, Vbd), (_, od) = bufs
  for dst, src in ((Kd, Kh), (Vd, Vh), (Kbd, Kbh), (Vbd, Vbh)):
    dst.copy_(src)
  qkv = torch.stack([torch.cat([b["q"], b["k"][b["m"]], b["v"][b["m"]]]) for b in flat]).to(dev, torch.bfloat16).contiguous()
  gp = _i32([rowmap[dial[i]["par"]] for i in gd] if gparent is None else gparent, dev)
  gn = _i32([dial[i]["n"] for i in gd] if gplen is None else gplen, dev)
  if lens is None:
    lens = [dial[i]["n"] + b["m"] for gi, i in enumerate(gd) for b in flat[gs[gi]:gs[gi + 1]]]
  rc = _raw(qkv, hd, Kd, Vd, Kbd, Vbd, _i32(gs if gstart is None else gstart, dev), gp, gn, _i32(lens, dev), od, S, G, S + 1, R, H, d, pitch,
            bpitch, flags)
  torch.cuda.synchronize()
  assert rc == 0, N.lib().gill_last_error()
  for big, _ in bufs:
    assert _guards_intact(big, FILL), "a guard word around a cache or the output changed"
  assert torch.equal(_bits(Kd).cpu(), _bits(Kh)) and torch.equal(_bits(Vd).cpu(), _bits(Vh)), "the call wrote the main cache"
  for s, b in enumerate(flat):      # the append: slot m takes the input bits, nothing else moves
    if s in emptied:
      continue
    m = b["m"]
    Kbh[s, :, m] = b["k"][m].view(H, d).bfloat16()
    Vbh[s, :, :d, m] = b["v"][m].view(H, d).bfloat16()
  assert torch.equal(_bits(Kbd).cpu(), _bits(Kbh)), "the branch K cache is not its old bits plus k_new at slot m"
  assert torch.equal(_bits(Vbd).cpu(), _bits(Vbh)), "the branch V^T cache is not its old bits plus v_new at column m"
  return od.cpu()


@pytest.mark.parametrize("kind", ["large", "nonfinite"])
@pytest.mark.parametrize("bpitch", BPITCHES)
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("Bc,H,d", SHAPES)
def test_attention_branch_accuracy_append_independence_and_agreement(cuda, Bc, H, d, pitch, bpitch, kind):
  from gill_amd import ops
  dialogues = _dialogues(Bc, pitch, bpitch, rot=SHAPES.index((Bc, H, d)) * 2 + (bpitch == 64))
  tag = f"attention_branch Bc{Bc} H{H} d{d} pitch {pitch} bpitch {bpitch} {kind}"
  print(f"[{tag}] (parent, n, sibling own counts): {dialogues}")
  case = _case(Bc, H, d, pitch, bpitch, dialogues, seed=700 + 13 * pitch // 32 + bpitch, kind=kind)
  dial = case["dial"]
  _, _, flat = _pack(dial)
  out = _branch(case, dial, bpitch, cuda)
  assert torch.isfinite(out.float()).all(), f"{tag}: non-finite output (a slot beyond n or m was read as data)"
  ref = torch.stack([b["ref"] for b in flat])
  rel = U.report_rows(tag, out.float()[None], ref[None])
  assert rel < U.ATTN_BAR, rel
  if kind != "large":
    return
  # the pack reversed: dialogues and siblings (the branch rows move with their branches)
  rev = [dict(par=dl["par"], n=dl["n"], br=dl["br"][::-1]) for dl in dial[::-1]]
  _, _, rflat = _pack(rev)
  orv = _branch(case, rev, bpitch, cuda)
  where = {id(b): s for s, b in enumerate(rflat)}
  for s, b in enumerate(flat):
    assert torch.equal(_bits(orv[where[id(b)]]), _bits(out[s])), f"{tag}: branch {s} differs when the pack is reversed"
  # the prefixes at other main-cache row indices (parent p at row p, the unnamed row last)
  omv = _branch(case, dial, bpitch, cuda, rowmap=list(range(Bc)))
  assert torch.equal(_bits(omv), _bits(out)), f"{tag}: a branch differs when its prefix lies in another cache row"
  # the first and last sibling of every dialogue alone (S = G = 1) through ops.attention_branch, and ops.attention_decode on a scratch row
  Kd, Vd = case["K"].to(cuda), case["Vt"].to(cuda)
  worst_dec, s0 = 0.0, 0
  for dl in dial:
    for j in sorted({0, len(dl["br"]) - 1}):
      b, s = dl["br"][j], s0 + j
      m, n = b["m"], dl["n"]
      Kb1, Vb1 = (t.to(cuda) for t in _branch_cache([b], H, d, bpitch, kind, case["seed"] + s, extra=0))
      q, kn, vn = (t.to(cuda, torch.bfloat16)[None].contiguous() for t in (b["q"], b["k"][m], b["v"][m]))
      oa = ops.attention_branch(q, kn, vn, Kd, Vd, Kb1, Vb1, _i32([0, 1], cuda), _i32([dl["par"] + 1], cuda), _i32([n], cuda), _i32([n + m], cuda))
      assert torch.equal(_bits(oa.cpu()[0]), _bits(out[s])), f"{tag}: branch {s} alone differs from itself among {len(dl['br']) - 1} siblings"
      sp = pitch + bpitch          # a scratch row with room for prefix + own tokens + the new one
      Ks = torch.zeros((1, H, sp, d), dtype=torch.bfloat16, device=cuda)
      Vs = torch.zeros((1, H, (d + 31) // 32 * 32, sp), dtype=torch.bfloat16, device=cuda)
      Ks[0, :, :n], Vs[0, :, :, :n] = Kd[dl["par"] + 1, :, :n], Vd[dl["par"] + 1, :, :, :n]
      Ks[0, :, n:n + m], Vs[0, :, :, n:n + m] = Kb1[0, :, :m], Vb1[0, :, :, :m]
      od = ops.attention_decode(q, kn, vn, Ks, Vs, _i32([n + m], cuda))
      torch.cuda.synchronize()
      rel_d = U.report_rows(f"{tag} branch {s} vs attention_decode", out[s].float()[None, None], od.float().cpu()[None])
      worst_dec = max(worst_dec, rel_d)
      assert rel_d < U.ATTN_BAR, (n, m, rel_d)
    s0 += len(dl["br"])
  assert torch.equal(_bits(Kd.cpu()), _bits(case["K"])) and torch.equal(_bits(Vd.cpu()), _bits(case["Vt"])), f"{tag}: ops.attention_branch wrote the main cache"
  print(f"[{tag}] worst branch figure {rel:.3e}, against attention_decode {worst_dec:.3e} (bar {U.ATTN_BAR})")


@pytest.mark.parametrize("Bc,H,d,pitch,bpitch", [(3, 12, 64, 96, 32), (2, 32, 80, 96, 64), (1, 32, 128, 320, 32)])
def test_attention_branch_clamps_and_flags(cuda, Bc, H, d, pitch, bpitch):
  R = Bc + 1
  # dialogue: 0 clean, 1 n = -5 (built for 0), 2 n = pitch + 1 (built for the pitch), 3 parent -1, 4 parent R, 5 own counts -1 and bpitch
  # (built for 0 and bpitch - 1) beside a clean sibling, 6 clean
  dialogues = [(0, 33, [1, 5]), (1 % Bc, 0, [2, 0]), (2 % Bc, pitch, [3]), (0, 9, [1, 2]), (1 % Bc, 31, [4]), (0, 40, [0, bpitch - 1, 7]),
               (2 % Bc, 64, [6, 0])]
  case = _case(Bc, H, d, pitch, bpitch, dialogues, seed=790, kind="large")
  dial = case["dial"]
  gs, gd, flat = _pack(dial)
  gparent = [dl["par"] + 1 for dl in dial]
  gplen = [dl["n"] for dl in dial]
  gplen[1], gplen[2] = -5, pitch + 1
  gparent[3], gparent[4] = -1, R
  lens = [gplen[gi] + b["m"] for gi in range(len(gd)) for b in flat[gs[gi]:gs[gi + 1]]]
  s5 = gs[5]
  lens[s5], lens[s5 + 1] = 40 - 1, 40 + bpitch
  flags = torch.zeros(len(flat), dtype=torch.int32, device=cuda)
  emptied = set(range(gs[3], gs[5]))
  out = _branch(case, dial, bpitch, cuda, gparent=gparent, gplen=gplen, lens=lens, flags=flags, emptied=emptied)
  want = [0] * len(flat)
  for s in list(range(gs[1], gs[5])) + [s5, s5 + 1]:
    want[s] = 1
  assert flags.cpu().tolist() == want
  for s in emptied:
    assert bool((out[s].float() == FILL).all()), f"emptied branch {s} stored an output"
  # the same pack without the overrides that change nothing of what the kept branches were built for: equal bits
  keep = [s for s in range(len(flat)) if s not in emptied]
  clean = _branch(case, [dl for i, dl in enumerate(dial) if i not in (3, 4)], bpitch, cuda)
  assert torch.equal(_bits(out[keep]), _bits(clean)), "a branch changed beside flagged groups, or a clamp did not give the clamped value"
  rel = U.report_rows("attention_branch clamps", out[keep].float()[None], torch.stack([flat[s]["ref"] for s in keep])[None])
  assert rel < U.ATTN_BAR, rel
  # a group of 33 and a range that ends beyond S: emptied, flagged at the group's first branch, nothing stored
  big = [dict(par=0, n=5, br=[dial[0]["br"][0]] * 33)]
  for gstart in ([0, 33, 33], [0, 0, 34]):
    # _pack cuts the 33 siblings into 32 + 1; the override hands the kernel one group of 33 beside an empty one, or a range past S = 33
    fl = torch.zeros(33, dtype=torch.int32, device=cuda)
    o = _branch(case, big, bpitch, cuda, gstart=gstart, gparent=[1, 1], gplen=[5, 5], flags=fl, emptied=set(range(33)))
    assert fl.cpu().tolist() == [1] + [0] * 32, gstart
    assert bool((o.float() == FILL).all()), "an emptied group stored an output"
  fl = torch.zeros(33, dtype=torch.int32, device=cuda)
  o = _branch(case, big, bpitch, cuda, gstart=[-1, 32, 33], gparent=[1, 1], gplen=[5, 5], flags=fl, emptied=set(range(32)))
  assert fl.cpu().tolist() == [1] + [0] * 32 and bool((o[:32].float() == FILL).all()) and not bool((o[32].float() == FILL).all())


def test_attention_branch_bad_arguments_launch_nothing(cuda):
  Bc, H, d, pitch, bpitch, S = 2, 12, 64, 96, 32, 3
  hd = H * d
  mk = lambda *shape: torch.full(shape, 3.0, dtype=torch.bfloat16, device=cuda)   # noqa: E731
  qkv, o = mk(S + 1, 3 * hd), torch.full((S * hd + 16,), 5.0, dtype=torch.bfloat16, device=cuda)
  Kd, Vd, Kb, Vb = mk(Bc, H, pitch, d), mk(Bc, H, d, pitch), mk(S, H, 2 * bpitch, d), mk(S, H, d, 2 * bpitch)
  gs, gp, gn, lens = _i32([0, 2, 3], cuda), _i32([1, 0], cuda), _i32([5, 9], cuda), _i32([6, 5, 12], cuda)
  flat = qkv.view(-1)

  def call(q=None, kn=None, vn=None, Kd=Kd, Vd=Vd, Kb=Kb, Vb=Vb, o=o, S=S, H=H, d=d, pitch=pitch, bpitch=bpitch, ld=None):
    return _raw(qkv, hd, Kd, Vd, Kb, Vb, gs, gp, gn, lens, o, S, 2, 3, Bc, H, d, pitch, bpitch, None, q=q, kn=kn, vn=vn, ld=ld)

  assert call(S=0) != 0, "S = 0 accepted"
  assert call(S=-1) != 0, "S = -1 accepted"
  assert call(S=4) != 0, "more branches than branch rows accepted"
  assert call(q=flat[1:]) != 0, "misaligned q accepted"
  assert call(kn=flat[hd + 1:]) != 0, "misaligned k_new accepted"
  assert call(vn=flat[2 * hd + 1:]) != 0, "misaligned v_new accepted"
  for name in ("Kd", "Vd", "Kb", "Vb"):
    t = dict(Kd=Kd, Vd=Vd, Kb=Kb, Vb=Vb)[name]
    assert call(**{name: t.view(-1)[1:]}) != 0, f"misaligned {name} accepted"
  assert call(o=o[1:]) != 0, "misaligned o accepted"
  assert call(H=16, d=48) != 0, "head dim 48 accepted"
  assert call(pitch=80) != 0, "pitch 80 accepted"
  assert call(bpitch=16) != 0, "bpitch 16 accepted"
  assert call(bpitch=48) != 0, "bpitch 48 accepted"
  assert call(bpitch=0) != 0, "bpitch 0 accepted"
  assert call(ld=3 * hd + 4) != 0, "row stride that breaks the 16-byte alignment accepted"
  torch.cuda.synchronize()
  for t, fill in ((o, 5.0), (Kd, 3.0), (Vd, 3.0), (Kb, 3.0), (Vb, 3.0)):
    assert bool((t.float() == fill).all()), "a refused call wrote something"
  assert call() == 0
  torch.cuda.synchronize()
  assert bool((Kd.float() == 3.0).all()) and bool((Vd.float() == 3.0).all())
  assert bool((o[:S * hd].float() == 3.0).all()) and bool((o[S * hd:].float() == 5.0).all()), "the accepted call: every value is 3, so is the output"


@pytest.mark.parametrize("Bc,H,d,pitch,bpitch", [(3, 12, 64, 96, 32), (2, 32, 80, 96, 64), (1, 32, 128, 320, 32)])
def test_kv_branch_adopt(cuda, Bc, H, d, pitch, bpitch):
  from gill_amd import _native as N
  from gill_amd import ops
  dpv, Sb = (d + 31) // 32 * 32, 3
  g = torch.Generator().manual_seed(810 + d)
  hosts = [_stale(shape, kind, g) for shape, kind in (((Sb, H, bpitch, d), "large"), ((Sb, H, dpv, bpitch), "nonfinite"),
                                                      ((Bc, H, pitch, d), "nonfinite"), ((Bc, H, dpv, pitch), "large"))]
  hosts[0] = U.bf(torch.randn((Sb, H, bpitch, d), generator=g)).bfloat16()
  hosts[1][:, :, :d] = U.bf(torch.randn((Sb, H, d, bpitch), generator=g)).bfloat16()
  bufs = [_guarded(tuple(t.shape), FILL, cuda) for t in hosts]
  (_, Kbd), (_, Vbd), (_, Kd), (_, Vd) = bufs
  for (_, dst), src in zip(bufs, hosts):
    dst.copy_(src)
  Kbh, Vbh, Kh, Vh = (t.clone() for t in hosts)
  for s, r, plen, count in ((1, Bc - 1, 0, 0), (2, 0, 7, 1), (0, Bc - 1, 33, min(bpitch, 31)), (1, 0, pitch - 1 - bpitch, bpitch),
                            (2, Bc - 1, pitch - 1, 0)):
    ops.kv_branch_adopt(Kbd, Vbd, Kd, Vd, s, r, plen, count)
    torch.cuda.synchronize()
    Kh[r, :, plen:plen + count] = Kbh[s, :, :count]
    Vh[r, :, :d, plen:plen + count] = Vbh[s, :, :d, :count]
    if dpv > d:
      Vh[r, :, d, plen:plen + count] = 1.0
    tag = f"adopt s {s} r {r} plen {plen} count {count}"
    assert torch.equal(_bits(Kd).cpu(), _bits(Kh)), f"{tag}: K is not its old bits plus the branch's keys at the destination slots"
    assert torch.equal(_bits(Vd).cpu(), _bits(Vh)), f"{tag}: V^T is not its old bits plus the branch's columns" + (" and the ones-row" if dpv > d else "")
    assert torch.equal(_bits(Kbd).cpu(), _bits(Kbh)) and torch.equal(_bits(Vbd).cpu(), _bits(Vbh)), f"{tag}: the branch cache was written"
    for big, _ in bufs:
      assert _guards_intact(big, FILL), f"{tag}: a guard word changed"
  raw = lambda s, r, plen, count, bp=bpitch: N.lib().gill_kv_branch_adopt(   # noqa: E731
    Kbd.data_ptr(), Vbd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), Sb, Bc, H, d, pitch, bp, s, r, plen, count, N.current_stream())
  assert raw(0, 0, pitch - 1 - 4, 5) != 0, "plen + count = pitch accepted"
  assert raw(0, 0, 0, bpitch + 1) != 0, "count > bpitch accepted"
  assert raw(-1, 0, 0, 1) != 0 and raw(Sb, 0, 0, 1) != 0, "a branch row out of range accepted"
  assert raw(0, -1, 0, 1) != 0 and raw(0, Bc, 0, 1) != 0, "a cache row out of range accepted"
  assert raw(0, 0, -1, 1) != 0 and raw(0, 0, 0, -1) != 0, "a negative plen or count accepted"
  torch.cuda.synchronize()
  assert torch.equal(_bits(Kd).cpu(), _bits(Kh)) and torch.equal(_bits(Vd).cpu(), _bits(Vh)), "a refused adopt wrote the cache"
