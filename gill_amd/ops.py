"""Operator-level Python wrappers over libgill_amd (gill_op_* in include/gill_amd.h).

These exist so the parity tests can pin every kernel the three stages are built from; the stages
themselves (gill_amd.models / layers / sd) call the stage-level entry points, not these.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _native as N

ACT = {"none": 0, "relu": 1, "gelu": 2, "silu": 3}


def _bf(t: torch.Tensor) -> torch.Tensor:
  assert t.dtype == torch.bfloat16 and t.is_cuda
  return t.contiguous()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
         alpha: float = 1.0, act: str = "none", out_f32: bool = False, splitk: int = 0, row_major: bool = False, guarded: bool = False):
  """act(alpha * a @ w.T + bias + resid); a (M,K) bf16, w (N,K) bf16, bias (N) fp32, resid (M,N) bf16 or fp32 (the OPT / CLIP residual stream).
  guarded: the output lives in a _guarded() buffer (NaN-prefilled, GUARD_WORDS sentinels behind it) and (out, guard_ok) is returned.
  row_major: keep weight-streaming shapes (N * K >= 4 Mi) on row-major weights instead of the 64 x 64-blocked copy (STREAM64 tile up to 256 rows, general
  tiles on the blocked layout above)."""
  if row_major:
    splitk = -1 if splitk <= 1 else -splitk
  a, w = _bf(a), _bf(w)
  M, K = a.shape
  Nn = w.shape[0]
  buf, out = _out_buffer((M, Nn), torch.float32 if out_f32 else torch.bfloat16, a.device, guarded)
  if bias is not None:
    bias = bias.float().contiguous()
  resid_f32 = resid is not None and resid.dtype == torch.float32
  if resid is not None:
    resid = resid.contiguous() if resid_f32 else _bf(resid)
    assert resid.is_cuda and tuple(resid.shape) == (M, Nn)
  N.check(N.lib().gill_op_gemm(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(resid), N.ptr(out), M, Nn, K, alpha, ACT[act],
                               int(out_f32) | (2 if resid_f32 else 0), splitk, N.current_stream()))
  return (out, _guard_ok(buf)) if guarded else out


def geglu_fp8(t: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
  """BASELINE configs[4]: diffusers GEGLU of LayerNorm(t) on the fp8 matrix instruction (csrc/linear_fp8.hip): t (M,C) bf16, w (2 inner, C) bf16 in
  diffusers order, bias (2 inner); activations and weights quantised to e4m3 as the engine's fp8 mode does.  Returns (M, inner) bf16."""
  t, w = _bf(t), _bf(w)
  M, Cc = t.shape
  inner = w.shape[0] // 2
  out = torch.empty((M, inner), device=t.device, dtype=torch.bfloat16)
  f = lambda x: x.float().contiguous()   # noqa: E731
  ln_g, ln_b, bias = f(ln_g), f(ln_b), f(bias)
  N.check(N.lib().gill_op_geglu_fp8(N.ptr(t), N.ptr(ln_g), N.ptr(ln_b), N.ptr(w), N.ptr(bias), N.ptr(out), M, inner, Cc, N.current_stream()))
  return out


def geglu(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], guarded: bool = False):
  """diffusers GEGLU: h, g = (a @ w.T + bias).chunk(2, -1); h * gelu(g).  guarded: as in gemm()."""
  a, w = _bf(a), _bf(w)
  M, K = a.shape
  inner = w.shape[0] // 2
  buf, out = _out_buffer((M, inner), torch.bfloat16, a.device, guarded)
  if bias is not None:
    bias = bias.float().contiguous()
  N.check(N.lib().gill_op_geglu(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(out), M, inner, K, N.current_stream()))
  return (out, _guard_ok(buf)) if guarded else out


def conv3x3(x1: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None,
            rowvec: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, stride: int = 1,
            upsample: bool = False, splitk: int = 0, pad_shift: Optional[int] = None, guarded: bool = False):
  """3x3 / pad 1 conv over NHWC bf16 x1 (B,H,W,C1) [channel-concat x2], weights OIHW fp32 -> NHWC bf16.  guarded: as in gemm().
  pad_shift (None: gill_op_conv3x3; 0 | 1: gill_op_conv3x3_ex): 1 with stride 2 is F.pad(x, (0, 1, 0, 1)) + conv(stride 2, pad 0)."""
  x1 = _bf(x1)
  B, IH, IW, C1 = x1.shape
  C2 = 0
  if x2 is not None:
    x2 = _bf(x2)
    C2 = x2.shape[-1]
  w = w_oihw.float().contiguous()
  Cout = w.shape[0]
  assert w.shape[1] == C1 + C2
  if upsample:
    OH, OW = 2 * IH, 2 * IW
  else:
    OH, OW = (IH + 2 - 3) // stride + 1, (IW + 2 - 3) // stride + 1
  if pad_shift:
    OH, OW = IH // 2, IW // 2
  buf, y = _out_buffer((B, OH, OW, Cout), torch.bfloat16, x1.device, guarded)
  if bias is not None:
    bias = bias.float().contiguous()
  if rowvec is not None:
    rowvec = rowvec.float().contiguous()
  if resid is not None:
    resid = _bf(resid)
  if pad_shift is not None:
    N.check(N.lib().gill_op_conv3x3_ex(N.ptr(x1), C1, N.ptr(x2), C2, N.ptr(w), N.ptr(bias), N.ptr(rowvec), N.ptr(resid),
                                       N.ptr(y), B, IH, IW, Cout, stride, int(upsample), int(pad_shift), splitk, N.current_stream()))
    return (y, _guard_ok(buf)) if guarded else y
  N.check(N.lib().gill_op_conv3x3(N.ptr(x1), C1, N.ptr(x2), C2, N.ptr(w), N.ptr(bias), N.ptr(rowvec), N.ptr(resid),
                                  N.ptr(y), B, IH, IW, Cout, stride, int(upsample), splitk, N.current_stream()))
  return (y, _guard_ok(buf)) if guarded else y


def conv3x3_ex(x1: torch.Tensor, w_oihw: torch.Tensor, pad_shift: int, **kw):
  """gill_op_conv3x3_ex: conv3x3 with the gather's origin shift stated."""
  return conv3x3(x1, w_oihw, pad_shift=int(pad_shift), **kw)


def conv3x3_gn(x: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
               groups: int = 32, eps: float = 1e-5, silu: bool = True, resid: Optional[torch.Tensor] = None, splitk: int = 2,
               want_raw: bool = True, coop: bool = True, rowvec: Optional[torch.Tensor] = None, want_table: bool = False, want_norm: bool = True):
  """3x3 convolution + the consuming GroupNorm (+ SiLU) without a GroupNorm launch of its own (include/gill_amd.h gill_op_conv3x3_gn):
  splitk >= 2 in the split-K reducer launch (coop is ignored); splitk == 1 in the
  convolution's epilogue (coop=True) or as conv + GroupNorm-apply (coop=False, the reference dataflow).  x (B,H,W,Cin) bf16 NHWC, rowvec (B,Cout).
  Returns (y_raw or None, y_norm or None[, table (B,2,Cout) fp32 when want_table]) — outputs NaN-prefilled, so an unwritten element shows."""
  x = _bf(x)
  B, H, W, Cin = x.shape
  Cout = w_oihw.shape[0]
  nan = float("nan")
  y_raw = torch.full((B, H, W, Cout), nan, device=x.device, dtype=torch.bfloat16) if want_raw else None
  y_norm = torch.full((B, H, W, Cout), nan, device=x.device, dtype=torch.bfloat16) if want_norm else None
  table = torch.full((B, 2, Cout), nan, device=x.device, dtype=torch.float32) if want_table else None
  f = lambda t: None if t is None else t.float().contiguous()   # noqa: E731
  w, bias, gamma, beta, rowvec = f(w_oihw), f(bias), f(gamma), f(beta), f(rowvec)
  resid = None if resid is None else _bf(resid)
  N.check(N.lib().gill_op_conv3x3_gn(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(rowvec), N.ptr(resid), N.ptr(gamma), N.ptr(beta), groups, float(eps),
                                     int(silu), N.ptr(y_raw), N.ptr(y_norm), N.ptr(table), B, H, W, Cin, Cout, splitk, int(coop), N.current_stream()))
  return (y_raw, y_norm, table) if want_table else (y_raw, y_norm)


def conv3x3_shortcut(x1: torch.Tensor, w_oihw: torch.Tensor, xs1: torch.Tensor, w_sc: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     x2: Optional[torch.Tensor] = None, xs2: Optional[torch.Tensor] = None, splitk: int = 0, guarded: bool = False):
  """conv3x3(x1 ++ x2, w_oihw) + bias + conv1x1(xs1 ++ xs2, w_sc) as one implicit GEMM (ResnetBlock2D conv2 + conv_shortcut).
  guarded: as in gemm()."""
  x1, xs1 = _bf(x1), _bf(xs1)
  B, IH, IW, C1 = x1.shape
  C2 = CS2 = 0
  if x2 is not None:
    x2 = _bf(x2); C2 = x2.shape[-1]
  if xs2 is not None:
    xs2 = _bf(xs2); CS2 = xs2.shape[-1]
  CS1 = xs1.shape[-1]
  w, wsc = w_oihw.float().contiguous(), w_sc.float().contiguous()
  Cout = w.shape[0]
  assert w.shape[1] == C1 + C2 and tuple(wsc.shape) == (Cout, CS1 + CS2)
  buf, y = _out_buffer((B, IH, IW, Cout), torch.bfloat16, x1.device, guarded)
  if bias is not None:
    bias = bias.float().contiguous()
  N.check(N.lib().gill_op_conv3x3_shortcut(N.ptr(x1), C1, N.ptr(x2), C2, N.ptr(w), N.ptr(bias), N.ptr(xs1), CS1, N.ptr(xs2), CS2,
                                           N.ptr(wsc), N.ptr(y), B, IH, IW, Cout, splitk, N.current_stream()))
  return (y, _guard_ok(buf)) if guarded else y


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
              causal: bool = False) -> torch.Tensor:
  """q (B,nq,H*d), k/v (B,nkv,H*d) bf16 -> (B,nq,H*d) bf16."""
  q, k, v = _bf(q), _bf(k), _bf(v)
  B, nq, hd = q.shape
  nkv = k.shape[1]
  d = hd // heads
  if scale is None:
    scale = d ** -0.5
  o = torch.empty_like(q)
  N.check(N.lib().gill_op_attention(N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(o), B, heads, nq, nkv, d, float(scale),
                                    int(causal), N.current_stream()))
  return o


def attention_decode(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, lens: torch.Tensor,
                     flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """Decode attention with append: q / k_new / v_new (B, H*d) bf16, one new token per row; K (B,H,pitch,d) and Vt (B,H,round_up(d,32),pitch)
  bf16 caches, updated IN PLACE at slot lens[b]; lens (B) int32 on the device; flags (B) int32 (optional) receives 1 where a length was
  clamped into the cache.  Returns (B, H*d) bf16."""
  B, H, pitch, d = K.shape
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (B, H * d)
  assert K.dtype == torch.bfloat16 and Vt.dtype == torch.bfloat16 and tuple(Vt.shape) == (B, H, (d + 31) // 32 * 32, pitch)
  assert lens.dtype == torch.int32 and lens.numel() == B and (flags is None or (flags.dtype == torch.int32 and flags.numel() == B))
  o = torch.empty_like(q)
  N.check(N.lib().gill_attention_decode(N.ptr(q), N.ptr(k_new), N.ptr(v_new), H * d, N.ptr(K), N.ptr(Vt), N.ptr(lens), N.ptr(o), B, H, d, pitch,
                                        N.ptr(flags), N.current_stream()))
  return o


def attention_append(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, lens: torch.Tensor,
                     flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """Decode attention with a multi-token append: q / k_new / v_new (B, nq, H*d) bf16, row b's nq consecutive new tokens (1 <= nq <= 16) at its
  cache length lens[b]; K (B,H,pitch,d) and Vt (B,H,round_up(d,32),pitch) bf16 caches, updated IN PLACE at slots lens[b] .. lens[b] + nq - 1; lens
  (B) int32 on the device; flags (B) int32 (optional) receives 1 where a length was clamped into [0, pitch - nq].  Returns (B, nq, H*d) bf16: bit for
  bit what nq successive attention_decode calls at lens, lens + 1, .. give."""
  B, H, pitch, d = K.shape
  nq = q.shape[1]
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (B, nq, H * d)
  assert K.dtype == torch.bfloat16 and Vt.dtype == torch.bfloat16 and tuple(Vt.shape) == (B, H, (d + 31) // 32 * 32, pitch)
  assert lens.dtype == torch.int32 and lens.numel() == B and (flags is None or (flags.dtype == torch.int32 and flags.numel() == B))
  o = torch.empty_like(q)
  N.check(N.lib().gill_attention_append(N.ptr(q), N.ptr(k_new), N.ptr(v_new), H * d, N.ptr(K), N.ptr(Vt), N.ptr(lens), N.ptr(o), B, nq, H, d, pitch,
                                        N.ptr(flags), N.current_stream()))
  return o


def attention_extend(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, lens: torch.Tensor,
                     cu_new: torch.Tensor, max_new: int, flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """Ragged multi-token attention with append: q / k_new / v_new (total_new, H*d) bf16, packed rows (each contiguous, or the three column thirds
  of one (total_new, 3*H*d) projection); cu_new (B + 1) int32 on the device, the prefix sums of the per-row new-token counts (zero is legal);
  row cu_new[b] + i is token lens[b] + i of sequence b.  K (B,H,pitch,d) and Vt (B,H,round_up(d,32),pitch) bf16 caches, updated IN PLACE at
  slots lens[b] .. lens[b] + count - 1; lens (B) int32 on the device; max_new: the host's bound on a row's count; flags (B) int32 (optional)
  receives 1 where a length was clamped into [0, pitch - count].  Returns (total_new, H*d) bf16."""
  B, H, pitch, d = K.shape
  total = q.shape[0]
  ld = q.stride(0)
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_cuda and tuple(t.shape) == (total, H * d) and t.stride(1) == 1 and t.stride(0) == ld
  assert K.dtype == torch.bfloat16 and Vt.dtype == torch.bfloat16 and tuple(Vt.shape) == (B, H, (d + 31) // 32 * 32, pitch)
  assert lens.dtype == torch.int32 and lens.numel() == B and cu_new.dtype == torch.int32 and cu_new.numel() == B + 1
  assert flags is None or (flags.dtype == torch.int32 and flags.numel() == B)
  o = torch.empty((total, H * d), dtype=torch.bfloat16, device=q.device)
  if total == 0:      # no row brought a token: nothing to store, nothing to attend
    return o
  N.check(N.lib().gill_attention_extend(q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), ld, N.ptr(K), N.ptr(Vt), N.ptr(lens), N.ptr(cu_new),
                                        N.ptr(o), B, total, int(max_new), H, d, pitch, N.ptr(flags), N.current_stream()))
  return o


def attention_fork(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, parent: torch.Tensor,
                   plen: torch.Tensor, cu_new: torch.Tensor, max_new: int, flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """Fork attention: C packed candidate continuations, q / k_new / v_new (total_new, H*d) bf16 packed rows as in attention_extend; candidate c
  attends to the slots 0 .. plen[c] - 1 of cache row parent[c] and causally to its own tokens.  K (Bc,H,pitch,d) and Vt
  (Bc,H,round_up(d,32),pitch) bf16 caches are READ ONLY; parent, plen (C) and cu_new (C + 1) int32 on the device; max_new: the host's bound on
  a candidate's count; flags (C) int32 (optional) receives 1 where a candidate was clamped or emptied.  The workspace
  (gill_attention_fork_ws_bytes) is allocated here.  Returns (total_new, H*d) bf16."""
  Bc, H, pitch, d = K.shape
  total = q.shape[0]
  ld = q.stride(0)
  C = parent.numel()
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_cuda and tuple(t.shape) == (total, H * d) and t.stride(1) == 1 and t.stride(0) == ld
  assert K.dtype == torch.bfloat16 and Vt.dtype == torch.bfloat16 and tuple(Vt.shape) == (Bc, H, (d + 31) // 32 * 32, pitch)
  assert K.is_contiguous() and Vt.is_contiguous()
  assert parent.dtype == torch.int32 and plen.dtype == torch.int32 and plen.numel() == C and cu_new.dtype == torch.int32 and cu_new.numel() == C + 1
  assert flags is None or (flags.dtype == torch.int32 and flags.numel() == C)
  o = torch.empty((total, H * d), dtype=torch.bfloat16, device=q.device)
  if total == 0:      # no candidate brought a token
    return o
  nws = int(N.lib().gill_attention_fork_ws_bytes(C, H, d, int(max_new)))
  ws = torch.empty(nws, dtype=torch.uint8, device=q.device) if nws > 0 else None
  N.check(N.lib().gill_attention_fork(q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), ld, N.ptr(K), N.ptr(Vt), N.ptr(parent), N.ptr(plen),
                                      N.ptr(cu_new), N.ptr(o), C, Bc, total, int(max_new), H, d, pitch, N.ptr(flags), N.ptr(ws), nws,
                                      N.current_stream()))
  return o


def attention_branch(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, Kb: torch.Tensor,
                     Vtb: torch.Tensor, gstart: torch.Tensor, gparent: torch.Tensor, gplen: torch.Tensor, lens: torch.Tensor,
                     flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """Branch decode attention: S branches, one new token each, q / k_new / v_new (S, H*d) bf16 rows (each contiguous, or the three column
  thirds of one (S, 3*H*d) projection).  K (Bc,H,pitch,d) and Vt (Bc,H,round_up(d,32),pitch) bf16 are the main cache, READ ONLY; Kb
  (Sb,H,bpitch,d) and Vtb (Sb,H,round_up(d,32),bpitch) bf16 the branch cache, updated IN PLACE: branch s stores its new key / value at slot
  lens[s] - gplen[g] of row s.  gstart (G + 1), gparent (G), gplen (G) and lens (S) int32 on the device: group g holds the branches
  gstart[g] .. gstart[g + 1] - 1 (at most 32), which attend to the slots 0 .. gplen[g] - 1 of main-cache row gparent[g], then to their own
  row.  flags (S) int32 (optional) receives 1 where a branch was clamped or its group emptied.  Returns (S, H*d) bf16."""
  Bc, H, pitch, d = K.shape
  Sb, bpitch = Kb.shape[0], Kb.shape[2]
  S, G = q.shape[0], gparent.numel()
  ld = q.stride(0)
  dpv = (d + 31) // 32 * 32
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_cuda and tuple(t.shape) == (S, H * d) and t.stride(1) == 1 and t.stride(0) == ld
  assert K.dtype == torch.bfloat16 and Vt.dtype == torch.bfloat16 and tuple(Vt.shape) == (Bc, H, dpv, pitch)
  assert Kb.dtype == torch.bfloat16 and Vtb.dtype == torch.bfloat16 and tuple(Kb.shape) == (Sb, H, bpitch, d) and tuple(Vtb.shape) == (Sb, H, dpv, bpitch)
  for t in (K, Vt, Kb, Vtb):
    assert t.is_cuda and t.is_contiguous()
  for t, n in ((gstart, G + 1), (gparent, G), (gplen, G), (lens, S)):
    assert t.dtype == torch.int32 and t.is_cuda and t.numel() == n
  assert flags is None or (flags.dtype == torch.int32 and flags.numel() == S)
  o = torch.empty((S, H * d), dtype=torch.bfloat16, device=q.device)
  N.check(N.lib().gill_attention_branch(q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), ld, N.ptr(K), N.ptr(Vt), N.ptr(Kb), N.ptr(Vtb),
                                        N.ptr(gstart), N.ptr(gparent), N.ptr(gplen), N.ptr(lens), N.ptr(o), S, G, Sb, Bc, H, d, pitch, bpitch,
                                        N.ptr(flags), N.current_stream()))
  return o


def kv_branch_adopt(Kb: torch.Tensor, Vtb: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, s: int, r: int, plen: int, count: int) -> None:
  """Adopt a branch into its dialogue: the first `count` keys / values of branch row s (Kb (Sb,H,bpitch,d), Vtb (Sb,H,round_up(d,32),bpitch))
  are copied to the slots plen .. plen + count - 1 of row r of the main cache (K, Vt), IN PLACE, with the ones-row entries of those slots
  where round_up(d,32) > d.  plen + count <= pitch - 1 and count <= bpitch; count = 0 is legal."""
  Bc, H, pitch, d = K.shape
  Sb, bpitch = Kb.shape[0], Kb.shape[2]
  dpv = (d + 31) // 32 * 32
  assert tuple(Vt.shape) == (Bc, H, dpv, pitch) and tuple(Kb.shape) == (Sb, H, bpitch, d) and tuple(Vtb.shape) == (Sb, H, dpv, bpitch)
  for t in (Kb, Vtb, K, Vt):
    assert t.dtype == torch.bfloat16 and t.is_cuda and t.is_contiguous()
  N.check(N.lib().gill_kv_branch_adopt(N.ptr(Kb), N.ptr(Vtb), N.ptr(K), N.ptr(Vt), Sb, Bc, H, d, pitch, bpitch, int(s), int(r), int(plen),
                                       int(count), N.current_stream()))


def _kv8_cache_checks(K8: torch.Tensor, Vt8: torch.Tensor, Kexp: torch.Tensor, Vexp: torch.Tensor):
  B, H, pitch, d = K8.shape
  assert K8.dtype == torch.uint8 and Vt8.dtype == torch.uint8 and tuple(Vt8.shape) == (B, H, (d + 31) // 32 * 32, pitch)
  assert Kexp.dtype == torch.int8 and Vexp.dtype == torch.int8 and tuple(Kexp.shape) == (B, H, pitch) and tuple(Vexp.shape) == (B, H, pitch)
  for t in (K8, Vt8, Kexp, Vexp):
    assert t.is_cuda and t.is_contiguous()
  return B, H, pitch, d


def attention_decode_kv8(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K8: torch.Tensor, Vt8: torch.Tensor, Kexp: torch.Tensor,
                         Vexp: torch.Tensor, lens: torch.Tensor, flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """attention_decode on an e4m3 cache: K8 (B,H,pitch,d) and Vt8 (B,H,round_up(d,32),pitch) uint8 (OCP e4m3 codes), Kexp / Vexp (B,H,pitch)
  int8 (a row's scale is 2^e), all updated IN PLACE at slot lens[b]: the new key and value rows are quantised by the kernel, and the
  quantised rows are what the token itself attends to.  q / k_new / v_new (B, H*d) bf16.  Returns (B, H*d) bf16."""
  B, H, pitch, d = _kv8_cache_checks(K8, Vt8, Kexp, Vexp)
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (B, H * d)
  assert lens.dtype == torch.int32 and lens.numel() == B and (flags is None or (flags.dtype == torch.int32 and flags.numel() == B))
  o = torch.empty_like(q)
  N.check(N.lib().gill_attention_decode_kv8(N.ptr(q), N.ptr(k_new), N.ptr(v_new), H * d, N.ptr(K8), N.ptr(Vt8), N.ptr(Kexp), N.ptr(Vexp),
                                            N.ptr(lens), N.ptr(o), B, H, d, pitch, N.ptr(flags), N.current_stream()))
  return o


def attention_extend_kv8(q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, K8: torch.Tensor, Vt8: torch.Tensor, Kexp: torch.Tensor,
                         Vexp: torch.Tensor, lens: torch.Tensor, cu_new: torch.Tensor, max_new: int,
                         flags: Optional[torch.Tensor] = None) -> torch.Tensor:
  """attention_extend on an e4m3 cache (the buffers of attention_decode_kv8, updated IN PLACE at slots lens[b] .. lens[b] + count - 1); q /
  k_new / v_new (total_new, H*d) bf16 packed rows, cu_new, max_new and flags as in attention_extend.  Returns (total_new, H*d) bf16."""
  B, H, pitch, d = _kv8_cache_checks(K8, Vt8, Kexp, Vexp)
  total = q.shape[0]
  ld = q.stride(0)
  for t in (q, k_new, v_new):
    assert t.dtype == torch.bfloat16 and t.is_cuda and tuple(t.shape) == (total, H * d) and t.stride(1) == 1 and t.stride(0) == ld
  assert lens.dtype == torch.int32 and lens.numel() == B and cu_new.dtype == torch.int32 and cu_new.numel() == B + 1
  assert flags is None or (flags.dtype == torch.int32 and flags.numel() == B)
  o = torch.empty((total, H * d), dtype=torch.bfloat16, device=q.device)
  if total == 0:      # no row brought a token: nothing to store, nothing to attend
    return o
  N.check(N.lib().gill_attention_extend_kv8(q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), ld, N.ptr(K8), N.ptr(Vt8), N.ptr(Kexp),
                                            N.ptr(Vexp), N.ptr(lens), N.ptr(cu_new), N.ptr(o), B, total, int(max_new), H, d, pitch,
                                            N.ptr(flags), N.current_stream()))
  return o


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
  assert x.is_cuda and x.dtype in (torch.bfloat16, torch.float32)
  x = x.contiguous()
  Cc = x.shape[-1]
  rows = x.numel() // Cc
  y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
  g, b = gamma.float().contiguous(), beta.float().contiguous()
  N.check(N.lib().gill_op_layernorm(N.ptr(x), int(x.dtype == torch.float32), N.ptr(g), N.ptr(b), N.ptr(y), rows, Cc, eps,
                                    N.current_stream()))
  return y


def groupnorm(x1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-5,
              silu: bool = False, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
  """GroupNorm(+SiLU) over NHWC bf16 (B,H,W,C1) [channel-concat x2] -> NHWC bf16 (B,H,W,C1+C2)."""
  x1 = _bf(x1)
  B, H, W, C1 = x1.shape
  C2 = 0
  if x2 is not None:
    x2 = _bf(x2)
    C2 = x2.shape[-1]
  y = torch.empty((B, H, W, C1 + C2), device=x1.device, dtype=torch.bfloat16)
  g, b = gamma.float().contiguous(), beta.float().contiguous()
  N.check(N.lib().gill_op_groupnorm(N.ptr(x1), C1, N.ptr(x2), C2, B, H * W, groups, N.ptr(g), N.ptr(b), eps, int(silu),
                                    N.ptr(y), N.current_stream()))
  return y


GN_SLAB_ROWS_MIN = 16      # csrc/ops.h: statistics buffers are sized for 16-row slabs, the smallest any producer files


def _gn_stats_buffer(B: int, rows: int, nbins: int, device) -> torch.Tensor:
  return torch.full((B * (rows // GN_SLAB_ROWS_MIN) * nbins * 2,), float("nan"), device=device, dtype=torch.float32)


def conv3x3_gn_stats(x1: torch.Tensor, w_oihw: torch.Tensor, bin: int, bias: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None,
                     rowvec: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, xs1: Optional[torch.Tensor] = None,
                     w_sc: Optional[torch.Tensor] = None, xs2: Optional[torch.Tensor] = None, upsample: bool = False, splitk: int = 1):
  """3x3 / pad 1 / stride 1 convolution launched with fused GroupNorm statistics in bins of `bin` channels (include/gill_amd.h
  gill_op_conv3x3_gn_stats; xs1 / w_sc [/ xs2]: the fused 1x1 shortcut segment; upsample: the four-tap form).  Returns (y (B,OH,OW,Cout) bf16,
  the whole raw partial buffer (flat fp32, sized for 16-row slabs), slab_rows, nslab): y and the buffer NaN-prefilled; the launcher wrote
  buffer[:B * nslab * (Cout // bin) * 2] as [B][nslab][Cout // bin][2]."""
  x1 = _bf(x1)
  B, IH, IW, C1 = x1.shape
  x2 = None if x2 is None else _bf(x2)
  xs1 = None if xs1 is None else _bf(xs1)
  xs2 = None if xs2 is None else _bf(xs2)
  C2 = 0 if x2 is None else x2.shape[-1]
  CS1 = 0 if xs1 is None else xs1.shape[-1]
  CS2 = 0 if xs2 is None else xs2.shape[-1]
  f = lambda t: None if t is None else t.float().contiguous()   # noqa: E731
  w, wsc, bias, rowvec = f(w_oihw), f(w_sc), f(bias), f(rowvec)
  Cout = w.shape[0]
  assert w.shape[1] == C1 + C2 and (wsc is None or tuple(wsc.shape) == (Cout, CS1 + CS2))
  resid = None if resid is None else _bf(resid)
  OH, OW = (2 * IH, 2 * IW) if upsample else (IH, IW)
  y = torch.full((B, OH, OW, Cout), float("nan"), device=x1.device, dtype=torch.bfloat16)
  stats = _gn_stats_buffer(B, OH * OW, Cout // bin, x1.device)
  rows, nslab = ctypes.c_int(0), ctypes.c_int(0)
  N.check(N.lib().gill_op_conv3x3_gn_stats(N.ptr(x1), C1, N.ptr(x2), C2, N.ptr(w), N.ptr(bias), N.ptr(rowvec), N.ptr(resid), N.ptr(xs1), CS1,
                                           N.ptr(xs2), CS2, N.ptr(wsc), N.ptr(y), N.ptr(stats), bin, B, IH, IW, Cout, int(upsample), splitk,
                                           ctypes.byref(rows), ctypes.byref(nslab), N.current_stream()))
  return y, stats, rows.value, nslab.value


def gemm_gn_stats(a: torch.Tensor, w: torch.Tensor, bin: int, rows_per_batch: int, bias: Optional[torch.Tensor] = None,
                  resid: Optional[torch.Tensor] = None, splitk: int = 1, act: str = "none"):
  """act(a (M,K) @ w (N,K).T + bias + resid) launched with fused GroupNorm statistics (gill_op_gemm_gn_stats): the VAE decoder's conv_in (im2col,
  K = 64) and attention to_out GEMMs.  Returns as conv3x3_gn_stats, y (M,N)."""
  a, w = _bf(a), _bf(w)
  M, K = a.shape
  Nn = w.shape[0]
  bias = None if bias is None else bias.float().contiguous()
  resid = None if resid is None else _bf(resid)
  y = torch.full((M, Nn), float("nan"), device=a.device, dtype=torch.bfloat16)
  stats = _gn_stats_buffer(M // rows_per_batch, rows_per_batch, Nn // bin, a.device)
  rows, nslab = ctypes.c_int(0), ctypes.c_int(0)
  N.check(N.lib().gill_op_gemm_gn_stats(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(resid), N.ptr(y), N.ptr(stats), bin, M, Nn, K, rows_per_batch,
                                        splitk, ACT[act], ctypes.byref(rows), ctypes.byref(nslab), N.current_stream()))
  return y, stats, rows.value, nslab.value


def groupnorm_from_stats(x1: torch.Tensor, stats1: torch.Tensor, bin1: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32,
                         eps: float = 1e-5, silu: bool = False, x2: Optional[torch.Tensor] = None, stats2: Optional[torch.Tensor] = None,
                         bin2: int = 0, want_table: bool = False, out8_scale: float = 0.0):
  """GroupNorm(+SiLU) of x1 (B,HW,C1) [++ x2 (B,HW,C2)] bf16 from caller-supplied partial sums (gill_op_groupnorm_from_stats): stats1
  (B,nslab1,C1 // bin1,2), stats2 (B,nslab2,C2 // bin2,2) fp32.  want_table (single source): the scale | shift table (B,2,C1) instead of y.
  out8_scale > 0: y is uint8 — the e4m3 bytes of fp8(out8_scale * value), as the fp8 convolutions read them — in a guarded buffer.
  Returns (y or None, table or None, stats1, stats2[, guard_ok when out8_scale > 0]): outputs NaN-prefilled, the statistics tensors as they
  are after the call."""
  x1 = _bf(x1)
  B, HW, C1 = x1.shape
  C2 = 0
  if x2 is not None:
    x2 = _bf(x2)
    C2 = x2.shape[-1]
  chk = lambda st, nb: st.is_cuda and st.dtype == torch.float32 and st.is_contiguous() and st.dim() == 4 and st.shape[0] == B and tuple(st.shape[2:]) == (nb, 2)   # noqa: E731
  assert chk(stats1, C1 // bin1) and (stats2 is None or chk(stats2, C2 // bin2))
  g, b = gamma.float().contiguous(), beta.float().contiguous()
  nan = float("nan")
  y = None if want_table else torch.full((B, HW, C1 + C2), nan, device=x1.device, dtype=torch.bfloat16)
  buf = None
  if out8_scale > 0:
    assert not want_table
    buf, y = _guarded((B, HW, C1 + C2), torch.uint8, x1.device)
  table = torch.full((B, 2, C1 + C2), nan, device=x1.device, dtype=torch.float32) if want_table else None
  N.check(N.lib().gill_op_groupnorm_from_stats(N.ptr(x1), C1, N.ptr(x2), C2, B, HW, groups, N.ptr(g), N.ptr(b), float(eps), int(silu), N.ptr(stats1),
                                               bin1, stats1.shape[1], N.ptr(stats2), bin2, 0 if stats2 is None else stats2.shape[1],
                                               N.ptr(y if buf is None else buf), N.ptr(table), float(out8_scale), N.current_stream()))
  if buf is not None:
    return y, table, stats1, stats2, _guard_ok(buf)
  return y, table, stats1, stats2


def conv3x3_fp8(x: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                splitk: int = 0) -> torch.Tensor:
  """3x3 / pad 1 / stride 1 conv with fp8 (e4m3) activations and weights on the fp8 MFMA (csrc/conv_fp8.hip): NHWC bf16 x
  (B,H,W,Cin), OIHW fp32 weights -> NHWC bf16.  Quantisation (x * 8 per tensor, weights per output channel) happens inside."""
  x = _bf(x)
  B, H, W, Cin = x.shape
  w = w_oihw.float().contiguous()
  Cout = w.shape[0]
  assert w.shape[1] == Cin and Cin % 64 == 0
  y = torch.empty((B, H, W, Cout), device=x.device, dtype=torch.bfloat16)
  if bias is not None:
    bias = bias.float().contiguous()
  if resid is not None:
    resid = _bf(resid)
  N.check(N.lib().gill_op_conv3x3_fp8(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(resid), N.ptr(y), B, H, W, Cin, Cout, splitk,
                                      N.current_stream()))
  return y


def ffn_fused(t: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
              b2: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor, resid: torch.Tensor, rows_per_batch: int = 0,
              o2: Optional[torch.Tensor] = None, wo: Optional[torch.Tensor] = None, bo2: Optional[torch.Tensor] = None,
              ln_stats: Optional[torch.Tensor] = None, ln_rows: int = 0):
  """The feed-forward sub-block of a C = 320 transformer block + proj_out + outer residual as one kernel (csrc/ffn.hip):
  out = (t + ff2(value * gelu(gate))) @ wp.T + bp + resid with [value | gate] = LN(t) @ w1.T + b1 (diffusers layouts: w1 (2560, 320),
  w2 (320, 1280), wp (320, 320)).  t, resid (M, 320) bf16, M % 128 == 0.  Returns out (M, 320) bf16 [, GroupNorm partial sums
  (M / 64, 64, 2) fp32 when rows_per_batch > 0].  o2 / wo / bo2 (all or none): t := t + o2 @ wo.T + bo2 first, inside the kernel
  (BasicTransformerBlock.attn2.to_out + its residual; o2 (M, 320), wo (320, 320)) — the form the UNet engine runs.
  ln_stats (planes, R, 2) fp32 (not with o2): the caller's row-sum planes {sum, sum of squares} of t in place of the one plane the entry
  forms itself, R = ln_rows or M; rows m >= R read the sums of row m - R (M <= 2 R)."""
  t, w1, w2, wp, resid = (_bf(x) for x in (t, w1, w2, wp, resid))
  M = t.shape[0]
  # outputs start as NaN: the engine hands these kernels stale arena memory, so a tile the kernel forgot to write must show in a test
  out = torch.full((M, 320), float("nan"), device=t.device, dtype=torch.bfloat16)
  stats = torch.full((M // 64, 64, 2), float("nan"), device=t.device, dtype=torch.float32) if rows_per_batch else None
  f = lambda x: x.float().contiguous()
  ln_g, ln_b, b1, b2, bp = f(ln_g), f(ln_b), f(b1), f(b2), f(bp)
  if o2 is not None:       # the PRE form: t := t + o2 @ wo.T + bo2 first, inside the kernel
    o2, wo, bo2 = _bf(o2), _bf(wo), f(bo2)
  planes = 0
  if ln_stats is not None:
    assert ln_stats.is_cuda and ln_stats.dtype == torch.float32 and ln_stats.is_contiguous() and ln_stats.dim() == 3 and ln_stats.shape[2] == 2
    planes = ln_stats.shape[0]
    assert ln_stats.shape[1] == (ln_rows or M), "ln_stats: (planes, ln_rows or M, 2)"
  N.check(N.lib().gill_op_ffn_fused_ex(N.ptr(t), N.ptr(ln_g), N.ptr(ln_b), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), N.ptr(wp), N.ptr(bp),
                                       N.ptr(resid), N.ptr(out), N.ptr(stats), M, rows_per_batch, N.ptr(o2), N.ptr(wo), N.ptr(bo2),
                                       N.ptr(ln_stats), planes, ln_rows, N.current_stream()))
  return (out, stats) if rows_per_batch else out


def lnproj(mode: int, x: torch.Tensor, t, w1: torch.Tensor, b1: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w2: torch.Tensor,
           B: int, HW: int, gn_ss: Optional[torch.Tensor] = None):
  """The two projections around norm1 (mode 0) / norm2 (mode 1) of a C = 320, 8-head transformer block as one kernel (csrc/lnproj.hip).
  mode 0: t = x @ w1.T + b1; q, k, v = LN(t) @ w2.T with w2 (960, 320) = to_q | to_k | to_v.  mode 1: t = t + x @ w1.T + b1 (x = the
  attention output); q = LN(t) @ w2.T with w2 (320, 320).  Returns (t (M, 320) bf16, q, k, vt) in the attention kernels' layouts
  (q, k (B, 8, hw_pad, 48), q pre-scaled by log2(e) / sqrt(40); vt (B, 8, 64, hw_pad) with row 48 = 1); k, vt None in mode 1.
  gn_ss (B, 2, 320) fp32 (mode 0, HW % 128 == 0): the block's GroupNorm as per-sample scale | shift rows, applied to the rows of x as
  the kernel loads them (x := bf16(x * scale + shift))."""
  x, w1, w2 = (_bf(v) for v in (x, w1, w2))
  M = B * HW
  hw_pad = (HW + 31) // 32 * 32
  # outputs start as NaN (the engine passes stale arena memory): pad columns 40..47, the ones-row of V^T and every row must be WRITTEN
  nan = float("nan")
  t = torch.full((M, 320), nan, device=x.device, dtype=torch.bfloat16) if mode == 0 else _bf(t).clone()
  q = torch.full((B, 8, hw_pad, 48), nan, device=x.device, dtype=torch.bfloat16)
  k = torch.full_like(q, nan) if mode == 0 else None
  vt = torch.full((B, 8, 64, hw_pad), nan, device=x.device, dtype=torch.bfloat16) if mode == 0 else None
  f = lambda v: v.float().contiguous()
  b1, ln_g, ln_b = f(b1), f(ln_g), f(ln_b)
  if gn_ss is not None:
    assert gn_ss.is_cuda and gn_ss.dtype == torch.float32 and gn_ss.is_contiguous() and tuple(gn_ss.shape) == (B, 2, 320)
  N.check(N.lib().gill_op_lnproj_ex(mode, N.ptr(x), N.ptr(t), N.ptr(w1), N.ptr(b1), N.ptr(ln_g), N.ptr(ln_b), N.ptr(w2), N.ptr(q), N.ptr(k),
                                    N.ptr(vt), B, HW, N.ptr(gn_ss), N.current_stream()))
  return t, q, k, vt


def cross_attention_folded(t: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor,
                           wo: torch.Tensor, bo: torch.Tensor, ctx: torch.Tensor, heads: int, B: int, HW: int):
  """norm2 + attn2 + residual of a BasicTransformerBlock with heads of 80..160 features as the engine runs it at UNet levels 1-3
  (csrc/xf_weights.hip "XALG"): out = t + softmax(LN(t) wq.T (ctx wk.T).T / sqrt(d)) (ctx wv.T) wo.T + bo, computed as two GEMMs on per-sample
  weights folded from (wq, wk) and (wo, wv).  t (B * HW, C); wq, wo (C, C); wk, wv (C, E); ctx (B, ctx_len <= 80, E).
  Returns (out (B * HW, C) bf16, P (B * HW, 80 * heads) bf16: the softmax weights, key j of head h at column 80 h + j)."""
  t, wq, wk, wv, wo, ctx = (_bf(v) for v in (t, wq, wk, wv, wo, ctx))
  M, C = t.shape
  E = ctx.shape[-1]
  f = lambda v: v.float().contiguous()
  ln_g, ln_b, bo = f(ln_g), f(ln_b), f(bo)
  nan = float("nan")      # (the engine passes stale arena memory: every element must be written)
  out = torch.full((M, C), nan, device=t.device, dtype=torch.bfloat16)
  P = torch.full((M, 80 * heads), nan, device=t.device, dtype=torch.bfloat16)
  N.check(N.lib().gill_op_cross_attention_folded(N.ptr(t), N.ptr(ln_g), N.ptr(ln_b), N.ptr(wq), N.ptr(wk), N.ptr(wv), N.ptr(wo), N.ptr(bo),
                                                 N.ptr(ctx), N.ptr(out), N.ptr(P), B, HW, C, heads, ctx.shape[1], E, N.current_stream()))
  return out, P


def padded_head_dim(d: int) -> int:
  """csrc/ops.h attn_padded_dim()."""
  for dp in (48, 64, 80, 128, 160):
    if d <= dp:
      return dp
  raise ValueError(f"unsupported head dim {d}")


ROWSTATS_GUARD_ROWS = 64


def linear_rowstats(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                    a2: Optional[torch.Tensor] = None, splitk: int = 0, inplace: bool = False):
  """The GEMM that writes the residual stream at UNet levels 1-3 and files its LayerNorm row sums (include/gill_amd.h gill_op_linear_rowstats):
  t = [a | a2] @ w.T + bias + resid; a (M,K1), a2 (M,K-K1), w (N,K) bf16.  inplace: the residual is read from the output buffer itself, as the engine's
  attn1 / attn2.to_out run.  Returns (t (M,N) bf16, planes (P,M,2) fp32, P = the launcher's plane count, guard): t and planes are NaN-prefilled (not t
  when inplace), and guard = (the ROWSTATS_GUARD_ROWS rows after t, the plane after the last one), which must still be all NaN afterwards."""
  a, w = _bf(a), _bf(w)
  M, K1 = a.shape
  Nn, K = w.shape
  if a2 is not None:
    a2 = _bf(a2)
    assert a2.shape == (M, K - K1)
  nan = float("nan")
  tbuf = torch.full((M + ROWSTATS_GUARD_ROWS, Nn), nan, device=a.device, dtype=torch.bfloat16)
  if resid is not None:
    resid = _bf(resid)
    if inplace:
      tbuf[:M] = resid
      resid = tbuf
  cap = max((Nn + 63) // 64, 2 * ((Nn + 127) // 128))        # csrc/ops.h GEMM_MAX_ROW_PLANES
  planes = torch.full((cap + 1, M, 2), nan, device=a.device, dtype=torch.float32)
  if bias is not None:
    bias = bias.float().contiguous()
  npl = ctypes.c_int(0)
  N.check(N.lib().gill_op_linear_rowstats(N.ptr(a), N.ptr(a2), K1, N.ptr(w), N.ptr(bias), N.ptr(resid), N.ptr(tbuf), N.ptr(planes), cap,
                                          ctypes.byref(npl), M, Nn, K, splitk, N.current_stream()))
  P = npl.value
  return tbuf[:M], planes[:P], (tbuf[M:], planes[P:])


def ln_gemm_geglu(t: torch.Tensor, planes: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w: torch.Tensor, bias: torch.Tensor,
                  ln_rows: int = 0, splitk: int = 1) -> torch.Tensor:
  """diffusers GEGLU of LayerNorm(t) as UNet levels 1-3 run it (include/gill_amd.h gill_op_ln_gemm, mode 0): the LayerNorm folded into the weights,
  mean / rstd from the row-sum planes (P, R, 2) fp32 (R = ln_rows or M; rows >= R wrap onto row - R).  t (M,C) bf16, w (2 inner, C) bf16 in diffusers
  order, bias (2 inner).  Returns (M, inner) bf16, NaN-prefilled."""
  t, w = _bf(t), _bf(w)
  M, Cc = t.shape
  inner = w.shape[0] // 2
  planes = planes.float().contiguous()
  assert planes.is_cuda and planes.shape[1:] == (ln_rows or M, 2)
  f = lambda x: x.float().contiguous()   # noqa: E731
  ln_g, ln_b, bias = f(ln_g), f(ln_b), f(bias)
  out = torch.full((M, inner), float("nan"), device=t.device, dtype=torch.bfloat16)
  N.check(N.lib().gill_op_ln_gemm(0, N.ptr(t), N.ptr(planes), planes.shape[0], ln_rows, N.ptr(ln_g), N.ptr(ln_b), N.ptr(w), N.ptr(bias), N.ptr(out),
                                  None, None, None, M, Cc, inner, 0, 0, 0, 0, splitk, N.current_stream()))
  return out


def ln_gemm_qkv(t: torch.Tensor, planes: Optional[torch.Tensor], ln_g: Optional[torch.Tensor], ln_b: Optional[torch.Tensor], w: torch.Tensor,
                bias: Optional[torch.Tensor], heads: int, ntok: int, ln_rows: int = 0, splitk: int = 1):
  """to_q [| to_k | to_v] of LayerNorm(t) scattered head-major, as UNet levels 1-3 run it (gill_op_ln_gemm, mode 1): t (B * ntok, C) bf16, planes as
  in ln_gemm_geglu, w (nseg C, C) bf16 with nseg = 1 | 3, bias (nseg C) or None.  Returns (q, k, vt): q, k (B, heads, ntok_pad, dp) with q pre-scaled
  by log2(e) / sqrt(d), vt (B, heads, dpv, ntok_pad) with row dp = 1 where dpv > dp; k, vt None when nseg == 1.  All NaN-prefilled.
  planes, ln_g and ln_b all None: the same scatter of t itself, no LayerNorm (the OPT / CLIP engines' QKV GEMM; weight-streaming shapes run on
  the 64 x 64-blocked copy of w as in gemm())."""
  t, w = _bf(t), _bf(w)
  M, Cc = t.shape
  nseg = w.shape[0] // Cc
  d = Cc // heads
  dp = padded_head_dim(d)
  dpv, ntok_pad, B = (dp + 31) // 32 * 32, (ntok + 31) // 32 * 32, M // ntok
  f = lambda x: x.float().contiguous()   # noqa: E731
  if planes is None:
    assert ln_g is None and ln_b is None
    nplanes = 0
  else:
    planes = planes.float().contiguous()
    assert planes.is_cuda and planes.shape[1:] == (ln_rows or M, 2)
    ln_g, ln_b = f(ln_g), f(ln_b)
    nplanes = planes.shape[0]
  bias = None if bias is None else f(bias)
  nan = float("nan")
  q = torch.full((B, heads, ntok_pad, dp), nan, device=t.device, dtype=torch.bfloat16)
  k = torch.full_like(q, nan) if nseg == 3 else None
  vt = torch.full((B, heads, dpv, ntok_pad), nan, device=t.device, dtype=torch.bfloat16) if nseg == 3 else None
  N.check(N.lib().gill_op_ln_gemm(1, N.ptr(t), N.ptr(planes), nplanes, ln_rows, N.ptr(ln_g), N.ptr(ln_b), N.ptr(w), N.ptr(bias), None,
                                  N.ptr(q), N.ptr(k), N.ptr(vt), M, Cc, 0, nseg, heads, d, ntok, splitk, N.current_stream()))
  return q, k, vt


def sd_sampler_run(sampler, v_prediction: bool, num_steps: int, guidance: float, latents0: torch.Tensor, model_out: torch.Tensor,
                   noise: Optional[torch.Tensor] = None, eta: float = 0.0):
  """The denoise loop's schedule, stage kernel, step kernel and device step counter with the UNet replaced by `model_out`
  (gill_op_sd_sampler_run).  sampler: kind string or gill_amd.sd.SamplerConfig; latents0 (B,n) fp32, model_out (ncalls,Bx,n) fp32 with
  Bx = 2B when guidance > 1, noise (ncalls,B,n) fp32 or None -> (latents after every call, UNet input of every call), each (ncalls,B,n)."""
  import ctypes as C
  from .sd import as_sampler_config
  sp = as_sampler_config(sampler).native(eta)
  B, n = latents0.shape
  ncalls = N.lib().gill_sd_schedule(C.byref(sp), int(bool(v_prediction)), int(num_steps), None, None, None)
  if ncalls < 0:
    N.check(ncalls)
  Bx = 2 * B if guidance > 1.0 else B
  if tuple(model_out.shape) != (ncalls, Bx, n) or (noise is not None and tuple(noise.shape) != (ncalls, B, n)):
    raise ValueError(f"model_out must be {(ncalls, Bx, n)} and noise {(ncalls, B, n)}")
  lat0, mo = latents0.float().contiguous(), model_out.float().contiguous()
  z = None if noise is None else noise.float().contiguous()
  lat = torch.empty((ncalls, B, n), device=lat0.device, dtype=torch.float32)
  uin = torch.empty_like(lat)
  N.check(N.lib().gill_op_sd_sampler_run(C.byref(sp), int(bool(v_prediction)), int(num_steps), float(guidance), N.ptr(lat0), N.ptr(mo),
                                         None if z is None else N.ptr(z), B, n, N.ptr(lat), N.ptr(uin), N.current_stream()))
  return lat, uin


def sd_sampler_run_from(sampler, v_prediction: bool, num_steps: int, start: int, guidance: float, latents0: torch.Tensor,
                        init_noise: torch.Tensor, model_out: torch.Tensor, noise: Optional[torch.Tensor] = None, eta: float = 0.0):
  """sd_sampler_run from step `start` of the schedule (gill_op_sd_sampler_run_from): the loop begins at a * latents0 + b * init_noise, (a, b)
  the add-noise pair of gill_sd_schedule_from; model_out / noise have one row per call of THAT table."""
  import ctypes as C
  from .sd import as_sampler_config
  sp = as_sampler_config(sampler).native(eta)
  B, n = latents0.shape
  ncalls = N.lib().gill_sd_schedule_from(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), None, None, None, None)
  if ncalls < 0:
    N.check(ncalls)
  Bx = 2 * B if guidance > 1.0 else B
  if tuple(model_out.shape) != (ncalls, Bx, n) or (noise is not None and tuple(noise.shape) != (ncalls, B, n)):
    raise ValueError(f"model_out must be {(ncalls, Bx, n)} and noise {(ncalls, B, n)}")
  if tuple(init_noise.shape) != (B, n):
    raise ValueError(f"init_noise must be {(B, n)}")
  lat0, z0, mo = latents0.float().contiguous(), init_noise.float().contiguous(), model_out.float().contiguous()
  z = None if noise is None else noise.float().contiguous()
  lat = torch.empty((ncalls, B, n), device=lat0.device, dtype=torch.float32)
  uin = torch.empty_like(lat)
  N.check(N.lib().gill_op_sd_sampler_run_from(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), float(guidance), N.ptr(lat0),
                                              N.ptr(z0), N.ptr(mo), None if z is None else N.ptr(z), B, n, N.ptr(lat), N.ptr(uin),
                                              N.current_stream()))
  return lat, uin


def sd_inpaint_prepare(image: torch.Tensor, mask: torch.Tensor):
  """Mask preprocessing of the inpainting loop (gill_sd_inpaint_prepare): image (B,3,H,W) fp32 in [-1,1], mask (Bm,1,H,W) fp32 in [0,1] with
  Bm 1 or B, 1 = repaint from 0.5 up -> (masked image (B,3,H,W) = image where mask < 0.5 else 0, latent mask (B,1,H/8,W/8) in {0,1})."""
  image, mask = image.float().contiguous(), mask.float().contiguous()
  if not (image.is_cuda and mask.is_cuda and image.dim() == 4 and image.shape[1] == 3):
    raise ValueError("image must be a (B,3,H,W) tensor on the GPU, mask a (Bm,1,H,W) tensor on the GPU")
  B, _, H, W = image.shape
  if mask.dim() != 4 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (1, H, W):
    raise ValueError(f"mask must be {(B, 1, H, W)} or {(1, 1, H, W)}, got {tuple(mask.shape)}")
  masked = torch.empty_like(image)
  lmask = torch.empty((B, 1, H // 8, W // 8), device=image.device, dtype=torch.float32)
  N.check(N.lib().gill_sd_inpaint_prepare(N.ptr(image), N.ptr(mask), B, int(mask.shape[0]), H, W, N.ptr(masked), N.ptr(lmask), N.current_stream()))
  return masked, lmask


def sd_inpaint_keep(sampler, v_prediction: bool, num_steps: int, start: int = 0, eta: float = 0.0) -> torch.Tensor:
  """The blend table of gill_sd_inpaint (gill_sd_inpaint_keep; host only): (ncalls,2) float64, row i the add_noise pair (ka, kb) at the noise
  level the latents have after call i; the last row is (1, 0)."""
  import ctypes as C
  from .sd import as_sampler_config
  sp = as_sampler_config(sampler).native(eta)
  n = N.lib().gill_sd_inpaint_keep(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), None)
  if n < 0:
    N.check(n)
  buf = (C.c_double * (2 * n))()
  N.check(min(0, N.lib().gill_sd_inpaint_keep(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), buf)))
  return torch.tensor(list(buf), dtype=torch.float64).reshape(n, 2)


def sd_inpaint(handle, sampler, cond: torch.Tensor, uncond: torch.Tensor, start: int, init_latents: torch.Tensor, init_noise: torch.Tensor,
               latent_mask: torch.Tensor, masked_latents: Optional[torch.Tensor], num_steps: int, guidance: float,
               noise: Optional[torch.Tensor] = None, eta: float = 0.0) -> torch.Tensor:
  """gill_sd_inpaint on a gill_unet handle (GillSDPipeline._h): cond (B,77,D) / uncond (1|B,77,D) bf16, init_latents / init_noise (B,4,L,L) fp32,
  latent_mask (B,1,L,L) fp32 (1 = repaint), masked_latents (B,4,L,L) fp32 or None -> latents (B,4,L,L).  None selects blend mode and needs a
  handle whose UNet takes the latents alone; a tensor selects concat mode and needs a 9-channel handle: the library refuses any other pairing.
  sampler: kind string, SamplerConfig, or a gill_sd_sampler already built (eta then ignored)."""
  import ctypes as C
  from .sd import as_sampler_config
  sp = sampler if isinstance(sampler, N.gill_sd_sampler) else as_sampler_config(sampler).native(eta)
  x0, z0, lm = init_latents.float().contiguous(), init_noise.float().contiguous(), latent_mask.float().contiguous()
  B = x0.shape[0]
  if tuple(z0.shape) != tuple(x0.shape) or tuple(lm.shape) != (B, 1) + tuple(x0.shape[2:]):
    raise ValueError(f"init_noise must be {tuple(x0.shape)} and latent_mask {(B, 1) + tuple(x0.shape[2:])}")
  xm = None if masked_latents is None else masked_latents.float().contiguous()
  if xm is not None and tuple(xm.shape) != tuple(x0.shape):
    raise ValueError(f"masked_latents must be {tuple(x0.shape)}")
  cond, uncond = cond.to(torch.bfloat16).contiguous(), uncond.to(torch.bfloat16).contiguous()
  z = None if noise is None else noise.float().contiguous()
  out = torch.empty_like(x0)
  N.check(N.lib().gill_sd_inpaint(handle, C.byref(sp), N.ptr(cond), N.ptr(uncond), int(uncond.shape[0]), int(start), N.ptr(x0), N.ptr(z0), N.ptr(lm),
                                  None if xm is None else N.ptr(xm), B, int(num_steps), float(guidance), N.ptr(out),
                                  None if z is None else N.ptr(z), N.current_stream()))
  return out


def sd_inpaint_run(sampler, v_prediction: bool, num_steps: int, start: int, guidance: float, latents0: torch.Tensor, init_noise: torch.Tensor,
                   latent_mask: torch.Tensor, model_out: torch.Tensor, noise: Optional[torch.Tensor] = None, eta: float = 0.0,
                   masked_latents: Optional[torch.Tensor] = None, hw: Optional[int] = None):
  """sd_sampler_run_from with the inpainting kernels (gill_op_sd_inpaint_run): latent_mask (B,hw), 1 = repaint.  masked_latents None: blend mode
  (the blend kernel after every step); masked_latents (B,n): concat mode (the UNet input is [in_scale * latents | mask | masked_latents], no
  blend).  -> (latents after every call (ncalls,B,n), UNet input of every call (ncalls,Bx,n_in), BOTH CFG halves; n_in = n or (2 n / hw + 1) hw)."""
  import ctypes as C
  from .sd import as_sampler_config
  sp = as_sampler_config(sampler).native(eta)
  B, n = latents0.shape
  hw = int(latent_mask.shape[-1] if hw is None else hw)
  ncalls = N.lib().gill_sd_schedule_from(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), None, None, None, None)
  if ncalls < 0:
    N.check(ncalls)
  Bx = 2 * B if guidance > 1.0 else B
  if tuple(model_out.shape) != (ncalls, Bx, n) or (noise is not None and tuple(noise.shape) != (ncalls, B, n)):
    raise ValueError(f"model_out must be {(ncalls, Bx, n)} and noise {(ncalls, B, n)}")
  if tuple(init_noise.shape) != (B, n):
    raise ValueError(f"init_noise must be {(B, n)}")
  if hw < 1 or n % hw != 0 or tuple(latent_mask.shape) != (B, hw):
    raise ValueError(f"latent_mask must be {(B, hw)} with hw dividing n = {n}, got {tuple(latent_mask.shape)}")
  if masked_latents is not None and tuple(masked_latents.shape) != (B, n):
    raise ValueError(f"masked_latents must be {(B, n)}")
  f = lambda x: x.float().contiguous()   # noqa: E731
  lat0, z0, mo, lm = f(latents0), f(init_noise), f(model_out), f(latent_mask)
  xm = None if masked_latents is None else f(masked_latents)
  z = None if noise is None else f(noise)
  n_in = n if xm is None else 2 * n + hw
  lat = torch.empty((ncalls, B, n), device=lat0.device, dtype=torch.float32)
  uin = torch.empty((ncalls, Bx, n_in), device=lat0.device, dtype=torch.float32)
  N.check(N.lib().gill_op_sd_inpaint_run(C.byref(sp), int(bool(v_prediction)), int(num_steps), int(start), float(guidance), N.ptr(lat0), N.ptr(z0),
                                         N.ptr(lm), None if xm is None else N.ptr(xm), N.ptr(mo), None if z is None else N.ptr(z), B, n, hw,
                                         N.ptr(lat), N.ptr(uin), N.current_stream()))
  return lat, uin


def vae_attention(n: torch.Tensor, wqkv: torch.Tensor, bqkv: torch.Tensor, wo: torch.Tensor, bo: torch.Tensor,
                  resid: Optional[torch.Tensor] = None, want_p: bool = False):
  """The VAE mid block's single-head attention behind its GroupNorm, as the engine launches it (gill_op_vae_attention): n (B,HW,C) bf16, the
  normalised input; wqkv (3C,C) bf16 = to_q | to_k | to_v rows, bqkv (3C); wo (C,C) bf16, bo (C); resid (B,HW,C) bf16 or None.  Returns
  (out (B,HW,C) bf16, P (B,HW,HW) bf16 — the stored probabilities of every image — or None, (split-K factors of the QKV, S and PV GEMMs)); out and
  P NaN-prefilled.  want_p = False: one score buffer reused by every image, as in the engine."""
  n, wqkv, wo = _bf(n), _bf(wqkv), _bf(wo)
  B, HW, Cc = n.shape
  assert tuple(wqkv.shape) == (3 * Cc, Cc) and tuple(wo.shape) == (Cc, Cc)
  bqkv, bo = bqkv.float().contiguous(), bo.float().contiguous()
  assert bqkv.numel() == 3 * Cc and bo.numel() == Cc
  resid = None if resid is None else _bf(resid)
  assert resid is None or resid.shape == n.shape
  nan = float("nan")
  out = torch.full((B, HW, Cc), nan, device=n.device, dtype=torch.bfloat16)
  P = torch.full((B, HW, HW), nan, device=n.device, dtype=torch.bfloat16) if want_p else None
  splits = (ctypes.c_int * 3)()
  N.check(N.lib().gill_op_vae_attention(N.ptr(n), N.ptr(resid), N.ptr(wqkv), N.ptr(bqkv), N.ptr(wo), N.ptr(bo), N.ptr(out), N.ptr(P), B, HW, Cc,
                                        splits, N.current_stream()))
  return out, P, tuple(splits)


def row_softmax(s: torch.Tensor, guard_rows: int = 2):
  """Softmax over the rows of s (rows,n) bf16 with the VAE attention's in-place kernel (gill_op_row_softmax), run on a copy of s followed by
  `guard_rows` rows the kernel must not touch.  Returns (P (rows,n) bf16, the guard rows after the call, the guard rows as they were filled)."""
  s = _bf(s)
  rows, n = s.shape
  buf = torch.empty((rows + guard_rows, n), device=s.device, dtype=torch.bfloat16)
  buf[:rows] = s
  buf[rows:] = torch.arange(guard_rows * n, device=s.device).reshape(guard_rows, n).remainder(251).to(torch.bfloat16) - 125.0
  guard = buf[rows:].clone()
  N.check(N.lib().gill_op_row_softmax(N.ptr(buf), rows, n, N.current_stream()))
  return buf[:rows].clone(), buf[rows:].clone(), guard


# ---- the kernels at the ends of the engines (tests/test_ends_gpu.py).  Every output is NaN-prefilled and followed by GUARD_WORDS sentinel elements
# in the same allocation; each wrapper returns, last, whether those still hold what they were filled with.
GUARD_WORDS = 256
_GUARD_VALUE = -12352.0      # exact in bf16


_GUARD_BYTE = 0xA5           # uint8 (e4m3) buffers: pre-filled with the NaN code 0x7f, guarded by this byte


def _guarded(shape, dtype, device):
  n = 1
  for d in shape:
    n *= int(d)
  if dtype == torch.uint8:
    buf = torch.full((n + GUARD_WORDS,), 0x7F, device=device, dtype=dtype)
    buf[n:] = _GUARD_BYTE
  else:
    buf = torch.full((n + GUARD_WORDS,), float("nan"), device=device, dtype=dtype)
    buf[n:] = _GUARD_VALUE
  return buf, buf[:n].view(*shape)


def _guard_ok(buf: torch.Tensor) -> bool:
  return bool((buf[-GUARD_WORDS:] == (_GUARD_BYTE if buf.dtype == torch.uint8 else _GUARD_VALUE)).all())


def _out_buffer(shape, dtype, device, guarded: bool):
  """(buffer, output view): a _guarded() pair, or (None, torch.empty) — the wrappers' default path."""
  if guarded:
    return _guarded(shape, dtype, device)
  return None, torch.empty(shape, device=device, dtype=dtype)


# ---- the fp8 mode's launchers on quantised operands (tests/test_fp8_ops_gpu.py).  e4m3 tensors travel as uint8; every output sits in a
# guarded buffer and each wrapper returns, last, whether the guard still holds.
def _u8(t: torch.Tensor) -> torch.Tensor:
  assert t.dtype == torch.uint8 and t.is_cuda
  return t.contiguous()


def conv_fp8_kpad(cin: int) -> int:
  """Bytes per weight row of the fp8 convolution (gill_conv_fp8_kpad): 9 * cin rounded up to whole 128-byte K steps."""
  k = N.lib().gill_conv_fp8_kpad(int(cin))
  assert k > 0, "Cin must be a positive multiple of 64"
  return k


def quant_fp8(x: torch.Tensor, scale: float):
  """fp8(scale * x) of a bf16 tensor (gill_op_quant_fp8; numel % 8 == 0) -> (uint8 tensor of x's shape, guard_ok)."""
  x = _bf(x)
  buf, y = _guarded(tuple(x.shape), torch.uint8, x.device)
  N.check(N.lib().gill_op_quant_fp8(N.ptr(x), float(scale), x.numel(), N.ptr(buf), N.current_stream()))
  return y, _guard_ok(buf)


def conv_weight_quant_fp8(w_oihw: torch.Tensor, act_scale: float):
  """The fp8 convolution's weight quantiser (gill_op_conv_weight_quant_fp8): w (Cout,Cin,3,3) fp32 | bf16 | fp16 ->
  (w8 (Cout,Kpad) uint8, colscale (Cout) fp32, guard_ok)."""
  assert w_oihw.is_cuda and w_oihw.dtype in N._DTYPES and w_oihw.dim() == 4 and tuple(w_oihw.shape[2:]) == (3, 3)
  w = w_oihw.contiguous()
  Cout, Cin = w.shape[:2]
  wbuf, w8 = _guarded((Cout, conv_fp8_kpad(Cin)), torch.uint8, w.device)
  sbuf, sc = _guarded((Cout,), torch.float32, w.device)
  N.check(N.lib().gill_op_conv_weight_quant_fp8(N.ptr(w), N._DTYPES[w.dtype], Cout, Cin, float(act_scale), N.ptr(wbuf), N.ptr(sbuf),
                                                N.current_stream()))
  return w8, sc, _guard_ok(wbuf) and _guard_ok(sbuf)


def conv3x3_fp8_q(x8: torch.Tensor, w8: torch.Tensor, colscale: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  rowvec: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, splitk: int = 1, stats_bin: int = 0,
                  partials: bool = False):
  """The fp8 convolution on quantised operands, launched as UNetRun::conv8 launches it (gill_op_conv3x3_fp8_q): x8 (B,H,W,Cin) uint8, w8
  (Cout,Kpad) uint8 and colscale (Cout) from conv_weight_quant_fp8, bias (Cout), rowvec (B,Cout), resid (B,H,W,Cout) bf16.
  Returns (y (B,H,W,Cout) bf16, guard_ok); with stats_bin > 0 (y, stats, guard_ok), stats the whole NaN-prefilled buffer of
  _gn_stats_buffer of which the launch files [B][H W / 64][Cout / stats_bin][2]; with partials=True (splitk > 1) (the fp32 partials
  (splitk,M,Cout), guard_ok) and no reducer launch."""
  x8, w8 = _u8(x8), _u8(w8)
  B, H, W, Cin = x8.shape
  Cout = w8.shape[0]
  assert w8.shape[1] == conv_fp8_kpad(Cin) and colscale.dtype == torch.float32 and colscale.numel() == Cout
  f = lambda t: None if t is None else t.float().contiguous()   # noqa: E731
  colscale, bias, rowvec = colscale.contiguous(), f(bias), f(rowvec)
  assert rowvec is None or tuple(rowvec.shape) == (B, Cout)
  resid = None if resid is None else _bf(resid)
  assert (not partials or splitk > 1) and (stats_bin == 0 or splitk == 1)
  M = B * H * W
  ybuf, y = _guarded((B, H, W, Cout), torch.bfloat16, x8.device)
  wsbuf = ws = stats = None
  if splitk > 1:
    wsbuf, ws = _guarded((splitk, M, Cout), torch.float32, x8.device)
  if stats_bin > 0:
    stats = _gn_stats_buffer(B, H * W, Cout // stats_bin, x8.device)
  N.check(N.lib().gill_op_conv3x3_fp8_q(N.ptr(x8), N.ptr(w8), N.ptr(colscale), N.ptr(bias), N.ptr(rowvec), N.ptr(resid), N.ptr(ybuf), N.ptr(stats),
                                        int(stats_bin), N.ptr(wsbuf), int(partials), B, H, W, Cin, Cout, int(splitk), N.current_stream()))
  ok = _guard_ok(ybuf) and (wsbuf is None or _guard_ok(wsbuf))
  if partials:
    return ws, ok
  return (y, stats, ok) if stats_bin > 0 else (y, ok)


def groupnorm_fp8(x1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, silu: bool, scale: float,
                  x2: Optional[torch.Tensor] = None, eps: float = 1e-5):
  """fp8(scale * [silu](GroupNorm(x1 ++ x2))) with the statistics taken from the tensors (gill_op_groupnorm_fp8): x1 (B,HW,C1) bf16 ->
  (uint8 (B,HW,C1+C2), guard_ok)."""
  x1 = _bf(x1)
  B, HW, C1 = x1.shape
  x2 = None if x2 is None else _bf(x2)
  C2 = 0 if x2 is None else x2.shape[-1]
  g, b = gamma.float().contiguous(), beta.float().contiguous()
  buf, y = _guarded((B, HW, C1 + C2), torch.uint8, x1.device)
  N.check(N.lib().gill_op_groupnorm_fp8(N.ptr(x1), C1, N.ptr(x2), C2, B, HW, int(groups), N.ptr(g), N.ptr(b), float(eps), int(silu), float(scale),
                                        N.ptr(buf), N.current_stream()))
  return y, _guard_ok(buf)


def linear_weight_quant_fp8(w: torch.Tensor, act_scale: float):
  """Per-row e4m3 quantisation of bf16 rows (gill_op_linear_weight_quant_fp8): w (N,K) -> (w8 (N,K) uint8, colscale (N) fp32, guard_ok)."""
  w = _bf(w)
  Nn, K = w.shape
  wbuf, w8 = _guarded((Nn, K), torch.uint8, w.device)
  sbuf, sc = _guarded((Nn,), torch.float32, w.device)
  N.check(N.lib().gill_op_linear_weight_quant_fp8(N.ptr(w), Nn, K, float(act_scale), N.ptr(wbuf), N.ptr(sbuf), N.current_stream()))
  return w8, sc, _guard_ok(wbuf) and _guard_ok(sbuf)


def ln_quant_fp8(t: torch.Tensor, stats: torch.Tensor, ln_rows: int, eps: float, act_scale: float):
  """fp8(act_scale * LayerNorm-without-affine(t)) from row-sum planes (gill_op_ln_quant_fp8): t (M,C) bf16, stats (planes,R,2) fp32 with
  R = ln_rows or M -> (uint8 (M,C), guard_ok)."""
  t = _bf(t)
  M, Cc = t.shape
  assert stats.is_cuda and stats.dtype == torch.float32 and stats.is_contiguous() and stats.dim() == 3
  assert tuple(stats.shape[1:]) == (ln_rows if ln_rows else M, 2)
  buf, y = _guarded((M, Cc), torch.uint8, t.device)
  N.check(N.lib().gill_op_ln_quant_fp8(N.ptr(t), M, Cc, N.ptr(stats), stats.shape[0], int(ln_rows), float(eps), float(act_scale), N.ptr(buf),
                                       N.current_stream()))
  return y, _guard_ok(buf)


def geglu_fp8_q(x8: torch.Tensor, w8: torch.Tensor, colscale: torch.Tensor, bias: Optional[torch.Tensor]):
  """The fp8 GEGLU projection on quantised operands (gill_op_geglu_fp8_q): x8 (M,K), w8 (N,K) uint8 with rows, colscale (N) and bias (N) in
  the physical [16 value | 16 gate] order -> (out (M,N/2) bf16, guard_ok)."""
  x8, w8 = _u8(x8), _u8(w8)
  M, K = x8.shape
  Nn = w8.shape[0]
  assert w8.shape[1] == K and colscale.dtype == torch.float32 and colscale.numel() == Nn
  colscale = colscale.contiguous()
  bias = None if bias is None else bias.float().contiguous()
  buf, out = _guarded((M, Nn // 2), torch.bfloat16, x8.device)
  N.check(N.lib().gill_op_geglu_fp8_q(N.ptr(x8), N.ptr(w8), N.ptr(colscale), N.ptr(bias), N.ptr(buf), M, Nn, K, N.current_stream()))
  return out, _guard_ok(buf)


def conv_out(x: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor] = None, force_general: bool = False):
  """conv_out of the UNet / VAE (gill_op_conv_out): x (B,H,W,Cin) bf16 NHWC, w (Cout,Cin,3,3) fp32 | fp16 | bf16, bias (Cout) or None ->
  (y (B,Cout,H,W) fp32, path, guard_ok); path: 0 one wave per pixel, 1 MFMA with a run-time K loop, 2 | 4 | 10 MFMA with that compile-time KS."""
  x = _bf(x)
  B, H, W, Cin = x.shape
  w = w_oihw.contiguous()
  Cout = w.shape[0]
  assert tuple(w.shape) == (Cout, Cin, 3, 3) and w.dtype in N._DTYPES
  bias = None if bias is None else bias.float().contiguous()
  buf, y = _guarded((B, Cout, H, W), torch.float32, x.device)
  path = ctypes.c_int(-1)
  N.check(N.lib().gill_op_conv_out(N.ptr(x), N.ptr(w), N._DTYPES[w.dtype], N.ptr(bias), N.ptr(buf), B, H, W, Cin, Cout, int(force_general),
                                   ctypes.byref(path), N.current_stream()))
  return y, path.value, _guard_ok(buf)


def conv_in(x: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None, nzero: int = 0,
            wide: bool = False):
  """conv_in of the UNet / VAE (gill_op_conv_in: im2col + the K = 64 GEMM): x (B,Cin,H,W) fp32 NCHW, w (Cout,Cin,3,3) -> (y (B,H,W,Cout) bf16
  NHWC, guard_ok).  counters: an int32 tensor whose first nzero words the im2col launch clears (in place).  wide: gill_op_conv_in_wide, K padded
  to a multiple of 64 (up to 14 input channels: the 9-channel inpainting UNet's conv_in)."""
  assert x.dtype == torch.float32 and x.is_cuda
  x = x.contiguous()
  B, Cin, H, W = x.shape
  w = w_oihw.contiguous()
  Cout = w.shape[0]
  assert tuple(w.shape) == (Cout, Cin, 3, 3) and w.dtype in N._DTYPES
  bias = None if bias is None else bias.float().contiguous()
  assert counters is None or (counters.dtype == torch.int32 and counters.numel() >= nzero)
  buf, y = _guarded((B, H, W, Cout), torch.bfloat16, x.device)
  fn = N.lib().gill_op_conv_in_wide if wide else N.lib().gill_op_conv_in
  N.check(fn(N.ptr(x), N.ptr(w), N._DTYPES[w.dtype], N.ptr(bias), N.ptr(buf), B, Cin, H, W, Cout, N.ptr(counters), int(nzero), N.current_stream()))
  return y, _guard_ok(buf)


def timestep_embed(t: torch.Tensor, dim: int):
  """diffusers Timesteps (gill_op_timestep_embed): t (n) fp32 -> (out (n, dim) bf16 = [cos | sin], guard_ok)."""
  assert t.dtype == torch.float32 and t.is_cuda and t.dim() == 1
  t = t.contiguous()
  buf, out = _guarded((t.numel(), dim), torch.bfloat16, t.device)
  N.check(N.lib().gill_op_timestep_embed(N.ptr(t), t.numel(), int(dim), N.ptr(buf), N.current_stream()))
  return out, _guard_ok(buf)


def reduce_ln(ws: torch.Tensor, sk: int, bias: torch.Tensor, h: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float = 1e-5):
  """The transformer block's split-K reducer + bias + fp32 residual + LayerNorm (gill_op_reduce_ln): ws (>= sk, M, D) fp32 of which the first sk
  slices are summed, h (M, D) fp32 (not modified: the kernel updates a copy) -> (new h (M,D) fp32, nb (M,D) bf16, guard_ok)."""
  M, D = h.shape
  assert ws.dtype == torch.float32 and ws.is_cuda and ws.is_contiguous() and ws.shape[0] >= sk and tuple(ws.shape[1:]) == (M, D)
  f = lambda x: x.float().contiguous()   # noqa: E731
  bias, g, b = f(bias), f(g), f(b)
  hbuf, hn = _guarded((M, D), torch.float32, h.device)
  hn.copy_(h)
  nbuf, nb = _guarded((M, D), torch.bfloat16, h.device)
  N.check(N.lib().gill_op_reduce_ln(N.ptr(ws), int(sk), M, D, N.ptr(bias), N.ptr(hbuf), N.ptr(g), N.ptr(b), N.ptr(nbuf), float(eps),
                                    N.current_stream()))
  return hn, nb, _guard_ok(hbuf) and _guard_ok(nbuf)


def linear_reduce_ln(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, h: torch.Tensor, g: torch.Tensor, b: torch.Tensor, splitk: int,
                     fuse: bool):
  """h + a @ w.T + bias into the fp32 stream and the LayerNorm (eps 1e-5) behind it, split `splitk` ways, as the pre-LN transformer block runs it
  (gill_op_linear_reduce_ln): fuse=True partials + the reducer of reduce_ln, fuse=False the GEMM's own reducer + the stand-alone LayerNorm.
  a (M,K) bf16, w (N,K) bf16, h (M,N) fp32 (not modified) -> (new h, nb (M,N) bf16, guard_ok)."""
  a, w = _bf(a), _bf(w)
  M, K = a.shape
  Nn = w.shape[0]
  assert tuple(h.shape) == (M, Nn) and w.shape[1] == K
  f = lambda x: x.float().contiguous()   # noqa: E731
  bias, g, b = f(bias), f(g), f(b)
  hbuf, hn = _guarded((M, Nn), torch.float32, a.device)
  hn.copy_(h)
  nbuf, nb = _guarded((M, Nn), torch.bfloat16, a.device)
  N.check(N.lib().gill_op_linear_reduce_ln(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(hbuf), N.ptr(g), N.ptr(b), N.ptr(nbuf), M, Nn, K, int(splitk),
                                           int(bool(fuse)), N.current_stream()))
  return hn, nb, _guard_ok(hbuf) and _guard_ok(nbuf)


def skinny_gemm(x: torch.Tensor, w: torch.Tensor):
  """The lm_head GEMV (gill_op_skinny_gemm): x (M,K) bf16, w (N,K) bf16 -> (out (M,N) fp32, guard_ok)."""
  x, w = _bf(x), _bf(w)
  M, K = x.shape
  Nn = w.shape[0]
  assert w.shape[1] == K
  buf, out = _guarded((M, Nn), torch.float32, x.device)
  N.check(N.lib().gill_op_skinny_gemm(N.ptr(x), N.ptr(w), N.ptr(buf), M, Nn, K, N.current_stream()))
  return out, _guard_ok(buf)


def _as_hwc_u8(img):
  """One image of clip_preprocess -> an (H,W,3) uint8 numpy array (host) or torch tensor (host or device)."""
  import numpy as np
  if type(img).__module__.startswith('PIL'):
    return np.asarray(img.convert('RGB'), dtype=np.uint8)
  if isinstance(img, (np.ndarray, torch.Tensor)):
    if img.dtype not in (np.uint8, torch.uint8) or img.ndim != 3 or img.shape[2] != 3:
      raise ValueError(f'clip_preprocess takes (H,W,3) uint8 images, got {tuple(img.shape)} {img.dtype}')
    return img
  raise ValueError(f'clip_preprocess takes PIL images, uint8 arrays or uint8 tensors, got {type(img)}')


def clip_preprocess(images, size: int, device, return_u8: bool = False):
  """The CLIP image preprocessing of utils.ClipImageProcessor(size, size) on the device (gill_clip_preprocess): Pillow's BICUBIC resize of the
  shortest edge to `size`, centre crop, x / 255, (x - mean) / std.  images: a list of PIL images (convert('RGB')), (H,W,3) uint8 arrays or uint8
  tensors on the host or the device, of any sizes, or one (B,H,W,3) uint8 tensor — on the device (decode_latents' output) it goes through without
  touching the host.  Host images are packed into one buffer and uploaded in one copy.  Returns (n,3,size,size) fp32 and, with return_u8, the
  cropped (n,size,size,3) uint8 pixels before normalisation, equal to Pillow's."""
  import numpy as np
  device = torch.device(device)
  if isinstance(images, torch.Tensor) and images.dim() == 4:
    if images.dtype != torch.uint8 or images.shape[3] != 3:
      raise ValueError(f'clip_preprocess takes (B,H,W,3) uint8 tensors, got {tuple(images.shape)} {images.dtype}')
    n, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    shapes = [(H, W)] * n
    offs = {i: i * H * W * 3 for i in range(n)}
    packed = images.to(device).contiguous().reshape(-1)
  else:
    items = [_as_hwc_u8(im) for im in images]
    shapes = [(int(a.shape[0]), int(a.shape[1])) for a in items]
    on_dev = [isinstance(a, torch.Tensor) and a.is_cuda for a in items]
    # host images first, in one staging buffer and one upload; images already on the device are copied there behind them
    order = [i for i, d in enumerate(on_dev) if not d] + [i for i, d in enumerate(on_dev) if d]
    offs, total = {}, 0
    for i in order:
      offs[i] = total
      total += shapes[i][0] * shapes[i][1] * 3
    host_bytes = sum(shapes[i][0] * shapes[i][1] * 3 for i, d in enumerate(on_dev) if not d)
    packed = torch.empty(max(total, 1), device=device, dtype=torch.uint8)
    if host_bytes:
      stage = np.empty(host_bytes, dtype=np.uint8)
      for i in order:
        if not on_dev[i]:
          a = items[i].numpy() if isinstance(items[i], torch.Tensor) else items[i]
          stage[offs[i]:offs[i] + a.size] = a.reshape(-1)
      packed[:host_bytes].copy_(torch.from_numpy(stage))
    for i in order:
      if on_dev[i]:
        packed[offs[i]:offs[i] + items[i].numel()].copy_(items[i].reshape(-1))
    n = len(items)
  if n == 0:
    raise ValueError('clip_preprocess: no images')
  meta = (ctypes.c_int64 * (3 * n))()
  for i in range(n):
    meta[3 * i], meta[3 * i + 1], meta[3 * i + 2] = offs[i], shapes[i][0], shapes[i][1]
  need = ctypes.c_int64(0)
  N.check(N.lib().gill_clip_preprocess_workspace(meta, n, int(size), ctypes.byref(need)))
  ws = torch.empty(need.value, device=device, dtype=torch.uint8)
  out = torch.empty((n, 3, size, size), device=device, dtype=torch.float32)
  u8 = torch.empty((n, size, size, 3), device=device, dtype=torch.uint8) if return_u8 else None
  with torch.cuda.device(device):
    N.check(N.lib().gill_clip_preprocess(N.ptr(packed), packed.numel(), meta, n, int(size), int(size), N.ptr(out), N.ptr(u8), N.ptr(ws), need.value,
                                         N.current_stream()))
  return (out, u8) if return_u8 else out


def lm_loss_geometry(M: int, V: int, D: int):
  """(row_tile, col_tile, n_slabs, cols_per_slab) of lm_head_loss at this shape (host only: gill_lm_loss_geometry)."""
  out = [ctypes.c_int() for _ in range(4)]
  N.check(N.lib().gill_lm_loss_geometry(int(M), int(V), int(D), *[ctypes.byref(o) for o in out]))
  return tuple(o.value for o in out)


def gemm_plan(cases, pp: int = 1, coop: int = 1, cus: int = 256):
  """What the GEMM launcher decides for each case (host only: gill_gemm_plan).  cases (n, 54) int32 descriptors -> (n, 34) int32 rows; the
  field orders are in include/gill_amd.h.  pp / coop / cus: GILL_GEMM_PP, GILL_GEMM_COOP and the CU count the plan is made for."""
  import numpy as np
  cases = np.ascontiguousarray(cases, dtype=np.int32).reshape(-1, 54)
  rows = np.zeros((cases.shape[0], 34), dtype=np.int32)
  N.check(N.lib().gill_gemm_plan(cases.ctypes.data, cases.shape[0], int(pp), int(coop), int(cus), rows.ctypes.data))
  return rows


def gemm_plan_log():
  """What the GEMM launcher ran on this thread since the previous call (host only: gill_gemm_plan_log): (rows, launched) — the plans of the
  most recent min(32, launched) launches, oldest first, as (n, 34) int32 rows in gemm_plan()'s layout, and the number of launches.  Clears
  the record."""
  import numpy as np
  rows = np.zeros((32, 34), dtype=np.int32)
  launched = ctypes.c_int(0)
  N.check(N.lib().gill_gemm_plan_log(rows.ctypes.data, 32, ctypes.byref(launched)))
  return rows[:min(32, launched.value)].copy(), launched.value


def unet_xf_plan(cases, lnproj: int = 1, xalg: int = 1, ffn_fused: int = 1):
  """Which kernels a UNet transformer block runs (host only: gill_unet_xf_plan).  cases (n, 8) int32 = [C, heads, ctx_len, ctx_dim, hw, fp8, Bx,
  shared] -> (n, 11) int32 rows = the load-time forms [lnproj, xalg, ffn_fused, ffn_pre, geglu_fp8] + the call's plan [lnproj, gn_table, cross, ffn,
  M, M1]; include/gill_amd.h has the codes.  lnproj / xalg / ffn_fused: GILL_UNET_LNPROJ, GILL_UNET_XALG, GILL_UNET_FFN_FUSED."""
  import numpy as np
  cases = np.ascontiguousarray(cases, dtype=np.int32).reshape(-1, 8)
  rows = np.zeros((cases.shape[0], 11), dtype=np.int32)
  N.check(N.lib().gill_unet_xf_plan(cases.ctypes.data, cases.shape[0], int(lnproj), int(xalg), int(ffn_fused), rows.ctypes.data))
  return rows


def attention_plan(B: int, H: int, nq: int, nkv: int, d: int, causal: bool = False, att_dma: int = 1):
  """Which kernel attention() runs for a shape (host only: gill_attention_plan): (family, dp, nthr, grid) — family 0 the register-staged
  attention_kernel<dp, nthr>, 1 the LDS-DMA attention_dma_kernel<dp, nthr>; grid in workgroups.  att_dma: GILL_ATT_DMA."""
  import numpy as np
  out = np.zeros(4, dtype=np.int32)
  N.check(N.lib().gill_attention_plan(int(B), int(H), int(nq), int(nkv), int(d), int(causal), int(att_dma), out.ctypes.data))
  return tuple(int(x) for x in out)


def gemm_query(queries, pp: int = 1, coop: int = 1, cus: int = 256):
  """The engines' pre-launch GEMM choices (host only: gill_gemm_query).  queries (n, 7) int32 = [what, six arguments] -> (n,) int32."""
  import numpy as np
  queries = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 7)
  out = np.zeros(queries.shape[0], dtype=np.int32)
  N.check(N.lib().gill_gemm_query(queries.ctypes.data, queries.shape[0], int(pp), int(coop), int(cus), out.ctypes.data))
  return out


def lm_head_loss(x: torch.Tensor, w: torch.Tensor, target: torch.Tensor, check: bool = True):
  """The LM-head loss without a logits tensor (gill_op_lm_head_loss): x (M,D) bf16, w (V,D) bf16, target (M) int64 with -100 = ignore ->
  (lse (M) fp32, tgt (M) fp32, rank (M) int32, summary (4) fp32 = [mean of lse - tgt over valid rows, n_valid, #rank < 1, #rank < 5]).
  rank counts the columns in front of the target (larger logit first, lower index on a tie); ignored rows: rank -1, lse = tgt = 0.
  check: refuse targets outside [0, V) other than -100 here (one host read); the library can only clamp them."""
  x, w = _bf(x), _bf(w)
  M, D = x.shape
  V = w.shape[0]
  assert w.shape[1] == D and target.shape == (M,)
  target = target.to(x.device, torch.int64).contiguous()
  if check and M:
    bad = (target != -100) & ((target < 0) | (target >= V))
    if bool(bad.any()):
      raise ValueError(f'target {int(target[bad][0])} is neither -100 nor a column of [0, {V})')
  lse = torch.empty((M,), device=x.device, dtype=torch.float32)
  tgt = torch.empty((M,), device=x.device, dtype=torch.float32)
  rank = torch.empty((M,), device=x.device, dtype=torch.int32)
  summary = torch.empty((4,), device=x.device, dtype=torch.float32)
  N.check(N.lib().gill_op_lm_head_loss(N.ptr(x), N.ptr(w), N.ptr(target), M, V, D, N.ptr(lse), N.ptr(tgt), N.ptr(rank), N.ptr(summary),
                                       N.current_stream()))
  return lse, tgt, rank, summary


# ---- the quantised decoder's format and linear (csrc/linear_w8.hip; tests/test_w8_ops_gpu.py).  Bytes travel as uint8 in the kernel's order.
def w8_max_rows() -> int:
  """W8_MAX_ROWS: the most activation rows linear_w8 takes."""
  return int(N.lib().gill_w8_max_rows())


def w8_quant(w: torch.Tensor):
  """bf16 (N,K) -> (w8 (N*K) uint8 in the kernel's order, scale (N) fp32 powers of two, guard_ok) (gill_op_w8_quant)."""
  w = _bf(w)
  Nn, K = w.shape
  wbuf, w8 = _guarded((Nn * K,), torch.uint8, w.device)
  sbuf, sc = _guarded((Nn,), torch.float32, w.device)
  N.check(N.lib().gill_op_w8_quant(N.ptr(w), Nn, K, N.ptr(wbuf), N.ptr(sbuf), N.current_stream()))
  return w8, sc, _guard_ok(wbuf) and _guard_ok(sbuf)


def w8_dequant(w8: torch.Tensor, scale: torch.Tensor, Nn: int, K: int, blk64: bool = False):
  """The bytes of w8_quant -> (bf16 (N,K) row-major, or with blk64 the 64 x 64-blocked order as a flat (N*K) tensor, guard_ok)."""
  w8 = _u8(w8)
  assert w8.numel() == Nn * K and scale.dtype == torch.float32 and scale.numel() == Nn
  buf, out = _guarded((Nn * K,) if blk64 else (Nn, K), torch.bfloat16, w8.device)
  N.check(N.lib().gill_op_w8_dequant(N.ptr(w8), N.ptr(scale.contiguous()), Nn, K, int(blk64), N.ptr(buf), N.current_stream()))
  return out, _guard_ok(buf)


def linear_w8(a: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
              act: str = "none", out_f32: bool = False, splitk: int = 0, ln: Optional[tuple] = None, out_rows: Optional[int] = None,
              canary: float = 0.0):
  """act(scale * (a @ bf16(w8).T) + bias) (+ resid) (gill_op_linear_w8): a (M,K) bf16, w8 / scale from w8_quant, bias (N) fp32, resid (M,N) fp32
  (added in place in a copy: the result is the updated residual).  ln = (gamma, beta): the split-partials + reducer + LayerNorm finish
  (needs bias and resid) -> (new resid fp32, LayerNorm bf16, guard_ok).  Otherwise -> (out (M,N), guard_ok).  out_rows > M: the output buffer
  has out_rows rows, filled with `canary` beforehand, and all of them are returned."""
  a, w8 = _bf(a), _u8(w8)
  M, K = a.shape
  Nn = scale.numel()
  assert w8.numel() == Nn * K and scale.dtype == torch.float32
  R = M if out_rows is None else int(out_rows)
  f = lambda x: None if x is None else x.float().contiguous()   # noqa: E731
  bias = f(bias)
  odt = torch.float32 if (out_f32 or resid is not None) else torch.bfloat16
  buf, out = _guarded((R, Nn), odt, a.device)
  if out_rows is not None:
    out.fill_(canary)
  rp = None
  if resid is not None:
    assert resid.dtype == torch.float32 and tuple(resid.shape) == (M, Nn)
    out[:M].copy_(resid)
    rp = N.ptr(buf)
  if ln is not None:
    g, b = f(ln[0]), f(ln[1])
    nbuf, nb = _guarded((M, Nn), torch.bfloat16, a.device)
    N.check(N.lib().gill_op_linear_w8(N.ptr(a), N.ptr(w8), N.ptr(scale.contiguous()), N.ptr(bias), rp, N.ptr(buf), M, Nn, K, ACT[act], 1, int(splitk),
                                      N.ptr(g), N.ptr(b), N.ptr(nbuf), N.current_stream()))
    return out, nb, _guard_ok(buf) and _guard_ok(nbuf)
  N.check(N.lib().gill_op_linear_w8(N.ptr(a), N.ptr(w8), N.ptr(scale.contiguous()), N.ptr(bias), rp, N.ptr(buf), M, Nn, K, ACT[act],
                                    int(odt == torch.float32), int(splitk), None, None, None, N.current_stream()))
  return out, _guard_ok(buf)


# ---- the image-block heads and the rerank score (csrc/img_heads.hip; tests/test_img_heads_gpu.py)
def img_block_heads(hidden: torch.Tensor, row_idx: torch.Tensor, ret: Optional[tuple] = None, decision: Optional[tuple] = None, _out=None):
  """What generate_for_images_and_texts computes from a block's first [IMG] hidden state, for n blocks in one launch (gill_op_img_block_heads).
  hidden (..., D) fp32 on the device (generate_batch's `hidden`; read as (rows, D)), row_idx (n,) int32 on the device: the flat rows, any order,
  repeats allowed, clamped into [0, rows) on the device.  ret = (W (E, D) bf16, b (E) fp32): ret_emb (n, E) fp32 = y / ||y||, y = W bf16(x) + b.
  decision = (W (C, D) bf16, b (C) fp32), C <= 4: probs (n, C) fp32 = softmax(z) and choice (n,) int32 = argmax z (tie: lower index).  Returns
  (ret_emb | None, probs | None, choice | None).  No host wait.  _out: caller-allocated (ret_emb, probs, choice) (the tests pass guarded ones)."""
  assert hidden.is_cuda and hidden.dtype == torch.float32 and hidden.dim() >= 2
  hidden = hidden.contiguous()
  D = int(hidden.shape[-1])
  rows = hidden.numel() // max(1, D)
  assert row_idx.is_cuda and row_idx.dtype == torch.int32 and row_idx.dim() == 1
  row_idx = row_idx.contiguous()
  n = int(row_idx.shape[0])
  dev = hidden.device

  def pair(p, name):
    if p is None:
      return None, None, 0
    w, b = _bf(p[0]), p[1].to(dev, torch.float32).contiguous()
    if w.dim() != 2 or w.shape[1] != D or b.shape != (w.shape[0],):
      raise ValueError(f'img_block_heads: {name} is (W (cols, {D}) bf16, b (cols,)), got {tuple(w.shape)} and {tuple(b.shape)}')
    return w, b, int(w.shape[0])
  wr, br, E = pair(ret, 'ret')
  wd, bd, Cc = pair(decision, 'decision')
  if _out is not None:
    ret_emb, probs, choice = _out
  else:
    ret_emb = torch.empty((n, E), device=dev, dtype=torch.float32) if ret is not None else None
    probs = torch.empty((n, Cc), device=dev, dtype=torch.float32) if decision is not None else None
    choice = torch.empty((n,), device=dev, dtype=torch.int32) if decision is not None else None
  with torch.cuda.device(dev):
    N.check(N.lib().gill_op_img_block_heads(N.ptr(hidden), rows, D, N.ptr(row_idx), n, N.ptr(wr), N.ptr(br), E, N.ptr(wd), N.ptr(bd), Cc,
                                            N.ptr(ret_emb), N.ptr(probs), N.ptr(choice), N.current_stream()))
  return ret_emb, probs, choice


def img_rerank_scores(visual: torch.Tensor, ret_emb: torch.Tensor, _out: Optional[torch.Tensor] = None) -> torch.Tensor:
  """The CLIP rerank score of generated images (gill_op_img_rerank_scores): visual (n * g, E) fp32 un-normalised rows, block b's images at rows
  b g .. b g + g - 1, ret_emb (n, E) fp32 -> scores (n, g) fp32 = the cosine of each image's row with its block's ret_emb; zero rows give 0.
  One launch, no host wait."""
  assert visual.is_cuda and visual.dtype == torch.float32 and visual.dim() == 2
  assert ret_emb.is_cuda and ret_emb.dtype == torch.float32 and ret_emb.dim() == 2 and ret_emb.shape[1] == visual.shape[1]
  visual, ret_emb = visual.contiguous(), ret_emb.contiguous()
  n, E = int(ret_emb.shape[0]), int(ret_emb.shape[1])
  if n == 0 or visual.shape[0] % n != 0 or visual.shape[0] == 0:
    raise ValueError(f'img_rerank_scores: visual holds {visual.shape[0]} rows for {n} blocks')
  g = int(visual.shape[0]) // n
  scores = torch.empty((n, g), device=visual.device, dtype=torch.float32) if _out is None else _out
  assert scores.shape == (n, g) and scores.dtype == torch.float32 and scores.is_contiguous()
  with torch.cuda.device(visual.device):
    N.check(N.lib().gill_op_img_rerank_scores(N.ptr(visual), N.ptr(ret_emb), n, g, E, N.ptr(scores), N.current_stream()))
  return scores
