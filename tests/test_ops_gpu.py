"""Operator-level parity: every HIP kernel of libgill_amd against a plain fp32 torch-CPU statement of
the same op, on the same bf16-rounded inputs.  Inputs are asymmetric random so a transposed MFMA
fragment or a swapped row/column cannot pass."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rnd(shape, seed, scale=1.0):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(shape, generator=g) * scale)


def _bf(x):
  return x.to(torch.bfloat16)


def _report(name, got, ref):
  got, ref = got.float().cpu(), ref.float().cpu()
  err = (got - ref).abs()
  rel = err.max().item() / max(ref.abs().max().item(), 1e-6)
  print(f"[{name}] max_abs={err.max().item():.4e} rel_to_max={rel:.4e} mse={(err**2).mean().item():.4e}")
  return rel


# ---------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 320, 128), (100, 132, 192), (8, 512, 4096), (616, 768, 512),
                                   (1024, 1280, 1280), (77, 1536, 512)])
def test_gemm_plain(cuda, M, N, K):
  from gill_amd import ops
  a, w = _bf(_rnd((M, K), 1)), _bf(_rnd((N, K), 2, 0.1))
  bias = _rnd((N,), 3)
  ref = a.float() @ w.float().T + bias
  out = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), splitk=1)
  assert _report(f"gemm {M}x{N}x{K}", out, ref) < 1e-2
  out32 = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), out_f32=True, splitk=1)
  assert _report(f"gemm f32out {M}x{N}x{K}", out32, ref) < 1e-4


@pytest.mark.parametrize("M,N,K,sk", [(4096, 320, 1600, 1), (1024, 640, 3200, 1), (512, 1280, 6400, 2), (384, 320, 1600, 3)])
def test_gemm_long_k_with_residual(cuda, M, N, K, sk):
  """The shapes of the UNet's fused feed-forward output GEMMs (N = 320 .. 1280, K = 5 N), with residual, unsplit and split-K.
  N % 160 == 0, M % 128 == 0, K >= 2560 run on the convolutions' 8-wave ping-pong tiles (gemm_plain_pingpong(), gemm.hip): cases 2 and 3."""
  from gill_amd import ops
  a, w = _bf(_rnd((M, K), 11)), _bf(_rnd((N, K), 12, 0.05))
  bias, resid = _rnd((N,), 13), _bf(_rnd((M, N), 14))
  ref = a.float() @ w.float().T + bias + resid.float()
  out = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), resid=resid.to(cuda), splitk=sk)
  assert _report(f"gemm long-K {M}x{N}x{K} sk{sk}", out, ref) < 1e-2


@pytest.mark.parametrize("act", ["relu", "silu", "gelu"])
def test_gemm_epilogue(cuda, act):
  from gill_amd import ops
  M, N, K = 200, 256, 256
  a, w = _bf(_rnd((M, K), 4)), _bf(_rnd((N, K), 5, 0.1))
  bias, resid = _rnd((N,), 6), _bf(_rnd((M, N), 7))
  pre = 0.5 * (a.float() @ w.float().T) + bias + resid.float()
  ref = {"relu": F.relu, "silu": F.silu, "gelu": F.gelu}[act](pre)
  out = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), resid=resid.to(cuda), alpha=0.5, act=act, out_f32=True, splitk=1)
  assert _report(f"gemm epi {act}", out, ref) < 1e-4


@pytest.mark.parametrize("M,N,K,sk", [(64, 512, 4096, 8), (130, 384, 1024, 4), (512, 1280, 11520, 9)])
def test_gemm_splitk(cuda, M, N, K, sk):
  from gill_amd import ops
  a, w = _bf(_rnd((M, K), 8)), _bf(_rnd((N, K), 9, 0.05))
  bias = _rnd((N,), 10)
  ref = F.relu(a.float() @ w.float().T + bias)
  out = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), act="relu", out_f32=True, splitk=sk)
  assert _report(f"gemm splitk{sk} {M}x{N}x{K}", out, ref) < 1e-4
  out_auto = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), act="relu", out_f32=True, splitk=0)
  assert _report(f"gemm splitk auto {M}x{N}x{K}", out_auto, ref) < 1e-4
  #  the skinny long-K cases reroute to the 64 x 64-blocked STREAM64 copy by default: pin the general row-major tiles on them too
  out_rm = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), act="relu", out_f32=True, splitk=sk, row_major=True)
  assert _report(f"gemm splitk{sk} {M}x{N}x{K} (row-major tiles)", out_rm, ref) < 1e-4


@pytest.mark.parametrize("M,N,K,sk", [(128, 4096, 4096, 0), (128, 2048, 2048, 1), (8, 4096, 1024, 0), (100, 1024, 4096, 3), (200, 2048, 2048, 0),
                                      (256, 4096, 1024, 2), (1, 4096, 4096, 0), (64, 1024, 8256, 0)])     # (last: K / 64 = 129 steps, no empty trailing split)
def test_gemm_stream64_blocked_weights(cuda, M, N, K, sk):
  """STREAM64 (gemm.hip): weight-streaming shapes (N K >= 4 Mi elements, K >= 1024) at <= 256 rows run on a 64 x 64-blocked copy of W —
  gill_op_gemm makes the copy with the engine's own relayout kernel (convert_to_bf16_blk64_launch), so this checks the relayout, the
  blocked K walk (whole, split: sk, heuristic: 0), one and two M tiles, ragged row counts, and the ReLU / fp32 epilogues, against torch."""
  from gill_amd import ops
  a, w = _bf(_rnd((M, K), 21)), _bf(_rnd((N, K), 22, 0.05))
  bias = _rnd((N,), 23)
  pre = a.float() @ w.float().T + bias
  out = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), act="relu", out_f32=True, splitk=sk)
  assert _report(f"gemm stream64 relu f32 {M}x{N}x{K} sk{sk}", out, F.relu(pre)) < 1e-4
  out16 = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), splitk=sk)
  assert _report(f"gemm stream64 bf16 {M}x{N}x{K} sk{sk}", out16, pre) < 1e-2
  again = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), splitk=sk)
  assert torch.equal(out16, again)
  out_rm = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), splitk=sk, row_major=True)      # the same shape on the general tiles
  assert _report(f"gemm row-major tiles bf16 {M}x{N}x{K} sk{sk}", out_rm, pre) < 1e-2


@pytest.mark.parametrize("M,N,K,sk", [(512, 4096, 1024, 0), (512, 1024, 4096, 0), (384, 2048, 2048, 2), (1000, 4096, 1024, 0), (260, 1600 + 64 * 7, 4096, 0)])
def test_gemm_blocked_weights_on_the_general_tiles(cuda, M, N, K, sk):
  """above 256 rows a GEMM on 64 x 64-blocked weights leaves the STREAM64 tile (CU-bound per M tile) for the general tiles, which read the
  blocked layout themselves (gemm.hip `wblk`: only the weight pointers differ).  Same tiles, same K order as on row-major weights, so the two
  results must be bit-identical; vs torch as usual.  (OPT prefills of 16 prompts and long get_log_likelihood_scores sequences take this path.)"""
  from gill_amd import ops
  a, w = _bf(_rnd((M, K), 31)), _bf(_rnd((N, K), 32, 0.05))
  bias = _rnd((N,), 33)
  pre = a.float() @ w.float().T + bias
  out = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), act="relu", out_f32=True, splitk=sk)
  assert _report(f"gemm blocked / general tiles relu f32 {M}x{N}x{K} sk{sk}", out, F.relu(pre)) < 1e-4
  out_rm = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), act="relu", out_f32=True, splitk=sk, row_major=True)
  assert torch.equal(out, out_rm)
  out16 = ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), splitk=sk)
  assert _report(f"gemm blocked / general tiles bf16 {M}x{N}x{K} sk{sk}", out16, pre) < 1e-2
  assert torch.equal(out16, ops.gemm(a.to(cuda), w.to(cuda), bias.to(cuda), splitk=sk, row_major=True))


def test_geglu(cuda):
  from gill_amd import ops
  M, K, inner = 192, 320, 1280
  a, w = _bf(_rnd((M, K), 11)), _bf(_rnd((2 * inner, K), 12, 0.1))
  bias = _rnd((2 * inner,), 13)
  proj = a.float() @ w.float().T + bias
  h, g = proj.chunk(2, dim=-1)
  ref = h * F.gelu(g)
  out = ops.geglu(a.to(cuda), w.to(cuda), bias.to(cuda))
  assert _report("geglu", out, ref) < 1e-2


# ---------------------------------------------------------------- conv3x3
def _conv_ref(x1, x2, w, bias, rowvec, resid, stride, ups):
  x = x1.float() if x2 is None else torch.cat([x1.float(), x2.float()], dim=-1)
  x = x.permute(0, 3, 1, 2)
  if ups:
    x = F.interpolate(x, scale_factor=2.0, mode="nearest")
  wq = w.to(torch.bfloat16).float()
  y = F.conv2d(x, wq, bias, stride=stride, padding=1)
  if rowvec is not None:
    y = y + rowvec[:, :, None, None]
  y = y.permute(0, 2, 3, 1)
  if resid is not None:
    y = y + resid.float()
  return y


@pytest.mark.parametrize("B,H,W,C1,C2,Cout,stride,ups", [
  (2, 16, 16, 64, 0, 128, 1, 0),
  (2, 16, 16, 320, 0, 320, 1, 0),
  (1, 12, 20, 128, 64, 160, 1, 0),     # non-square, two-source concat, BN=160 path
  (2, 16, 16, 128, 0, 128, 2, 0),      # downsample
  (2, 8, 8, 128, 0, 128, 1, 1),        # fused nearest-2x upsample
  (3, 8, 8, 640, 640, 640, 1, 0),
  # M % 256 == 0 and Cout % 160 == 0: the 256 x 160 ping-pong kernel (gemm_kernel<8,160,CONV,EPI,3>)
  (4, 8, 8, 64, 0, 160, 1, 0),         # one N tile, 9 K steps (3 per split at sk 3)
  (2, 16, 16, 128, 64, 160, 1, 0),     # two-source concat
  (4, 32, 32, 128, 0, 160, 2, 0),      # stride 2
  (2, 8, 8, 128, 0, 320, 1, 1),        # fused nearest-2x upsample
  # full-width maps on the ping-pong tiles
  (8, 64, 64, 128, 0, 320, 1, 0),      # 256-row tiles, 64-wide rows
  (16, 32, 32, 64, 64, 640, 1, 0),     # 256-row tiles, 32-wide rows, two sources
  (2, 32, 32, 192, 0, 160, 1, 0),      # 128-row tiles, three chunks
])
def test_conv3x3(cuda, B, H, W, C1, C2, Cout, stride, ups):
  from gill_amd import ops
  x1 = _bf(_rnd((B, H, W, C1), 20))
  x2 = _bf(_rnd((B, H, W, C2), 21)) if C2 else None
  w = _rnd((Cout, C1 + C2, 3, 3), 22, 0.05)
  bias, rowvec = _rnd((Cout,), 23), _rnd((B, Cout), 24)
  ref0 = _conv_ref(x1, x2, w, bias, rowvec, None, stride, ups)
  resid = _bf(_rnd(tuple(ref0.shape), 25))
  ref = ref0 + resid.float()
  for sk in (1, 3):
    out = ops.conv3x3(x1.to(cuda), w.to(cuda), bias.to(cuda), x2=None if x2 is None else x2.to(cuda),
                      rowvec=rowvec.to(cuda), resid=resid.to(cuda), stride=stride, upsample=bool(ups), splitk=sk)
    assert tuple(out.shape) == tuple(ref.shape)
    assert _report(f"conv B{B} {H}x{W} {C1}+{C2}->{Cout} s{stride} u{ups} sk{sk}", out, ref) < 1.5e-2


@pytest.mark.parametrize("B,H,W,C1,C2,Cout", [
  (2, 8, 8, 128, 0, 128),        # 128 source rows per class: the four-wave 128 x 128 tile
  (2, 8, 8, 128, 0, 320),        # ... 128 x 160
  (1, 6, 10, 64, 64, 160),       # non-square, two sources, ragged last tile (60 source rows)
  (4, 16, 16, 64, 0, 160),       # 1024 source rows: 128-row ping-pong tiles
  (16, 32, 32, 64, 0, 320),      # 256-row ping-pong tiles (the level-1 -> level-0 upsampler's grid)
  (16, 8, 8, 640, 0, 640),       # long K, short rows (level 3 -> 2 geometry at half width)
])
def test_conv3x3_upsample_four_tap_form(cuda, B, H, W, C1, C2, Cout):
  """conv3x3(nearest_2x(x)) as the engines run it: four 2x2-tap convolutions of the source grid with pre-summed weights (gemm.hip
  "UPS4"; Upsample2D of the UNet / VAE decoder).  Checked against interpolate + conv2d, and — same rounding of the inputs, a
  different but equally exact association of the taps — against the 9-tap gather kernel."""
  from gill_amd import ops
  x1 = _bf(_rnd((B, H, W, C1), 50))
  x2 = _bf(_rnd((B, H, W, C2), 51)) if C2 else None
  w = _rnd((Cout, C1 + C2, 3, 3), 52, 0.05)
  bias = _rnd((Cout,), 53)
  ref = _conv_ref(x1, x2, w, bias, None, None, 1, 1)
  for sk in (1, 2):
    out = ops.conv3x3(x1.to(cuda), w.to(cuda), bias.to(cuda), x2=None if x2 is None else x2.to(cuda), upsample=True, splitk=sk)
    assert tuple(out.shape) == (B, 2 * H, 2 * W, Cout)
    assert _report(f"ups4 conv B{B} {H}x{W} {C1}+{C2}->{Cout} sk{sk}", out, ref) < 1.5e-2
  # with a residual the op falls back to the 9-tap gather: both forms must agree to bf16 rounding
  zero = torch.zeros((B, 2 * H, 2 * W, Cout), dtype=torch.bfloat16)
  nine = ops.conv3x3(x1.to(cuda), w.to(cuda), bias.to(cuda), x2=None if x2 is None else x2.to(cuda), resid=zero.to(cuda), upsample=True, splitk=1)
  assert _report("ups4 vs 9-tap gather", out, nine.float().cpu()) < 1e-2


@pytest.mark.parametrize("B,H,W,C1,C2,CS1,CS2,Cout", [
  (2, 32, 32, 128, 0, 192, 64, 160),     # 128-row ping-pong tiles; shortcut over two sources (an up block's conv2)
  (8, 64, 64, 64, 0, 128, 0, 320),       # 256-row ping-pong tiles
  (16, 32, 32, 128, 0, 64, 0, 640),
  (2, 16, 16, 128, 0, 64, 0, 128),       # not a ping-pong shape: the 128-row kernel's shortcut segment
])
def test_conv3x3_fused_shortcut(cuda, B, H, W, C1, C2, CS1, CS2, Cout):
  """ResnetBlock2D conv2 + conv_shortcut as one implicit GEMM (K = 9 Cin taps, then the raw input's channels at the centre pixel)."""
  from gill_amd import ops
  x1 = _bf(_rnd((B, H, W, C1), 40))
  x2 = _bf(_rnd((B, H, W, C2), 41)) if C2 else None
  xs1 = _bf(_rnd((B, H, W, CS1), 42))
  xs2 = _bf(_rnd((B, H, W, CS2), 43)) if CS2 else None
  w = _rnd((Cout, C1 + C2, 3, 3), 44, 0.05)
  wsc = _rnd((Cout, CS1 + CS2), 45, 0.05)
  bias = _rnd((Cout,), 46)
  xs = xs1.float() if xs2 is None else torch.cat([xs1.float(), xs2.float()], -1)
  ref = _conv_ref(x1, x2, w, bias, None, None, 1, 0) + xs @ wsc.bfloat16().float().T
  for sk in (1, 2):
    out = ops.conv3x3_shortcut(x1.to(cuda), w.to(cuda), xs1.to(cuda), wsc.to(cuda), bias.to(cuda), x2=None if x2 is None else x2.to(cuda),
                               xs2=None if xs2 is None else xs2.to(cuda), splitk=sk)
    assert _report(f"conv+shortcut B{B} {H}x{W} {C1}+{C2} (+{CS1}+{CS2}) -> {Cout} sk{sk}", out, ref) < 1.5e-2


def test_conv3x3_pingpong_short_k_and_bit_identity(cuda):
  """The ping-pong kernel with ONE K step per split (prologue / drain paths of its phase schedule), and its claim of bit-identical
  outputs against the two-workgroups-per-CU kernel (same per-element summation order): the same seeded conv in two subprocesses,
  GILL_GEMM_PP=0 and =1 (the switch is read once per process), must print the same digest."""
  import os, subprocess, sys
  from gill_amd import ops
  x = _bf(_rnd((1, 16, 16, 64), 30)); w = _rnd((320, 64, 3, 3), 31, 0.05)
  ref = _conv_ref(x, None, w, None, None, None, 1, 0)
  out = ops.conv3x3(x.to(cuda), w.to(cuda), splitk=9)
  assert _report("conv 16x16 64->320 sk9 (1 K step per split)", out, ref) < 1.5e-2
  code = ("import hashlib, torch, sys; sys.path.insert(0, %r); from gill_amd import ops, synth\n"
          "x = synth.normal('pp_x', (2, 32, 32, 320), 1).bfloat16().cuda(); w = synth.normal('pp_w', (640, 320, 3, 3), 2, std=0.05).cuda()\n"
          "b = synth.normal('pp_b', (640,), 3).cuda()\n"
          "h = hashlib.sha256()\n"
          "for sk in (1, 2, 5):\n"
          "  h.update(ops.conv3x3(x, w, b, splitk=sk).cpu().view(torch.int16).numpy().tobytes())\n"
          "print('DIGEST', h.hexdigest())\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  digests = []
  for pp in ("0", "1"):
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GILL_GEMM_PP=pp), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    digests.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST")][0])
  assert digests[0] == digests[1], digests


def test_upsample_conv_switch_both_forms_in_the_unet(cuda):
  """GILL_CONV_UPS4 (read once per process): a tiny UNet forward with the upsamplers in the four-tap form and with the 9-tap gather, in two
  subprocesses on the same seeded weights — the two must agree to bf16 rounding of the summed weights (and both have their oracle tests)."""
  import os, subprocess, sys
  code = ("import torch, sys; sys.path.insert(0, %r); from gill_amd import synth; from gill_amd.sd import GillSDPipeline\n"
          "cfg = synth.UNetConfig.tiny(16)\n"
          "sd = {k: v.bfloat16() for k, v in synth.unet_state_dict(cfg, seed=91).items()}\n"
          "pipe = GillSDPipeline(sd, cfg, synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=91), 'cuda:0', max_batch=2)\n"
          "x = synth.normal('u4_x', (2, 4, 16, 16), 92); ctx = synth.normal('u4_c', (2, cfg.ctx_len, cfg.cross_attention_dim), 93)\n"
          "y = pipe.unet(x, torch.tensor([801.0, 21.0]), ctx).float().cpu()\n"
          "torch.save(y, sys.argv[1])\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  import tempfile
  outs = []
  with tempfile.TemporaryDirectory() as d:
    for sw in ("0", "1"):
      f = os.path.join(d, f"y{sw}.pt")
      r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, GILL_CONV_UPS4=sw), capture_output=True, text=True, timeout=600)
      assert r.returncode == 0, r.stderr[-2000:]
      outs.append(torch.load(f))
  assert torch.isfinite(outs[0]).all() and not torch.equal(outs[0], outs[1])       # (the switch did switch: different roundings)
  assert _report("tiny UNet forward: 9-tap gather vs four-tap upsamplers", outs[1], outs[0]) < 2e-2


# ---------------------------------------------------------------- attention
def _attn_ref(q, k, v, H, scale, causal):
  B, nq, hd = q.shape
  nkv = k.shape[1]
  d = hd // H
  qh = q.float().view(B, nq, H, d).transpose(1, 2)
  kh = k.float().view(B, nkv, H, d).transpose(1, 2)
  vh = v.float().view(B, nkv, H, d).transpose(1, 2)
  s = (qh @ kh.transpose(-1, -2)) * scale
  if causal:
    mask = torch.ones(nq, nkv, dtype=torch.bool).tril(diagonal=nkv - nq)
    s = s.masked_fill(~mask, float("-inf"))
  p = s.softmax(-1)
  return (p @ vh).transpose(1, 2).reshape(B, nq, hd)


@pytest.mark.parametrize("B,H,nq,nkv,d,causal", [
  (2, 8, 256, 256, 40, False),    # UNet level-0 shape class (d=40 -> padded 48): the LDS-DMA kernel, 128-query workgroups
  (1, 8, 1024, 1024, 40, False),
  (2, 8, 4096, 4096, 40, False),  # the UNet's level-0 self-attention itself: LDS-DMA kernel, 256-query workgroups, 64 key tiles
  (2, 8, 256, 100, 40, False),    # LDS-DMA kernel with a ragged last key tile (100 keys in a 128-key allocation)
  (3, 8, 384, 192, 40, False),    # ... an odd number of key tiles (the loop is unrolled by two) and of (sample, head) pairs per XCD
  (2, 8, 64, 77, 40, False),      # cross-attention: ragged kv length
  (2, 8, 256, 77, 80, False),
  (1, 8, 64, 64, 160, False),
  (2, 4, 77, 8, 128, False),      # mapper decoder cross-attention
  (2, 4, 77, 77, 128, False),
  (2, 32, 37, 37, 128, True),     # OPT-6.7b causal, ragged length
  (2, 12, 40, 40, 64, True),      # OPT-125m causal
  (1, 2, 200, 200, 64, True),
])
def test_attention(cuda, B, H, nq, nkv, d, causal):
  from gill_amd import ops
  q, k, v = (_bf(_rnd((B, n, H * d), s)) for n, s in ((nq, 30), (nkv, 31), (nkv, 32)))
  scale = d ** -0.5
  ref = _attn_ref(q, k, v, H, scale, causal)
  out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H, scale, causal)
  assert _report(f"attn B{B} H{H} {nq}x{nkv} d{d} causal{int(causal)}", out, ref) < 2e-2


def test_attention_softmax_spike(cuda):
  """Force a large running-max jump mid-sequence (online-softmax rescale path)."""
  from gill_amd import ops
  B, H, n, d = 1, 2, 192, 64
  q, k, v = _rnd((B, n, H * d), 33), _rnd((B, n, H * d), 34), _rnd((B, n, H * d), 35)
  k[:, 150] = q[:, 5] * 4.0   # one key aligned with one query -> spike in a late kv tile
  q, k, v = _bf(q), _bf(k), _bf(v)
  ref = _attn_ref(q, k, v, H, d ** -0.5, False)
  out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H)
  assert _report("attn spike", out, ref) < 2e-2


def _decode_shapes():
  from kv_cache_util import DECODE_SHAPES
  return DECODE_SHAPES


@pytest.mark.parametrize("B,H,nq,nkv,d", _decode_shapes())
def test_attention_causal_decode_offset(cuda, B, H, nq, nkv, d):
  """causal=True with nq < nkv, as a KV-cached decode step runs it: nq new rows (1, an 8-token [IMG] block, or a late prefill piece)
  against nkv = past + nq keys, query i attending kv <= i + (nkv - nq).  attention.hip's per-tile bound (kv_end_blk), per-wave bound
  (wave_kv_end), need_mask and qidx = qrow + coff all depend on that offset.  The bar of test_attention, per query row, so that one
  wrong row cannot hide under another row's maximum.  Operands (kv_cache_util.decode_attn_inputs): a peaked softmax in which the
  diagonal key matters, for which tests/test_kv_cache_host.py shows that a hidden newest key, an offset off by one, a visible
  stale key, K/V of the wrong batch row or a shifted V all fail this very check."""
  from gill_amd import ops
  from kv_cache_util import ATTN_BAR, decode_attn_inputs, report_rows
  q, k, v = decode_attn_inputs(B, H, nq, nkv, d, seed=40)
  scale = d ** -0.5
  ref = _attn_ref(q, k, v, H, scale, True)
  out = ops.attention(_bf(q).to(cuda), _bf(k).to(cuda), _bf(v).to(cuda), H, scale, True)
  assert torch.isfinite(out.float()).all()
  assert report_rows(f"attn decode B{B} H{H} {nq}x{nkv} d{d}", out, ref) < ATTN_BAR
  assert _report(f"attn decode B{B} H{H} {nq}x{nkv} d{d} (whole tensor)", out, ref) < 2e-2


@pytest.mark.parametrize("H,nq,nkv,d", [(32, 1, 129, 128), (12, 8, 71, 64), (12, 8, 136, 64)])
def test_attention_causal_decode_spike_on_newest_key(cuda, H, nq, nkv, d):
  """In the style of test_attention_softmax_spike: the key the step has just appended (index nkv - 1) is aligned with the last query, so
  it dominates that row's softmax -- from the last key tile, after the running max has settled on earlier tiles.  A step that did
  not see its newest key would return a different row altogether."""
  from gill_amd import ops
  from kv_cache_util import ATTN_BAR, report_rows
  B = 2
  q, k, v = _rnd((B, nq, H * d), 61), _rnd((B, nkv, H * d), 62), _rnd((B, nkv, H * d), 63)
  k[:, nkv - 1] = q[:, nq - 1] * 4.0
  q, k, v = _bf(q), _bf(k), _bf(v)
  ref = _attn_ref(q, k, v, H, d ** -0.5, True)
  blind = _attn_ref(q[:, -1:], k[:, :-1], v[:, :-1], H, d ** -0.5, False)
  assert _report("newest key matters to the last row (oracle with vs without it)", blind, ref[:, -1:]) > 10 * ATTN_BAR
  out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H, d ** -0.5, True)
  assert report_rows(f"attn decode spike on the newest key H{H} {nq}x{nkv} d{d}", out, ref) < ATTN_BAR


@pytest.mark.parametrize("H,nq,nkv,d,row", [(32, 8, 72, 128, 3), (12, 8, 65, 64, 0), (12, 33, 97, 64, 30), (12, 130, 300, 64, 127)])
def test_attention_causal_decode_first_masked_key_has_no_effect(cuda, H, nq, nkv, d, row):
  """The first masked key of query `row` (index qidx + 1, present in K: the next token of the same step) is aligned with that query:
  seen, it would dominate the row.  It must have exactly no effect on rows 0 .. row: they are bit-identical to a run in which that
  key's K and V rows hold other finite values (the later rows, which do see the key, must differ), and they meet the oracle.
  (The 33 x 97 case caught attention.hip moving the running max of every row of a wave as soon as one row asked for it: rows 0 .. 30
  share their wave with row 31, which sees the key, so their rounding followed a key they have masked.)"""
  from gill_amd import ops
  from kv_cache_util import ATTN_BAR, report_rows
  B = 2
  q, k, v = _rnd((B, nq, H * d), 64), _rnd((B, nkv, H * d), 65), _rnd((B, nkv, H * d), 66)
  masked = row + (nkv - nq) + 1
  k[:, masked] = q[:, row] * 4.0
  q, k, v = _bf(q), _bf(k), _bf(v)
  k2, v2 = k.clone(), v.clone()
  k2[:, masked], v2[:, masked] = _bf(_rnd((B, H * d), 67) * 3.0), _bf(_rnd((B, H * d), 68) * 50.0)
  ref = _attn_ref(q, k, v, H, d ** -0.5, True)
  seen = _attn_ref(q[:, row:row + 1], k[:, :masked + 1], v[:, :masked + 1], H, d ** -0.5, False)
  assert _report("the masked key would matter (oracle, seen vs masked)", seen, ref[:, row:row + 1]) > 10 * ATTN_BAR
  out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H, d ** -0.5, True)
  out2 = ops.attention(q.to(cuda), k2.to(cuda), v2.to(cuda), H, d ** -0.5, True)
  assert torch.equal(out[:, :row + 1], out2[:, :row + 1])
  assert not torch.equal(out[:, row + 1:], out2[:, row + 1:])
  assert report_rows(f"attn decode, first masked key aligned H{H} {nq}x{nkv} d{d}", out, ref) < ATTN_BAR


@pytest.mark.parametrize("mag", [1.0, 64.0, 4096.0])
def test_attention_d40_large_scores(cuda, mag):
  """d = 40 (the QF3 / LDS-DMA kernel): scores far outside bf16's integer range, and a running max that jumps in a late tile.
  The offset rides in three bf16 padding dims as an exact split of the fp32 running max, so magnitude must not matter
  (the one-dim bf16 offset of round 3's kernel lost the low bits at |score| >= 2^15).  The reference uses the operands the
  kernel sees — Q pre-multiplied by scale * log2(e) and rounded to bf16 by the QKV producer (GemmArgs::qscale) — because at these
  magnitudes that rounding alone moves scores by whole units and decides near-ties of an almost one-hot softmax."""
  from gill_amd import ops
  B, H, n, d = 1, 8, 256, 40
  q, k, v = _rnd((B, n, H * d), 36), _rnd((B, n, H * d), 37), _rnd((B, n, H * d), 38)
  k[:, 200] = q[:, 7] * 3.0      # spike in the last 64-key tile
  q = q * mag
  q, k, v = _bf(q), _bf(k), _bf(v)
  scale = d ** -0.5
  q2 = _bf(q.float() * (scale * 1.4426950408889634))          # what pack_heads / the QKV epilogue hand the kernel
  ref = _attn_ref(q2, k, v, H, 0.6931471805599453, False)      # softmax(ln 2 * s2) = exp2-softmax of s2 = q2 . k
  out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H)
  assert torch.isfinite(out.float()).all()
  assert _report(f"attn d40 mag {mag}", out, ref) < 2e-2


def test_attention_dma_matches_register_staged(cuda):
  """The LDS-DMA kernel against the register-staged kernel on the same operands (GILL_ATT_DMA=0 in a child process)."""
  import subprocess, sys, os, tempfile
  from gill_amd import ops
  B, H, n, d = 2, 8, 512, 40
  q, k, v = (_bf(_rnd((B, n, H * d), s)) for s in (51, 52, 53))
  out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), H).float().cpu()
  with tempfile.TemporaryDirectory() as td:
    torch.save((q, k, v), os.path.join(td, "in.pt"))
    code = ("import torch, sys; sys.path.insert(0, %r); from gill_amd import ops; q, k, v = torch.load(%r); "
            "o = ops.attention(q.cuda(), k.cuda(), v.cuda(), %d).float().cpu(); torch.save(o, %r)"
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(td, "in.pt"), H, os.path.join(td, "out.pt")))
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, GILL_ATT_DMA="0"))
    old = torch.load(os.path.join(td, "out.pt"))
  assert _report("attn dma vs register-staged", out, old) < 1e-2


@pytest.mark.parametrize("B,H,W,Cin,Cout,splitk,silu,resid,raw", [
  (2, 16, 16, 1280, 1280, 2, True, False, False),    # UNet level 2: conv1 -> norm2 (raw tensor not written)
  (3, 8, 8, 1280, 1280, 8, True, False, False),      # level 3
  (2, 16, 16, 1280, 1280, 2, False, True, True),     # conv2 + residual -> the transformer block's GroupNorm (no SiLU, eps 1e-6)
  (2, 8, 8, 640, 640, 4, True, True, True),          # groups of 20 channels (Cout 640): 4 groups per 80-column block
  (8, 8, 8, 1280, 1280, 8, True, False, False),      # level 3 at the CFG batch 8: 4 x 8 tiles x 8 splits = 256 workgroups, two samples per 128-row tile
  (8, 16, 16, 1280, 1280, 2, False, True, True),     # level 2 at the CFG batch 8: 16 x 8 x 2 = 256 workgroups, two M tiles per sample
  (4, 8, 8, 640, 640, 4, True, True, True),          # groups of 20 channels, four samples
  (8, 16, 16, 640, 1280, 3, True, False, True),      # an odd split factor
])
def test_conv3x3_split_k_reducer_with_fused_groupnorm(cuda, B, H, W, Cin, Cout, splitk, silu, resid, raw):
  """gemm_reduce.hip "REDUCE + GROUPNORM": the split-K reducer of a 3x3 convolution also runs the GroupNorm (+ SiLU) that consumes the
  output (diffusers ResnetBlock2D conv1 -> norm2 -> silu; conv2 -> next block's norm), against F.conv2d + F.group_norm in fp32.
  The operator's coop flag concerns splitk == 1 only: on the smallest row it is set once and must change nothing."""
  from gill_amd import ops
  x = _bf(_rnd((B, H, W, Cin), 90))
  w = _rnd((Cout, Cin, 3, 3), 91, (9 * Cin) ** -0.5)
  b = 0.1 * _rnd((Cout,), 92)
  r = _bf(_rnd((B, H, W, Cout), 93)) if resid else None
  gamma, beta = 1.0 + 0.2 * _rnd((Cout,), 94), 0.1 * _rnd((Cout,), 95)
  eps = 1e-5 if silu else 1e-6
  ref_raw = F.conv2d(x.float().permute(0, 3, 1, 2), _bf(w).float(), b, padding=1)
  if resid:
    ref_raw = ref_raw + r.float().permute(0, 3, 1, 2)
  ref = F.group_norm(_bf(ref_raw).float(), 32, gamma, beta, eps)
  if silu:
    ref = F.silu(ref)
  args = (x.to(cuda), w.to(cuda), b.to(cuda), gamma.to(cuda), beta.to(cuda), 32, eps, silu, None if r is None else r.to(cuda), splitk, raw)
  y_raw, y_norm = ops.conv3x3_gn(*args, coop=False)
  assert torch.isfinite(y_norm.float()).all()
  assert _report(f"conv+GN B{B} {H}x{W} {Cin}->{Cout} sk{splitk}", y_norm.permute(0, 3, 1, 2), ref) < 1.5e-2
  if raw:
    assert _report("  raw", y_raw.permute(0, 3, 1, 2), ref_raw) < 1.5e-2
  if (B, H, W, Cout) == (2, 8, 8, 640):      # coop is ignored for splitk >= 2: the same reducer launch, the same bits, no waiting workgroup
    from gill_amd import _native as N
    c_raw, c_norm = ops.conv3x3_gn(*args, coop=True)
    assert torch.equal(c_norm, y_norm) and torch.equal(c_raw, y_raw)
    assert N.lib().gill_coop_timeouts() == 0


@pytest.mark.parametrize("B,H,W,Cin,Cout,silu,resid,raw,rowvec,table", [
  (8, 64, 64, 320, 320, True, False, False, True, False),     # UNet level 0 at the CFG batch 8: conv1 + time-embedding row -> norm2 (256 workgroups of 256 x 160)
  (4, 64, 64, 320, 320, False, True, True, False, True),      # the shared CFG prefix (4 samples, 128-row tiles): conv2 + residual -> the transformer's GroupNorm, + table
  (8, 32, 32, 640, 640, True, False, False, True, False),     # level 1: 128-row tiles, 8 workgroups per (sample, N tile), groups of 20 channels
  (8, 32, 32, 320, 640, False, True, True, False, False),     # level 1, conv2 form with the raw tensor kept
  (2, 32, 32, 640, 320, True, False, True, True, True),       # few samples: 16 + 16 workgroups on a 256-CU chip
  (1, 16, 16, 320, 320, True, False, False, False, False),    # one sample of 256 rows: two 128-row tiles per (sample, N tile), four workgroups in all
])
def test_conv3x3_groupnorm_finished_in_the_epilogue(cuda, B, H, W, Cin, Cout, silu, resid, raw, rowvec, table):
  """gemm.hip "COOP" (EPI 6, round 6): the GroupNorm (+ SiLU) that consumes a non-split 3x3 convolution, finished by the convolution's own
  workgroups — each publishes its per-slab partial sums, waits for the other M tiles of its (sample, N tile) on an arrival counter, totals the
  partials in the GroupNorm-apply kernel's order and normalises straight from its accumulators.  Against F.conv2d + F.group_norm in fp32, and
  against the reference dataflow (conv with fused statistics + groupnorm_apply_launch, coop=False): IDENTICAL bits — same statistics, same
  summation order, same rounding of the values normalised.  table: the scale | shift form lnproj.hip consumes (y = raw * scale + shift)."""
  from gill_amd import ops
  x = _bf(_rnd((B, H, W, Cin), 290))
  w = _rnd((Cout, Cin, 3, 3), 291, (9 * Cin) ** -0.5)
  b = 0.1 * _rnd((Cout,), 292)
  r = _bf(_rnd((B, H, W, Cout), 293)) if resid else None
  rv = 0.3 * _rnd((B, Cout), 296) if rowvec else None
  gamma, beta = 1.0 + 0.2 * _rnd((Cout,), 294), 0.1 * _rnd((Cout,), 295)
  eps = 1e-5 if silu else 1e-6
  ref_raw = F.conv2d(x.float().permute(0, 3, 1, 2), _bf(w).float(), b, padding=1)
  if rowvec:
    ref_raw = ref_raw + rv.view(B, Cout, 1, 1)
  if resid:
    ref_raw = ref_raw + r.float().permute(0, 3, 1, 2)
  ref = F.group_norm(_bf(ref_raw).float(), 32, gamma, beta, eps)
  if silu:
    ref = F.silu(ref)
  dev = lambda t: None if t is None else t.to(cuda)   # noqa: E731
  res = ops.conv3x3_gn(dev(x), dev(w), dev(b), dev(gamma), dev(beta), 32, eps, silu, dev(r), 1, raw, coop=True, rowvec=dev(rv), want_table=table)
  y_raw, y_norm = res[0], res[1]
  assert torch.isfinite(y_norm.float()).all()
  assert _report(f"conv+GN in the epilogue B{B} {H}x{W} {Cin}->{Cout}", y_norm.permute(0, 3, 1, 2), ref) < 1.5e-2
  if raw:
    assert _report("  raw", y_raw.permute(0, 3, 1, 2), ref_raw) < 1.5e-2
  base_raw, base_norm = ops.conv3x3_gn(dev(x), dev(w), dev(b), dev(gamma), dev(beta), 32, eps, silu, dev(r), 1, True, coop=False, rowvec=dev(rv))
  assert torch.equal(y_norm, base_norm), f"in-epilogue GroupNorm differs from conv + GroupNorm-apply: {(y_norm.float() - base_norm.float()).abs().max().item():.3e}"
  if raw:
    assert torch.equal(y_raw, base_raw)
  again = ops.conv3x3_gn(dev(x), dev(w), dev(b), dev(gamma), dev(beta), 32, eps, silu, dev(r), 1, raw, coop=True, rowvec=dev(rv))[1]
  assert torch.equal(y_norm, again)
  from gill_amd import _native as N
  assert N.lib().gill_coop_timeouts() == 0      # no bounded wait gave up (include/gill_amd.h "Exclusive-device contract")
  if table:
    t = res[2]
    assert torch.isfinite(t).all()
    from_table = base_raw.float() * t[:, 0].view(B, 1, 1, Cout) + t[:, 1].view(B, 1, 1, Cout)
    if silu:
      from_table = F.silu(from_table)
    assert _report("  raw * scale + shift (table)", from_table.permute(0, 3, 1, 2), ref) < 1.5e-2


# ---------------------------------------------------------------- norms
@pytest.mark.parametrize("rows,C,f32", [(37, 512, True), (64, 4096, True), (300, 320, False), (16, 1280, False),
                                        (5, 768, True)])
def test_layernorm(cuda, rows, C, f32):
  from gill_amd import ops
  x = _rnd((rows, C), 40) * 3 + 1.5
  if not f32:
    x = _bf(x)
  g, b = _rnd((C,), 41), _rnd((C,), 42)
  ref = F.layer_norm(x.float(), (C,), g, b, 1e-5)
  out = ops.layernorm(x.to(cuda), g.to(cuda), b.to(cuda), 1e-5)
  assert _report(f"layernorm {rows}x{C}", out, ref) < 1e-2


@pytest.mark.parametrize("B,H,W,C1,C2,silu", [(2, 16, 16, 320, 0, True), (2, 8, 8, 1280, 640, True),
                                               (1, 32, 32, 320, 0, False), (3, 8, 8, 640, 320, True),
                                               (2, 64, 64, 320, 0, True),
                                               # maps that are not whole 32-pixel slabs of the statistics pass (the tiny configs' sizes)
                                               (2, 2, 2, 320, 0, True), (1, 4, 4, 640, 320, True), (2, 10, 10, 128, 0, False)])
def test_groupnorm(cuda, B, H, W, C1, C2, silu):
  from gill_amd import ops
  x1 = _bf(_rnd((B, H, W, C1), 50) * 2 + 3.0)   # large mean: exercises the shifted-variance path
  x2 = _bf(_rnd((B, H, W, C2), 51)) if C2 else None
  C = C1 + C2
  g, b = _rnd((C,), 52), _rnd((C,), 53)
  x = x1.float() if x2 is None else torch.cat([x1.float(), x2.float()], -1)
  ref = F.group_norm(x.permute(0, 3, 1, 2), 32, g, b, 1e-5)
  if silu:
    ref = F.silu(ref)
  ref = ref.permute(0, 2, 3, 1)
  out = ops.groupnorm(x1.to(cuda), g.to(cuda), b.to(cuda), 32, 1e-5, silu, None if x2 is None else x2.to(cuda))
  assert _report(f"groupnorm B{B} {H}x{W} {C1}+{C2}", out, ref) < 1.5e-2


from gill_amd import synth   # noqa: E402


# ---------------------------------------------------------------- fused feed-forward block (csrc/ffn.hip)
@pytest.mark.parametrize("M,rows_per_batch", [(128, 128), (512, 256), (4096, 1024)])
def test_ffn_fused_vs_torch(cuda, M, rows_per_batch):
  """BasicTransformerBlock.ff (norm3 -> GEGLU -> Linear) + residual, then proj_out + the outer residual — at C = 320 one kernel: against
  the fp32 restatement on the same bf16-rounded operands, and its GroupNorm partial sums (64-row slabs, bins of 5 channels) against sums
  of the tensor it wrote.  Ref: diffusers BasicTransformerBlock / Transformer2DModel as restated in oracle/unet_ref.py:_transformer."""
  from gill_amd import ops
  C, H = 320, 1280
  t = _bf(_rnd((M, C), 60, 1.5) + 0.3)
  resid = _bf(_rnd((M, C), 61))
  ln_g, ln_b = 1.0 + 0.2 * _rnd((C,), 62), 0.1 * _rnd((C,), 63)
  w1, b1 = _bf(_rnd((2 * H, C), 64, 0.06)), 0.1 * _rnd((2 * H,), 65)
  w2, b2 = _bf(_rnd((C, H), 66, 0.03)), 0.1 * _rnd((C,), 67)
  wp, bp = _bf(_rnd((C, C), 68, 0.05)), 0.1 * _rnd((C,), 69)
  x = F.layer_norm(t.float(), (C,), ln_g, ln_b, 1e-5)
  pr = x @ w1.float().T + b1
  h = pr[:, :H] * F.gelu(pr[:, H:])
  y = t.float() + h @ w2.float().T + b2
  ref = y @ wp.float().T + bp + resid.float()
  out, stats = ops.ffn_fused(t.to(cuda), ln_g.to(cuda), ln_b.to(cuda), w1.to(cuda), b1.to(cuda), w2.to(cuda), b2.to(cuda), wp.to(cuda),
                             bp.to(cuda), resid.to(cuda), rows_per_batch=rows_per_batch)
  assert torch.isfinite(out.float()).all() and torch.isfinite(stats).all()      # (NaN-prefilled by the wrapper: every tile was written)
  assert _report(f"fused FFN M={M}", out, ref) < 1e-2
  o = out.float().cpu().view(M // 64, 64, 64, 5)                  # (slab, row, bin, channel in bin)
  want = torch.stack([o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], dim=-1)
  got = stats.cpu()
  assert torch.allclose(got, want, rtol=2e-4, atol=2e-3), float((got - want).abs().max())



@pytest.mark.parametrize("M", [128, 1024])
def test_ffn_fused_with_attn2_to_out_in_front_vs_torch(cuda, M):
  """The form the UNet engine runs: attn2.to_out + its residual inside the same kernel (t = t_prev + to_out(o2), never stored), then the
  feed-forward block as above — against the fp32 restatement on the same bf16-rounded operands (t rounded to bf16 where the separate
  GEMM would have stored it)."""
  from gill_amd import ops
  C, H = 320, 1280
  t_prev = _bf(_rnd((M, C), 160, 1.5) + 0.3)
  o2 = _bf(_rnd((M, C), 161))
  wo, bo2 = _bf(_rnd((C, C), 162, 0.06)), 0.2 * _rnd((C,), 163)
  resid = _bf(_rnd((M, C), 164))
  ln_g, ln_b = 1.0 + 0.2 * _rnd((C,), 165), 0.1 * _rnd((C,), 166)
  w1, b1 = _bf(_rnd((2 * H, C), 167, 0.06)), 0.1 * _rnd((2 * H,), 168)
  w2, b2 = _bf(_rnd((C, H), 169, 0.03)), 0.1 * _rnd((C,), 170)
  wp, bp = _bf(_rnd((C, C), 171, 0.05)), 0.1 * _rnd((C,), 172)
  t = _bf(t_prev.float() + o2.float() @ wo.float().T + bo2).float()
  pr = F.layer_norm(t, (C,), ln_g, ln_b, 1e-5) @ w1.float().T + b1
  y = t + (pr[:, :H] * F.gelu(pr[:, H:])) @ w2.float().T + b2
  ref = y @ wp.float().T + bp + resid.float()
  out, stats = ops.ffn_fused(t_prev.to(cuda), ln_g.to(cuda), ln_b.to(cuda), w1.to(cuda), b1.to(cuda), w2.to(cuda), b2.to(cuda), wp.to(cuda),
                             bp.to(cuda), resid.to(cuda), rows_per_batch=128, o2=o2.to(cuda), wo=wo.to(cuda), bo2=bo2.to(cuda))
  assert _report(f"fused FFN with attn2.to_out M={M}", out, ref) < 1e-2
  o = out.float().cpu().view(M // 64, 64, 64, 5)
  want = torch.stack([o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], dim=-1)
  assert torch.allclose(stats.cpu(), want, rtol=2e-4, atol=2e-3)

# ---------------------------------------------------------------- fused projection pairs around norm1 / norm2 (csrc/lnproj.hip)
@pytest.mark.parametrize("B,HW", [(1, 128), (2, 192), (2, 1024)])
def test_lnproj_proj_in_qkv_vs_torch(cuda, B, HW):
  """Transformer2DModel.proj_in -> norm1 -> attn1.to_q / to_k / to_v at C = 320 (8 heads of 40) as one kernel: the residual stream and the
  head-major q / k / v^T it scatters (padded head dim 48, q pre-scaled, spare V^T row = 1) against the fp32 restatement on the same
  bf16-rounded operands.  Ref: diffusers Transformer2DModel / BasicTransformerBlock as restated in oracle/unet_ref.py:_transformer."""
  from gill_amd import ops
  C, nh, d, M = 320, 8, 40, B * HW
  hw_pad = (HW + 31) // 32 * 32
  x = _bf(_rnd((M, C), 70))
  w1, b1 = _bf(_rnd((C, C), 71, 0.08)), 0.2 * _rnd((C,), 72)
  ln_g, ln_b = 1.0 + 0.2 * _rnd((C,), 73), 0.1 * _rnd((C,), 74)
  w2 = _bf(_rnd((3 * C, C), 75, 0.06))
  t_ref = x.float() @ w1.float().T + b1
  tb = _bf(t_ref).float()                       # (the kernel normalises the ROUNDED residual stream, as every other consumer reads it)
  qkv = F.layer_norm(tb, (C,), ln_g, ln_b, 1e-5) @ w2.float().T
  t, q, k, vt = ops.lnproj(0, x.to(cuda), None, w1.to(cuda), b1.to(cuda), ln_g.to(cuda), ln_b.to(cuda), w2.to(cuda), B, HW)
  assert _report(f"lnproj mode 0 t B={B} HW={HW}", t, t_ref) < 6e-3
  heads = lambda v: v.view(B, HW, nh, d).permute(0, 2, 1, 3)                      # (B, h, tok, d)
  qs = 1.4426950408889634 / d ** 0.5
  assert _report("lnproj q", q[:, :, :HW, :d], heads(qkv[:, :C]) * qs) < 1e-2
  assert _report("lnproj k", k[:, :, :HW, :d], heads(qkv[:, C:2 * C])) < 1e-2
  assert _report("lnproj v^T", vt[:, :, :d, :HW], heads(qkv[:, 2 * C:]).transpose(2, 3)) < 1e-2
  assert float(q[:, :, :HW, d:].float().abs().max()) == 0 and float(k[:, :, :HW, d:].float().abs().max()) == 0
  assert torch.all(vt[:, :, 48, :HW].float() == 1.0)
  # (the wrapper pre-fills every output with NaN: all of t, all 48 columns of q / k and rows 0 .. 48 of V^T were written; rows 49 .. 63
  # of V^T only feed output rows of the attention kernel that are never stored, and the kernel does not write them)
  assert torch.isfinite(t.float()).all() and torch.isfinite(q[:, :, :HW].float()).all() and torch.isfinite(k[:, :, :HW].float()).all()
  assert torch.isfinite(vt[:, :, :49, :HW].float()).all()
  assert float(vt[:, :, d:48, :HW].float().abs().max()) == 0


# ---------------------------------------------------------------- cross-attention as two GEMMs on per-sample weights (csrc/xf_weights.hip "XALG")
@pytest.mark.parametrize("B,HW,C,nh,ctx_len", [(2, 64, 1280, 8, 77), (3, 256, 1280, 8, 77), (2, 1024, 640, 8, 77), (2, 128, 640, 4, 80), (1, 64, 640, 8, 5),
                                                 (8, 1024, 640, 8, 77)])     # (last: level 1 at the CFG batch 8 — both GEMMs on 256 ping-pong workgroups, per-sample weights)
def test_cross_attention_folded_vs_torch(cuda, B, HW, C, nh, ctx_len):
  """norm2 -> attn2 (to_q, to_k / to_v of the prompt context, softmax, to_out) -> residual of a BasicTransformerBlock, computed by the two
  GEMMs the engine runs at UNet levels 1-3 — P = softmax80(LN(t) Mq_b^T) and out = t + P Wo_b^T + bo on weights folded per sample from
  (to_q, to_k, ctx) and (to_out, to_v, ctx) — against the fp32 attention on the same bf16-rounded operands.  The softmax weights themselves
  are checked too (key slots >= ctx_len must be exactly 0, rows must sum to 1).  Ref: diffusers CrossAttention as restated in
  oracle/unet_ref.py:_attention / _transformer."""
  from gill_amd import ops
  E, d, M = 768, C // nh, B * HW
  t = _bf(_rnd((M, C), 90, 1.5) + 0.3)
  ln_g, ln_b = 1.0 + 0.2 * _rnd((C,), 91), 0.1 * _rnd((C,), 92)
  wq, wk, wv = _bf(_rnd((C, C), 93, 0.05)), _bf(_rnd((C, E), 94, 0.05)), _bf(_rnd((C, E), 95, 0.05))
  wo, bo = _bf(_rnd((C, C), 96, 0.05)), 0.2 * _rnd((C,), 97)
  ctx = _bf(_rnd((B, ctx_len, E), 98))
  q = F.layer_norm(t.float(), (C,), ln_g, ln_b, 1e-5) @ wq.float().T                                       # (M, C)
  k, v = ctx.float() @ wk.float().T, ctx.float() @ wv.float().T                                            # (B, ctx_len, C)
  hq = q.view(B, HW, nh, d).permute(0, 2, 1, 3)
  hk, hv = (x.view(B, ctx_len, nh, d).permute(0, 2, 1, 3) for x in (k, v))
  p_ref = torch.softmax(hq @ hk.transpose(2, 3) / d ** 0.5, dim=-1)                                        # (B, h, HW, ctx_len)
  o_ref = (p_ref @ hv).permute(0, 2, 1, 3).reshape(M, C)
  out_ref = t.float() + o_ref @ wo.float().T + bo
  out, P = ops.cross_attention_folded(t.to(cuda), ln_g.to(cuda), ln_b.to(cuda), wq.to(cuda), wk.to(cuda), wv.to(cuda), wo.to(cuda), bo.to(cuda),
                                      ctx.to(cuda), nh, B, HW)
  assert torch.isfinite(out.float()).all() and torch.isfinite(P.float()).all()        # (NaN-prefilled by the wrapper: all written)
  Pv = P.float().cpu().view(B, HW, nh, 80).permute(0, 2, 1, 3)
  assert float(Pv[..., ctx_len:].abs().max()) == 0 if ctx_len < 80 else True
  assert float((Pv.sum(-1) - 1).abs().max()) < 2e-2                                   # (bf16 weights: 80 roundings of <= 2^-9 relative)
  assert _report(f"xalg softmax weights B={B} HW={HW} C={C}", Pv[..., :ctx_len], p_ref) < 2e-2
  # the attention term alone (what the two GEMMs add to the residual stream), then the sum
  assert _report("xalg attention term", out.float().cpu() - t.float(), out_ref - t.float()) < 2e-2
  assert _report("xalg out", out, out_ref) < 6e-3


@pytest.mark.parametrize("B,HW", [(1, 128), (2, 1024)])
def test_lnproj_to_out_to_q_vs_torch(cuda, B, HW):
  """attn1.to_out + residual -> norm2 -> attn2.to_q as one kernel, against the fp32 restatement on the same bf16-rounded operands."""
  from gill_amd import ops
  C, nh, d, M = 320, 8, 40, B * HW
  o = _bf(_rnd((M, C), 80))
  t0 = _bf(_rnd((M, C), 81, 1.5) + 0.2)
  w1, b1 = _bf(_rnd((C, C), 82, 0.08)), 0.2 * _rnd((C,), 83)
  ln_g, ln_b = 1.0 + 0.2 * _rnd((C,), 84), 0.1 * _rnd((C,), 85)
  w2 = _bf(_rnd((C, C), 86, 0.06))
  t_ref = o.float() @ w1.float().T + b1 + t0.float()
  q_ref = F.layer_norm(_bf(t_ref).float(), (C,), ln_g, ln_b, 1e-5) @ w2.float().T
  t, q, _, _ = ops.lnproj(1, o.to(cuda), t0.to(cuda), w1.to(cuda), b1.to(cuda), ln_g.to(cuda), ln_b.to(cuda), w2.to(cuda), B, HW)
  assert _report(f"lnproj mode 1 t B={B} HW={HW}", t, t_ref) < 6e-3
  qs = 1.4426950408889634 / d ** 0.5
  assert _report("lnproj q2", q[:, :, :HW, :d], q_ref.view(B, HW, nh, d).permute(0, 2, 1, 3) * qs) < 1e-2
  assert torch.isfinite(q[:, :, :HW].float()).all() and float(q[:, :, :HW, d:].float().abs().max()) == 0     # (NaN-prefilled: written, pads zero)
