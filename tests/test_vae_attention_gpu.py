"""The VAE mid block's single-head attention chain (csrc/vae.hip vae_attention_chain through gill_op_vae_attention: the QKV GEMM in the
natural-exponent domain, per image S = Q K^T into bf16, vae_row_softmax_kernel, O = P V, to_out + residual) and its softmax kernel on its own
(gill_op_row_softmax), against the fp64 restatement of tests/vae_attention_util.py.

The bars are twice the measured bf16-storage distance of each (shape, gain) (vae_attention_util.STORAGE, tools/vae_attention_tolerance.py,
profiles/vae_attention.md); tests/test_vae_attention_host.py shows what they catch."""
import pytest
import torch

import vae_attention_util as A

pytestmark = pytest.mark.gpu


def _dev(inp, cuda):
  bf = lambda t: t.to(torch.bfloat16).to(cuda)   # noqa: E731
  return dict(n=bf(inp["n"]), wqkv=bf(torch.cat([inp["wq"], inp["wk"], inp["wv"]])), bqkv=torch.cat([inp["bq"], inp["bk"], inp["bv"]]).float().to(cuda),
              wo=bf(inp["wo"]), bo=inp["bo"].float().to(cuda))


_splits_seen = {}


# (2, 64, 64): the smallest legal geometry; (3, 256, 128): the tiny VAE's own; (2, 576, 512): the SD channel count with HW a multiple of neither 512
# (the softmax's per-wave stride) nor 128 (a ragged N tile of the S GEMM, ldc = 576), PV with 9 K steps; (2, 1024, 512)
@pytest.mark.parametrize("gain", A.GAINS)
@pytest.mark.parametrize("shape", A.SHAPES, ids=str)
def test_chain_matches_the_fp64_restatement(cuda, shape, gain):
  from gill_amd import ops
  key = (*shape, gain)
  inp = A.attn_inputs(*key, A.case_seed(*key))
  exact = A.exact_of(inp)
  d = _dev(inp, cuda)
  resid = inp["resid"].to(torch.bfloat16).to(cuda)
  out, P, splits = ops.vae_attention(**d, want_p=True)
  outr, Pr, splits_r = ops.vae_attention(**d, resid=resid, want_p=True)
  print(f"[vae attention {key}] split-K factors QKV / S / PV: {splits}")
  _splits_seen[shape] = splits
  assert splits == splits_r and all(s >= 1 for s in splits)
  for t in (out, P, outr, Pr):
    assert bool(torch.isfinite(t).all())      # (NaN prefill: everything was written)
  assert torch.equal(P, Pr)
  res = A.check_chain(key, out.cpu(), outr.cpu(), P.cpu(), exact)
  for name, got, bar in res:
    print(f"[vae attention {key}] {name}: {got:.3e} (bar {bar:.3e})")
  for name, got, bar in res:
    assert got <= bar, (key, name, got, bar)
  # the engine's form — one score buffer reused by every image — gives the same bits as the strided one, run after run
  for _ in range(2):
    o1, none, s1 = ops.vae_attention(**d, resid=resid)
    assert none is None and s1 == splits and torch.equal(o1, outr)
  assert torch.equal(ops.vae_attention(**d, resid=resid, want_p=True)[0], outr)


def test_shapes_cover_split_and_unsplit_pv(cuda):
  """The PV GEMM (K = HW) must run both ways over the shape list: gemm_pick_splitk() leaves the tiny VAE's (4 K steps) unsplit and splits C = 512."""
  from gill_amd import ops
  for shape in A.SHAPES:
    if shape not in _splits_seen:
      d = _dev(A.attn_inputs(*shape, 1, A.case_seed(*shape, 1)), cuda)
      _splits_seen[shape] = ops.vae_attention(**d)[2]
  pv = {shape: s[2] for shape, s in _splits_seen.items()}
  print(f"[vae attention] PV split per shape: {pv}")
  assert any(v > 1 for v in pv.values()) and any(v == 1 for v in pv.values()), pv


def test_whole_block_matches_the_oracle(cuda):
  """ops.groupnorm(eps 1e-6) -> the op with resid = x, against oracle/vae_ref._attn on a state dict of the same tensors: pins the op's weight
  layout (to_q | to_k | to_v rows, to_out.0) to the oracle's names.  Bars: twice vae_attention_util.BLOCK_STORAGE."""
  from gill_amd import ops
  from oracle import vae_ref
  B, HW, C, gain = A.BLOCK_CASE
  x, gamma, beta, inp = A.block_inputs(B, HW, C, gain, A.case_seed(*A.BLOCK_CASE))
  side = int(HW ** 0.5)
  sd = {k: v.float() for k, v in A.block_state_dict(gamma, beta, inp).items()}
  want = vae_ref._attn(sd, "a", x.float().reshape(B, side, side, C).permute(0, 3, 1, 2), 32).permute(0, 2, 3, 1).reshape(B, HW, C)
  xd = x.to(torch.bfloat16).to(cuda)
  n = ops.groupnorm(xd.reshape(B, side, side, C), gamma.float().to(cuda), beta.float().to(cuda), groups=32, eps=1e-6)
  out, _, _ = ops.vae_attention(**{**_dev(inp, cuda), "n": n.reshape(B, HW, C)}, resid=xd)
  assert bool(torch.isfinite(out).all())
  s, r = A.distances(out.cpu(), want)
  print(f"[vae attention block] sample {s:.3e} (bar {2 * A.BLOCK_STORAGE[0]:.3e}), row {r:.3e} (bar {2 * A.BLOCK_STORAGE[1]:.3e})")
  assert s <= 2 * A.BLOCK_STORAGE[0] and r <= 2 * A.BLOCK_STORAGE[1], (s, r)


def test_chain_refuses_a_token_count_off_the_tile(cuda):
  from gill_amd import _native as N, ops
  d = _dev(A.attn_inputs(1, 72, 64, 1, 1), cuda)
  with pytest.raises(N.GillNativeError, match="multiples of 64"):
    ops.vae_attention(**d)


@pytest.mark.parametrize("shape", A.SOFTMAX_SHAPES, ids=str)
def test_row_softmax_matches_fp64(cuda, shape):
  """One bf16 ulp against the fp64 softmax of the same bf16 values (vae_attention_util.check_softmax); the rows behind the matrix stay as they were."""
  from gill_amd import ops
  for s in A.softmax_cases(*shape, seed=shape[1]):
    got, guard_after, guard_before = ops.row_softmax(s.to(cuda))
    assert A.check_softmax(got.cpu(), s) == []
    assert torch.equal(guard_after.view(torch.int16), guard_before.view(torch.int16))
  last = got[-1].float()       # the single entry 80 above the rest: exactly one 1 and zeros
  assert last.sum().item() == 1.0 and last.max().item() == 1.0


def test_row_softmax_refuses_a_row_length_off_the_vector(cuda):
  from gill_amd import _native as N, ops
  s = torch.zeros((4, 12), device=cuda, dtype=torch.bfloat16)
  with pytest.raises(N.GillNativeError, match="multiple of 8"):
    ops.row_softmax(s)
