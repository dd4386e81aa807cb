"""gill_opt_forward_cached on a w8 handle (GILL_OPT_W8) through the C ABI on the MI355X: the calls with past_len > 0 and at most
gill_w8_max_rows() rows run their linears on the e4m3 bytes, with self-attention as projection -> gill_attention_append -> out-projection
(gill_opt_cached_uses_w8 is the branch); the prefill, the calls of more rows and every call of a bf16 handle keep the bf16 kernels.

Geometries, schedules, batches and weights are kv_cache_util.GEOMETRIES' (opt125: 12 layers, 30 + 20 x 1 + 8 + 68 x 1 + 8 + 70 x 1 at
B = 2 and 9; opt67: 2 layers, 30 + 1 + 1 + 1 + 8 + 25 x 1 at B = 1 and 4) on peaked_opt_state_dict, teacher-forced.  Three handles run each
schedule, as test_w8_decode_gpu._run builds them: w8 on sd, mode 0 on w8_util.w8_state_dict(sd) (the same bf16 values as the w8 handle's
dequantised copies), mode 0 on sd.

  branch query      1 exactly for a w8 handle, past > 0 and B * T_new <= 16;
  oracle            every call of the w8 handle against oracle.opt_ref on w8_state_dict(sd) at REL_BAR / COS_BAR (kv_cache_util.check_calls).
                    At B = 4 and B = 9 the 8-token block has more than 16 rows and falls back to the bf16 kernels on a cache the routed
                    steps wrote, and the routed steps after it read what it wrote: the cache-compatibility check;
  prefill           bit-identical to the mode-0 handle on the dequantised weights;
  routed calls      within CACHED_VS_FULL_REL_BAR of that handle and NOT bit-identical to it (another fp32 summation order);
  weights in use    against the mode-0 handle on the original sd the routed calls differ by more than CACHED_VS_FULL_REL_BAR;
  exact identities  an 8-token step equals 8 single-token steps from the same cache state (B = 1 and 2); a row's routed steps at B = 1 equal
                    its rows at B = 2; a T_new = 1 routed call equals gill_opt_decode_step with every length = past_len.
tests/test_w8_cached_host.py shows on the CPU that on these weights every defect of kv_cache_util.DEFECTS misses the oracle bars by 48x or
more while bf16 kernel arithmetic stays within 0.19 of them."""
import pytest
import torch

import kv_cache_util as U
import w8_util as W
from oracle import opt_ref
from test_ragged_decode_gpu import SLOW, _weights
from test_w8_decode_gpu import _HandleEx, _sdq

pytestmark = pytest.mark.gpu

CASES = [("opt125", 2), ("opt125", 9), pytest.param("opt67", 1, marks=SLOW), pytest.param("opt67", 4, marks=SLOW)]
_RUN = {}


def _routed(B, past, tn):
  return past > 0 and B * tn <= W.MAX_ROWS


def _run(cuda, geom, B):
  """The geometry's schedule at batch B on the three handles, once per module."""
  if (geom, B) not in _RUN:
    cfg, sd, seed = _weights(geom)
    schedule = U.GEOMETRIES[geom]["schedule"]
    T = sum(schedule)
    x = U.token_embeds(sd, cfg, B, T, seed)
    out = dict(cfg=cfg, x=x, calls=U.calls_of(schedule))
    for key, weights, mode in (("w8", sd, 1), ("dq", _sdq(geom), 0), ("bf", sd, 0)):
      h = _HandleEx(weights, cfg, max(B, 8), T + 30, cuda, mode)
      try:
        out[key] = [h.cached(x[:, past:past + tn], past) for past, tn in out["calls"]]
      finally:
        h.close()
    _RUN[(geom, B)] = out
  return _RUN[(geom, B)]


def test_branch_query(cuda):
  from gill_amd import _native as N
  cfg, sd, _ = _weights("opt125")
  lib = N.lib()
  rows = lib.gill_w8_max_rows()
  assert rows == W.MAX_ROWS
  h8, h0 = _HandleEx(sd, cfg, 8, 64, cuda, 1), _HandleEx(sd, cfg, 8, 64, cuda, 0)
  try:
    for B in (1, 2, 3, 4, 8, 9, 16, 17):
      for tn in (1, 2, 4, 8, 16, 17):
        for past in (0, 1, 30):
          assert lib.gill_opt_cached_uses_w8(h8.h, B, tn, past) == int(past > 0 and B * tn <= rows), (B, tn, past)
          assert lib.gill_opt_cached_uses_w8(h0.h, B, tn, past) == 0, (B, tn, past)
    assert lib.gill_opt_cached_uses_w8(h8.h, 1, 16, 5) == 1 and lib.gill_opt_cached_uses_w8(h8.h, 1, 17, 5) == 0
    assert lib.gill_opt_cached_uses_w8(h8.h, 2, 8, 0) == 0
    assert lib.gill_opt_cached_uses_w8(None, 1, 1, 5) == 0
    # the ragged step's query and the row limit are what they were
    assert lib.gill_opt_decode_uses_w8(h8.h, rows) == 1 and lib.gill_opt_decode_uses_w8(h8.h, rows + 1) == 0
  finally:
    h8.close()
    h0.close()


@pytest.mark.parametrize("geom,B", CASES)
def test_w8_cached_vs_oracle_on_the_dequantised_weights(cuda, geom, B):
  r = _run(cuda, geom, B)
  cfg = r["cfg"]
  ref = opt_ref.opt_hidden_states(_sdq(geom), cfg.num_layers, cfg.num_heads, r["x"])
  unrouted = [c for c, (past, tn) in enumerate(r["calls"]) if past > 0 and not _routed(B, past, tn)]
  print(f"[{geom} B={B}] calls past the prefill that fall back to the bf16 kernels: {[r['calls'][c] for c in unrouted]}")
  assert bool(unrouted) == (B * 8 > W.MAX_ROWS)
  U.check_calls(f"{geom} B={B} w8 cached vs oracle on w8_state_dict", r["w8"], ref, r["calls"])


@pytest.mark.parametrize("geom,B", CASES)
def test_w8_cached_vs_bf16_handle_on_the_dequantised_weights(cuda, geom, B):
  r = _run(cuda, geom, B)
  calls = r["calls"]
  assert calls[0][0] == 0 and torch.equal(r["w8"][0], r["dq"][0]), \
    f"prefill differs by {(r['w8'][0] - r['dq'][0]).abs().max().item():.3e}: it must run the bf16 kernels on w8 * s"
  routed = [c for c, (past, tn) in enumerate(calls) if _routed(B, past, tn)]
  assert routed
  U.check_calls(f"{geom} B={B} routed w8 calls vs bf16 calls on the same weights", [r["w8"][c] for c in routed],
                torch.cat(r["dq"], 1), [calls[c] for c in routed], rel_bar=U.CACHED_VS_FULL_REL_BAR)
  same = [calls[c] for c in routed if torch.equal(r["w8"][c], r["dq"][c])]
  print(f"[{geom} B={B}] routed calls bit-identical to the bf16 handle: {len(same)} of {len(routed)}")
  assert not same, f"routed calls {same[:5]} are bit-identical to the bf16 kernels' result: they did not run on the e4m3 bytes"


@pytest.mark.parametrize("geom,B", CASES)
def test_w8_cached_differs_from_the_unquantised_model(cuda, geom, B):
  r = _run(cuda, geom, B)
  rels = [((r["w8"][c] - r["bf"][c]).norm() / r["bf"][c].norm()).item() for c, (past, tn) in enumerate(r["calls"]) if _routed(B, past, tn)]
  print(f"[{geom} B={B}] routed w8 calls vs the mode-0 handle on the original weights: per-call rel-L2 {min(rels):.3e} .. {max(rels):.3e}")
  assert max(rels) > U.CACHED_VS_FULL_REL_BAR


@pytest.mark.parametrize("geom", ["opt125", pytest.param("opt67", marks=SLOW)])
def test_exact_identities_chunk_batch_and_step(cuda, geom):
  """On one w8 handle, from the cache state a B = 2 prefill of 30 tokens leaves (a call at past_len rewrites the slots from past_len on and
  reads nothing beyond its own rows, so every replay below starts from the same state)."""
  cfg, sd, seed = _weights(geom)
  x = U.token_embeds(sd, cfg, 2, 46, seed + 7)
  h = _HandleEx(sd, cfg, 8, 64, cuda, 1)
  try:
    h.cached(x[:, :30], 0)
    for B in (2, 1):
      xb = x[:B]
      block = h.cached(xb[:, 30:38], 30)                                       # one 8-token step
      singles = [h.cached(xb[:, 30 + i:31 + i], 30 + i) for i in range(8)]     # the same 8 tokens one by one
      assert torch.equal(block, torch.cat(singles, 1)), \
        f"B={B}: an 8-token step differs from 8 single-token steps by {(block - torch.cat(singles, 1)).abs().max().item():.3e}"
      again = h.cached(xb[:, 30:38], 30)
      assert torch.equal(block, again), f"B={B}: the 8-token step is not repeatable"
      if B == 2:
        block2, singles2 = block, singles
      else:
        # batch identity: row 0 alone on the same cache rows
        assert torch.equal(block[0], block2[0]), "the 8-token step of row 0 at B = 1 differs from its rows at B = 2"
        for i in range(8):
          assert torch.equal(singles[i][0], singles2[i][0]), f"step {i} of row 0 at B = 1 differs from its row at B = 2"
      # step identity: gill_opt_decode_step with every length = past_len
      for i in (0, 3, 7):
        st = h.step(xb[:, 30 + i], [30 + i] * B)
        assert torch.equal(st, singles[i][:, 0]), f"B={B}: a T_new = 1 call at past {30 + i} differs from gill_opt_decode_step"
    # a two-token and a 16-token chunk against the single steps (B = 1: 16 rows)
    ref16 = torch.cat([h.cached(x[:1, 30 + i:31 + i], 30 + i) for i in range(16)], 1)
    assert torch.equal(h.cached(x[:1, 30:46], 30), ref16)
    two = torch.cat([h.cached(x[:1, 30 + i:32 + i], 30 + i) for i in range(0, 16, 2)], 1)
    assert torch.equal(two, ref16)
  finally:
    h.close()
