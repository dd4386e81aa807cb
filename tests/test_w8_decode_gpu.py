"""The OPT engine in w8 mode (gill_opt_create_ex, GILL_OPT_W8) through the C ABI on the MI355X, like test_ragged_decode_gpu.py:
right-padded prefill, then teacher-forced single-token steps at per-row lengths.

The quantised model is the bf16 model whose four matrices per layer are w8 * s (w8_util.w8_state_dict), so
  * the reference of a w8 handle is every row alone through oracle.opt_ref on w8_state_dict(sd), at ragged_decode_util.check_ragged's
    standing bars (the arithmetic class is the bf16 path's: those bars are the reference's, not the code under test's);
  * a mode-0 handle loaded with w8_state_dict(sd) holds the same bf16 values as the w8 handle's dequantised copies: the prefill (the same
    kernels on both) must agree bit for bit, which proves the copies exact, and the decode steps (fp8 kernel against bf16 GEMM: another
    fp32 summation order) per step under kv_cache_util.CACHED_VS_FULL_REL_BAR;
  * a step at B = W8_MAX_ROWS + 1 falls back to the bf16 kernels: bit-identical to the mode-0 handle;
  * against a mode-0 handle on the ORIGINAL sd the w8 handle differs by more than that agreement bar: the quantised weights are in use.
    (tests/test_w8_host.py::test_quantisation_moves_the_oracle_by_3_bars: on the CPU the two oracles differ by 3 x the bar or more at
    these inputs.)"""
import ctypes as C

import pytest
import torch

import kv_cache_util as U
import ragged_decode_util as R
import w8_util as W
from test_ragged_decode_gpu import SLOW, _Handle, _inputs, _weights

pytestmark = pytest.mark.gpu


class _HandleEx(_Handle):
  def __init__(self, sd, cfg, max_batch, max_seq, dev, mode):
    from gill_amd import _native as N
    self.N, self.cfg, self.dev = N, cfg, dev
    c = N.gill_opt_config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                          ffn_dim=cfg.ffn_dim, max_positions=cfg.max_positions, max_batch=max_batch, max_seq=max_seq)
    arr, keep = N.make_tensor_table(sd, dev)
    self.h = C.c_void_p()
    with torch.cuda.device(dev):
      N.check(N.lib().gill_opt_create_ex(C.byref(self.h), C.byref(c), arr, len(keep), mode))
    del keep


_SDQ, _RUN = {}, {}


def _sdq(geom):
  cfg, sd, _ = _weights(geom)
  if geom not in _SDQ:
    _SDQ[geom] = W.w8_state_dict(sd, cfg)
  return _SDQ[geom]


def _run(cuda, geom, name):
  """One schedule on the three handles (w8 on sd; mode 0 on w8_state_dict(sd); mode 0 on sd), once per module."""
  if (geom, name) not in _RUN:
    cfg, sd, seed = _weights(geom)
    lengths, steps = R.RUNS[name]
    seqs, prompt_ids, step_x = _inputs(cfg, sd, lengths, steps, seed + 10)
    out = dict(cfg=cfg, lengths=lengths, steps=steps, seqs=seqs)
    for key, weights, mode in (("w8", sd, 1), ("dq", _sdq(geom), 0), ("bf", sd, 0)):
      h = _HandleEx(weights, cfg, max(len(lengths), 8), max(lengths) + steps + 5, cuda, mode)
      try:
        out[key] = h.ragged(prompt_ids, lengths, step_x)
      finally:
        h.close()
    _RUN[(geom, name)] = out
  return _RUN[(geom, name)]


def test_mode_and_branch_queries(cuda):
  from gill_amd import _native as N
  cfg, sd, _ = _weights("opt125")
  lib = N.lib()
  rows = lib.gill_w8_max_rows()
  assert rows == W.MAX_ROWS
  h8, h0 = _HandleEx(sd, cfg, 8, 64, cuda, 1), _HandleEx(sd, cfg, 8, 64, cuda, 0)
  try:
    assert lib.gill_opt_weight_mode(h8.h) == 1 and lib.gill_opt_weight_mode(h0.h) == 0
    assert lib.gill_opt_decode_uses_w8(h8.h, 1) == 1 and lib.gill_opt_decode_uses_w8(h8.h, rows) == 1
    assert lib.gill_opt_decode_uses_w8(h8.h, rows + 1) == 0
    assert lib.gill_opt_decode_uses_w8(h0.h, 1) == 0 and lib.gill_opt_decode_uses_w8(h0.h, rows) == 0
    bad = C.c_void_p()
    c = N.gill_opt_config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                          ffn_dim=cfg.ffn_dim, max_positions=cfg.max_positions, max_batch=8, max_seq=64)
    arr, keep = N.make_tensor_table(sd, cuda)
    assert lib.gill_opt_create_ex(C.byref(bad), C.byref(c), arr, len(keep), 2) != 0
  finally:
    h8.close()
    h0.close()


@pytest.mark.parametrize("geom,name", [("opt125", "b3"), ("opt125", "b9"), pytest.param("opt67", "b3", marks=SLOW)])
def test_w8_handle_vs_oracle_on_the_dequantised_weights(cuda, geom, name):
  r = _run(cuda, geom, name)
  pre, st = r["w8"]
  opro, ost = R.oracle_rows(_sdq(geom), r["cfg"], r["seqs"], r["lengths"], r["steps"])
  R.check_ragged(f"{geom} {name} w8 handle vs oracle on w8_state_dict", pre, st, opro, ost, r["lengths"])


@pytest.mark.parametrize("geom,name", [("opt125", "b3"), ("opt125", "b9"), pytest.param("opt67", "b3", marks=SLOW)])
def test_w8_handle_vs_bf16_handle_on_the_dequantised_weights(cuda, geom, name):
  r = _run(cuda, geom, name)
  (pre8, st8), (pre0, st0) = r["w8"], r["dq"]
  assert torch.equal(pre8, pre0), f"prefill differs by {(pre8 - pre0).abs().max().item():.3e}: the dequantised copies are not w8 * s"
  S = r["steps"]
  U.check_calls(f"{geom} {name} w8 steps vs bf16 steps on the same weights", [st8[:, s:s + 1] for s in range(S)], st0, [(s, 1) for s in range(S)],
                rel_bar=U.CACHED_VS_FULL_REL_BAR)


def test_w8_handle_differs_from_the_unquantised_model(cuda):
  r = _run(cuda, "opt125", "b3")
  st8, stb = r["w8"][1], r["bf"][1]
  rel = max(((st8[:, s] - stb[:, s]).norm() / stb[:, s].norm()).item() for s in range(r["steps"]))
  print(f"w8 handle vs mode-0 handle on the original weights: largest per-step rel-L2 {rel:.3e}")
  assert rel > U.CACHED_VS_FULL_REL_BAR


def test_more_rows_than_the_kernel_takes_fall_back_to_the_bf16_kernels(cuda):
  """One step at B = W8_MAX_ROWS + 1 after a prefill: bit-identical to the mode-0 handle on w8_state_dict(sd)."""
  from gill_amd import synth
  cfg, sd, seed = _weights("opt125")
  B = W.MAX_ROWS + 1
  lengths = [5 + (3 * b) % 11 for b in range(B)]
  T = max(lengths)
  ids = torch.cat([synth.synthetic_prompt_ids(16, T + 1, seed=seed + 20, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:, :T + 1],
                   synth.synthetic_prompt_ids(16, T + 1, seed=seed + 21, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:B - 16, :T + 1]])
  x = torch.nn.functional.embedding(ids[:, T], sd["model.decoder.embed_tokens.weight"])
  outs = []
  for weights, mode in ((sd, 1), (_sdq("opt125"), 0)):
    h = _HandleEx(weights, cfg, B, T + 8, cuda, mode)
    try:
      pre = h.prefill_ids(ids[:, :T])
      outs.append((pre, h.step(x, lengths)))
    finally:
      h.close()
  assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
