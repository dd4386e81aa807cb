"""CPU-side checks of the on-device decode decision's C ABI (csrc/decode.hip, include/gill_amd.h): the rule struct as
ctypes lays it out, and argument errors reported before anything is launched."""
import ctypes as C


def test_decode_rule_struct_layout():
  from gill_amd import _native as N
  r = N.gill_decode_rule
  # int32 n_ret, ret_ids[16], n_gen, gen_ids[16], step, min_word_tokens, ret_eq_gen, then three doubles (8-aligned)
  assert r.ret_ids.offset == 4 and r.n_gen.offset == 68 and r.gen_ids.offset == 72
  assert r.ret_eq_gen.offset == 144 and r.ret_scale.offset == 152 and r.filter_value.offset == 168
  assert C.sizeof(r) == 176


def test_decode_entries_reject_bad_arguments():
  from gill_amd import _native as N
  lib = N.lib()
  rule = N.gill_decode_rule()
  assert lib.gill_opt_filter_logits(None, None, None, 1, 0.7, 0.9, float("-inf"), 1, None) != 0
  assert lib.gill_last_error()
  assert lib.gill_opt_pick_token(None, None, 1, C.byref(rule), None, 1, 0, None, None, None) != 0
  assert lib.gill_opt_next_token(None, None, 1, 1, C.byref(rule), None, None, 1, 0, None, None, None) != 0
  assert lib.gill_opt_decode_logits(None, None, 1, 1, C.byref(rule), None, None) != 0
  assert b"null" in lib.gill_last_error()
