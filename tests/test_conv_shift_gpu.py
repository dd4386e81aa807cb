"""The conv gather's origin shift (GemmArgs::pad_shift, gill_op_conv3x3_ex): stride-2 windows of diffusers' Downsample2D(padding=0),
F.pad(x, (0, 1, 0, 1)) + conv(stride 2, pad 0), against torch on bf16-rounded inputs and weights — the tolerance of the stride-2 case of
tests/test_ops_gpu.py (max error relative to the largest reference value < 1.5e-2)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rnd(shape, seed, scale=1.0):
  return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel(got, ref):
  got, ref = got.float().cpu(), ref.float().cpu()
  return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def _case(B, IH, IW, Cin, Cout):
  x = _rnd((B, IH, IW, Cin), 40).to(torch.bfloat16)
  w = _rnd((Cout, Cin, 3, 3), 41, 0.05)
  bias = _rnd((Cout,), 42)
  ref = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.to(torch.bfloat16).float(), bias, stride=2).permute(0, 2, 3, 1)
  return x, w, bias, ref


@pytest.mark.parametrize("B,IH,IW,Cin,Cout,sk", [
  (2, 16, 16, 64, 64, 1),
  (1, 8, 8, 64, 128, 1),       # M = 16: less than any tile
  (2, 12, 20, 128, 64, 1),     # non-square: the right and the bottom edge differ
  (1, 32, 32, 64, 64, 2),      # split-K
])
def test_shifted_stride2_conv(cuda, B, IH, IW, Cin, Cout, sk):
  from gill_amd import ops
  x, w, bias, ref = _case(B, IH, IW, Cin, Cout)
  out = ops.conv3x3_ex(x.to(cuda), w.to(cuda), 1, bias=bias.to(cuda), stride=2, splitk=sk)
  assert tuple(out.shape) == (B, IH // 2, IW // 2, Cout) == tuple(ref.shape)
  whole, row, col = _rel(out, ref), _rel(out[:, -1], ref[:, -1]), _rel(out[:, :, -1], ref[:, :, -1])
  print(f"[conv shift B{B} {IH}x{IW} {Cin}->{Cout} sk{sk}] rel_to_max whole={whole:.3e} last row={row:.3e} last col={col:.3e}")
  assert whole < 1.5e-2
  assert row < 1.5e-2 and col < 1.5e-2      # where the zero edge enters


@pytest.mark.parametrize("stride", [1, 2])
def test_no_shift_is_the_old_entry_bit_for_bit(cuda, stride):
  from gill_amd import ops
  x, w, bias, _ = _case(2, 16, 16, 64, 64)
  a = ops.conv3x3(x.to(cuda), w.to(cuda), bias.to(cuda), stride=stride, splitk=1)
  b = ops.conv3x3_ex(x.to(cuda), w.to(cuda), 0, bias=bias.to(cuda), stride=stride, splitk=1)
  assert torch.equal(a, b)


def test_bad_shift_arguments_are_refused(cuda):
  from gill_amd import _native as N, ops
  x, w, bias, _ = _case(1, 9, 8, 64, 64)      # odd IH
  with pytest.raises(N.GillNativeError, match="even"):
    ops.conv3x3_ex(x.to(cuda), w.to(cuda), 1, stride=2)
  x, w, bias, _ = _case(1, 8, 8, 64, 64)
  with pytest.raises(N.GillNativeError, match="stride 2"):
    ops.conv3x3_ex(x.to(cuda), w.to(cuda), 1, stride=1)
