"""conv_in with two K steps (gill_op_conv_in_wide: im2col to K = 128 + the GEMM), the form the 9-channel inpainting UNet's first layer runs in:
8 .. 14 input channels against the fp64 restatement of tests/ends_util.py.  Integer inputs must come out exactly (a wrong or unzeroed padding
column of the second K step shows there); fp32 inputs within one bf16 ulp of the exact value plus 2 * 128 * 2^-24 (sum |x^ w^| + |bias|): the
bar of ends_util.check_conv_in with the accumulation length of this K."""
import pytest
import torch

import ends_util as U

pytestmark = pytest.mark.gpu

# (B, Cin, H, W, Cout): the inpainting UNet's 9 at two widths and more than one row tile, the first and last channel counts of the second K step
SHAPES = ((2, 9, 3, 5, 64), (2, 9, 8, 8, 320), (1, 8, 4, 4, 128), (1, 14, 2, 6, 64))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_conv_in_wide_matches_fp64(cuda, shape):
  from gill_amd import ops
  x, w, b = U.conv_in_inputs(shape, True)
  want = U.conv_in_exact(x, w, b)[0]
  assert want.abs().max().item() < 256      # exact in bf16 (|y| <= 9 * 14 * 2 + 8 needs checking from 13 channels up)
  for dtype in (torch.float32, torch.bfloat16):
    y, guard = ops.conv_in(x.float().to(cuda), w.to(dtype).to(cuda), b.float().to(cuda), wide=True)
    assert guard and torch.equal(y.cpu().double(), want), (shape, dtype)
  x, w, b = U.conv_in_inputs(shape, False)
  want, mag = U.conv_in_exact(x, w, b)
  y, guard = ops.conv_in(x.float().to(cuda), w.float().to(cuda), b.float().to(cuda), wide=True)
  bar = U.bf16_ulp(want) + 2.0 * 128 * 2.0 ** -24 * mag
  ratio = ((y.cpu().double() - want).abs() / bar).max().item()
  print(f"[conv_in wide {shape}] worst |got - exact| / (bf16 ulp + slack) = {ratio:.3e}")
  assert guard and bool(torch.isfinite(y).all()) and ratio <= 1.0, (shape, ratio)


def test_conv_in_wide_is_conv_in_up_to_7_channels_and_refuses_15(cuda):
  from gill_amd import _native as N, ops
  x, w, b = U.conv_in_inputs(U.CONV_IN_SHAPES[2], False)      # 7 channels: K = 64 in both entries
  xd, wd, bd = x.float().to(cuda), w.float().to(cuda), b.float().to(cuda)
  assert torch.equal(ops.conv_in(xd, wd, bd, wide=True)[0].view(torch.int16), ops.conv_in(xd, wd, bd)[0].view(torch.int16))
  with pytest.raises(N.GillNativeError, match="1 .. 14"):
    ops.conv_in(torch.zeros((1, 15, 2, 2), device=cuda), torch.zeros((64, 15, 3, 3), device=cuda), wide=True)
