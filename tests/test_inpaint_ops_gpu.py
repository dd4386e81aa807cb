"""The inpainting kernels (csrc/elementwise.hip: inpaint_prepare_kernel, sd_blend_kernel, sd_stage_concat_kernel) on their own.

Prepare: exact against inpaint_util.prepare_ref, with the threshold's two neighbours and a plane that is set only off the latent grid.
Loop under a teacher (gill_op_sd_inpaint_run, B = 2, latents 4 x 8 x 8, 6 steps from start 0 and 3, every sampler): against the row semantics
in float64 with the blend after every call, at the bar of tests/test_samplers_gpu.py — for a binary mask the blend is a select between two fp32
values and adds no term of its own — plus the identities the mask's two extremes and the concat layout must satisfy bit for bit."""
import numpy as np
import pytest
import torch

import inpaint_util as I
import sampler_util as U
import vae_encoder_util as V
from test_samplers_gpu import BAR

pytestmark = pytest.mark.gpu

CASES = [("pndm", 0.0), ("ddim", 0.0), ("ddim", 0.7), ("dpmsolver++", 0.0), ("euler", 0.0), ("euler_ancestral", 0.0)]
B, C_LAT, HW, N_STEPS, G = 2, 4, 64, 6, 7.5
N_LAT = C_LAT * HW


@pytest.mark.parametrize("Bm", [1, 2])
def test_prepare_is_exact(cuda, Bm):
  from gill_amd import ops
  Bi, H = 2, 32
  img = V.test_images(Bi, H, seed=31)
  rng = np.random.default_rng(32)
  m = rng.random((Bm, 1, H, H)).astype(np.float32)
  m[0, 0, 0, :8] = 0.5                                  # exactly the threshold: repaint
  m[0, 0, 8, :8] = np.nextafter(np.float32(0.5), np.float32(0))     # one ulp below: keep
  m[0, 0, 16, 0], m[0, 0, 16, 8] = 0.5, np.nextafter(np.float32(0.5), np.float32(0))
  off = np.zeros((H, H), np.float32)
  off[3::8, 3::8] = 1.0                                 # set only off the latent grid: latent mask all zero, pixels still zeroed
  m[Bm - 1, 0] = off if Bm == 2 else m[0, 0]
  mask = torch.from_numpy(m)
  want_img, want_lm = I.prepare_ref(img, mask)
  got_img, got_lm = ops.sd_inpaint_prepare(img.to(cuda), mask.to(cuda))
  assert tuple(got_lm.shape) == (Bi, 1, H // 8, H // 8)
  assert torch.equal(got_img.cpu(), want_img) and torch.equal(got_lm.cpu(), want_lm)
  assert want_lm[0, 0, 0, 0] == 1 and want_lm[0, 0, 1, 0] == 0 and want_lm[0, 0, 2, 0] == 1 and want_lm[0, 0, 2, 1] == 0
  if Bm == 2:
    assert got_lm[1].abs().sum() == 0 and got_img[1, :, 3::8, 3::8].abs().sum() == 0 and got_img[1].abs().sum() > 0


def test_prepare_off_grid_plane_with_one_mask_for_the_batch(cuda):
  from gill_amd import ops
  img = V.test_images(2, 32, seed=33)
  mask = torch.zeros(1, 1, 32, 32)
  mask[0, 0, 3::8, 3::8] = 1.0
  want_img, want_lm = I.prepare_ref(img, mask)
  got_img, got_lm = ops.sd_inpaint_prepare(img.to(cuda), mask.to(cuda))
  assert torch.equal(got_img.cpu(), want_img) and torch.equal(got_lm.cpu(), want_lm) and got_lm.abs().sum() == 0
  assert got_img[:, :, 3::8, 3::8].abs().sum() == 0


def _inputs(kind, eta, start):
  k, ts, sig, rows, (a, b) = V.native_schedule_from(kind, 0, N_STEPS, start, eta)
  x0, mo, z = U.teacher_inputs(70 + start, k, B, 2 * B, N_LAT)
  rng = np.random.default_rng(80 + start)
  z0 = rng.standard_normal((B, N_LAT)).astype(np.float32)
  xm = rng.standard_normal((B, N_LAT)).astype(np.float32)
  m = (rng.random((B, HW)) < 0.5).astype(np.float32)      # a different mask per sample, about half ones
  noisy = bool((rows[:, 11] != 0).any())
  return k, rows, (a, b), x0, z0, xm, m, mo, (z if noisy else None)


def _full(m):      # (B,hw) -> (B,n): one plane per sample over the channels
  return np.tile(m, (1, C_LAT))


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("kind,eta", CASES)
def test_blend_loop_under_a_teacher(cuda, kind, eta, start):
  from gill_amd import ops
  k, rows, (a, b), x0, z0, _, m, mo, z = _inputs(kind, eta, start)
  if kind == "euler" and start == 3:
    m = np.repeat(m[:1], B, axis=0)      # a batch-1 mask, repeated by the caller
  t = lambda v: None if v is None else torch.from_numpy(v).to(cuda)  # noqa: E731
  run = lambda mask: ops.sd_inpaint_run(kind, False, N_STEPS, start, G, t(x0), t(z0), t(mask), t(mo), t(z), eta=eta)  # noqa: E731
  got_l, got_i = run(m)
  assert tuple(got_l.shape) == (k, B, N_LAT) and tuple(got_i.shape) == (k, 2 * B, N_LAT)
  _, keep = I.native_keep(kind, 0, N_STEPS, start, eta)
  xs = a * x0.astype(np.float64) + b * z0.astype(np.float64)
  want_l, want_i = I.apply_rows_after(rows, G, xs, mo, z, I.blend(keep, x0, z0, _full(m)))
  gl, gi = got_l.cpu().numpy(), got_i.cpu().numpy()
  worst_l = max(U.rel_l2(gl[i], want_l[i]) for i in range(k))
  worst_i = max(max(U.rel_l2(gi[i, :B], want_i[i]), U.rel_l2(gi[i, B:], want_i[i])) for i in range(k))
  print(f"[inpaint blend {kind} eta={eta} start={start}] worst per-call rel_l2: latents {worst_l:.3e}, UNet inputs {worst_i:.3e} (bar {BAR:.3e})")
  assert worst_l <= BAR and worst_i <= BAR
  assert torch.equal(got_i[:, :B], got_i[:, B:])      # both CFG halves
  # kept pixels after every call: fl32(ka * x0 + kb * z0) to 1 ulp of that value, (ka, kb) the fp32 pair the device reads
  kept = _full(m) == 0
  worst_ulp = 0.0
  for i in range(k):
    ka, kb = np.float64(np.float32(keep[i, 0])), np.float64(np.float32(keep[i, 1]))
    exact = ka * x0.astype(np.float64) + kb * z0.astype(np.float64)
    ulp = np.spacing(np.abs(exact.astype(np.float32))).astype(np.float64)
    err = np.abs(gl[i].astype(np.float64) - exact) / ulp
    worst_ulp = max(worst_ulp, float(err[kept].max()))
  print(f"[inpaint blend {kind} eta={eta} start={start}] kept pixels: worst distance from ka x0 + kb z0 = {worst_ulp:.3f} ulp")
  assert worst_ulp <= 1.0
  # mask all ones: the loop without a mask, bit for bit
  plain_l, plain_i = ops.sd_sampler_run_from(kind, False, N_STEPS, start, G, t(x0), t(z0), t(mo), t(z), eta=eta)
  ones_l, ones_i = run(np.ones_like(m))
  assert torch.equal(ones_l, plain_l) and torch.equal(ones_i[:, :B], plain_i)
  # mask all zeros: the clean image latents at the end, bit for bit
  zeros_l, _ = run(np.zeros_like(m))
  assert torch.equal(zeros_l[-1].cpu(), torch.from_numpy(x0))


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("kind,eta", CASES)
def test_concat_loop_under_a_teacher(cuda, kind, eta, start):
  from gill_amd import ops
  k, rows, (a, b), x0, z0, xm, m, mo, z = _inputs(kind, eta, start)
  t = lambda v: None if v is None else torch.from_numpy(v).to(cuda)  # noqa: E731
  got_l, got_i = ops.sd_inpaint_run(kind, False, N_STEPS, start, G, t(x0), t(z0), t(m), t(mo), t(z), eta=eta, masked_latents=t(xm))
  n_in = (2 * C_LAT + 1) * HW
  assert tuple(got_l.shape) == (k, B, N_LAT) and tuple(got_i.shape) == (k, 2 * B, n_in)
  plain_l, plain_i = ops.sd_sampler_run_from(kind, False, N_STEPS, start, G, t(x0), t(z0), t(mo), t(z), eta=eta)
  assert torch.equal(got_l, plain_l)      # no blend
  gi = got_i.reshape(k, 2, B, 2 * C_LAT + 1, HW)
  for half in range(2):
    assert torch.equal(gi[:, half, :, :C_LAT].reshape(k, B, N_LAT), plain_i)      # in_scale * latents, as the plain stage kernel forms it
    assert torch.equal(gi[:, half, :, C_LAT].cpu(), torch.from_numpy(m).expand(k, -1, -1))
    assert torch.equal(gi[:, half, :, C_LAT + 1:].reshape(k, B, N_LAT).cpu(), torch.from_numpy(xm).expand(k, -1, -1))
  xs = a * x0.astype(np.float64) + b * z0.astype(np.float64)
  want_l, want_i = I.apply_rows_after(rows, G, xs, mo, z)
  worst = max(max(U.rel_l2(got_l[i].cpu().numpy(), want_l[i]), U.rel_l2(gi[i, 0, :, :C_LAT].reshape(B, N_LAT).cpu().numpy(), want_i[i]))
              for i in range(k))
  print(f"[inpaint concat {kind} eta={eta} start={start}] worst per-call rel_l2={worst:.3e} (bar {BAR:.3e})")
  assert worst <= BAR


def test_operator_argument_errors(cuda):
  from gill_amd import _native as N
  from gill_amd import ops
  _, _, _, x0, z0, _, m, mo, _ = _inputs("ddim", 0.0, 3)
  t = lambda v: torch.from_numpy(v).to(cuda)  # noqa: E731
  with pytest.raises(ValueError, match="latent_mask"):
    ops.sd_inpaint_run("ddim", False, N_STEPS, 3, G, t(x0), t(z0), t(m[:, :60]), t(mo))       # hw does not divide n
  with pytest.raises(ValueError, match="mask must be"):
    ops.sd_inpaint_prepare(torch.zeros(2, 3, 32, 32, device=cuda), torch.zeros(3, 1, 32, 32, device=cuda))
  with pytest.raises(N.GillNativeError, match="multiples of 8"):
    ops.sd_inpaint_prepare(torch.zeros(1, 3, 36, 36, device=cuda), torch.zeros(1, 1, 36, 36, device=cuda))
