"""Host checks of inpainting (gill_sd_inpaint_keep: csrc/sd_schedule.hip; GillSDPipeline.preprocess_mask); no GPU.

The keep table's row i is the add_noise pair at the noise level the latents have after call i: gill_sd_schedule_from's own pair one step on for
ddim / dpmsolver++ / euler / euler_ancestral, (sqrt(abar), sqrt(1 - abar)) at timestep i + 1 of the replayed warm-up list for pndm, and (1, 0)
after the last call.  Values are fp32 (built in double, rounded once): compared to fp32 rounding, abs <= 1e-7 * max(1, |v|)."""
import ctypes as C

import numpy as np
import pytest
import torch

import inpaint_util as I
import sampler_util as U
import vae_encoder_util as V

N_STEPS, STARTS = 6, (0, 3, 5)


def _close(got, want):
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  return bool((np.abs(got - want) <= 1e-7 * np.maximum(1.0, np.abs(want))).all())


def _library_alphas_cumprod():
  """The fp32 abar table the library's schedules are built from, widened (gill_pndm_schedule exports it)."""
  from gill_amd import _native as N
  ts, ac = (C.c_int32 * 16)(), (C.c_double * 1000)()
  assert N.lib().gill_pndm_schedule(N_STEPS, ts, ac) == N_STEPS + 1
  return np.array(ac[:], dtype=np.float64)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("kind", U.KINDS)
def test_keep_table(kind, start):
  k, keep = I.native_keep(kind, 0, N_STEPS, start)
  ncalls, ts, _, _, _ = V.native_schedule_from(kind, 0, N_STEPS, start)
  assert k == ncalls and keep.shape == (ncalls, 2)
  assert keep[-1, 0] == 1.0 and keep[-1, 1] == 0.0
  ac = _library_alphas_cumprod()
  for i in range(ncalls - 1):
    if kind == "pndm":
      t = int(ts[i + 1])
      want = (np.sqrt(ac[t]), np.sqrt(1 - ac[t]))
    else:
      want = V.native_schedule_from(kind, 0, N_STEPS, start + i + 1)[4]
    assert _close(keep[i], want), (kind, start, i, keep[i], want)
  if kind == "pndm" and ncalls > 2:      # (start == N - 1 is the warm-up pair alone: row 1 is then the last row)
    assert np.array_equal(keep[0], keep[1])


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("kind", U.KINDS)
def test_keep_table_against_the_float64_restatement(kind, start):
  """inpaint_util.keep_ref (what the GPU tests' CPU drivers blend with) is built on torch's abar; the library's own fp32 product is held to 5e-6
  relative of it (tests/test_native_abi.py), so the bars are those of tests/test_schedule_from_host.py::test_add_noise_pair: that bound pushed
  through a = sqrt(abar), b = sqrt(1 - abar) and sigma = sqrt(1 / abar - 1)."""
  _, keep = I.native_keep(kind, 0, N_STEPS, start)
  ref = I.keep_ref(kind, N_STEPS, start)
  assert keep.shape == ref.shape and np.array_equal(keep[-1], ref[-1])
  for (a, b), (ra, rb) in zip(keep[:-1], ref[:-1]):
    if kind in ("euler", "euler_ancestral"):
      abar = 1.0 / (1.0 + rb * rb)
      assert a == 1.0 and ra == 1.0 and abs(b - rb) <= 2.5e-6 / (abar * rb) + 1e-7 * rb, (kind, start, b, rb)
    else:
      abar = ra * ra
      assert abs(a - ra) <= 2.5e-6 * ra + 1e-7 and abs(b - rb) <= 2.5e-6 * abar / rb + 1e-7, (kind, start, a, b, ra, rb)


@pytest.mark.parametrize("kind", U.KINDS)
def test_keep_refuses_what_the_schedule_refuses(kind):
  for n, start in ((N_STEPS, -1), (N_STEPS, N_STEPS), (0, 0), (1001, 0)):
    assert I.native_keep(kind, 0, n, start)[0] < 0, (kind, n, start)
    assert V.native_schedule_from(kind, 0, n, start)[0] < 0


def test_keep_is_the_same_for_v_prediction():
  for kind in U.KINDS:
    assert np.array_equal(I.native_keep(kind, 1, N_STEPS, 3)[1], I.native_keep(kind, 0, N_STEPS, 3)[1])


class _Cfg:
  sample_size = 4


def test_preprocess_mask_forms():
  from PIL import Image
  from gill_amd.sd import GillSDPipeline
  pipe = GillSDPipeline.__new__(GillSDPipeline)     # host plumbing only: no handle
  pipe.cfg = _Cfg()
  rng = np.random.default_rng(3)
  u8 = rng.integers(0, 256, size=(2, 32, 32), dtype=np.uint8)
  arr = u8.astype(np.float32) / 255.0
  want = torch.from_numpy(arr)[:, None]
  pil = [Image.fromarray(a, mode="L") for a in u8]
  forms = {"pil list": pil, "(B,H,W) array": arr, "(B,H,W,1) array": arr[..., None], "(B,1,H,W) tensor": want.clone()}
  for name, f in forms.items():
    got = pipe.preprocess_mask(f)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 1, 32, 32) and torch.equal(got, want), name
  assert torch.equal(pipe.preprocess_mask(pil[0]), want[:1])                    # one PIL image: batch 1
  assert torch.equal(pipe.preprocess_mask(pil[0].convert("RGB")), want[:1])     # converted to "L" (grey RGB -> the same values)
  for bad in (np.zeros((2, 16, 16), np.float32), torch.zeros(2, 3, 32, 32), torch.zeros(32, 32)):
    with pytest.raises(ValueError, match="32x32"):
      pipe.preprocess_mask(bad)


def test_prepare_ref_takes_the_top_left_pixel_of_every_cell():
  img = torch.ones(1, 3, 16, 16)
  m = torch.zeros(1, 1, 16, 16)
  m[0, 0, 8, 0] = 1.0
  m[0, 0, 3, 3] = 0.5
  masked, lm = I.prepare_ref(img, m)
  assert lm.tolist() == [[[[0.0, 0.0], [1.0, 0.0]]]]
  assert masked[0, :, 8, 0].abs().sum() == 0 and masked[0, :, 3, 3].abs().sum() == 0 and masked.sum() == 3 * (256 - 2)
  assert torch.equal(lm, torch.nn.functional.interpolate((m >= 0.5).float(), size=(2, 2)))
