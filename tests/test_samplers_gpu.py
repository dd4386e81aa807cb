"""GPU checks of the samplers beside PNDM: the stage / step kernels under a teacher (gill_op_sd_sampler_run), and the whole pipeline on the
tiny UNet against the CPU oracle driven by sampler_util's float64 restatements."""
import json
import os

import numpy as np
import pytest
import torch

import sampler_util as U
from gill_amd import synth

pytestmark = pytest.mark.gpu

# (B, n): a partial block; n no multiple of the block; several blocks; and — grid_for caps a launch at 8192 blocks of 256 threads — one more
# element count than a single pass of the capped grid covers, so the grid-stride loop's second pass runs (2 calls only: it is 8 MiB a row)
SHAPES = ((1, 64), (3, 144), (2, 16384))
BIG = (1, 8192 * 256 + 77)
SAMPLERS = (("ddim", 0.0), ("ddim", 0.7), ("dpmsolver++", 0.0), ("euler", 0.0), ("euler_ancestral", 0.0))
# Largest per-call rel-L2 between the float32 and the float64 run of the restatement over every case of
# test_sampler_kernels_vs_float64_restatement (CPU, same inputs; tools/sampler_tolerance.py prints it per sampler): 8.93e-07, at Euler with
# v-prediction, whose eps = (x - x0) / sigma cancels; every other sampler stays below 5e-07.  The bar is 10 x that.
F32_DISTANCE = 8.93e-7
BAR = 10 * F32_DISTANCE
assert BAR <= 1e-4      # a bar above that would hold something other than rounding


def _seed(B, n, N):
  return 17 * B + n % 1000 + N


def kernel_cases():
  """(B, n, N, guidance) of the restatement comparison — also what tools/sampler_tolerance.py sweeps."""
  return [(B, n, N, g) for (B, n) in SHAPES for N in (2, 3, 20) for g in (1.0, 7.5)] + [(BIG[0], BIG[1], 2, 7.5)]


def _case(kind, eta, pred, N, g, B, n, dev):
  Bx = 2 * B if g > 1 else B
  lat0, mo, z = U.teacher_inputs(_seed(B, n, N), N, B, Bx, n)
  z = z if U.needs_noise(kind, eta) else None
  want = U.run_ref(kind, pred, N, g, lat0, mo, z, eta)
  t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
  return t(lat0), t(mo), t(z), want


def _check(kind, eta, pred, N, g, B, n, dev):
  from gill_amd import ops
  lat0, mo, z, (want_l, want_i) = _case(kind, eta, pred, N, g, B, n, dev)
  got_l, got_i = ops.sd_sampler_run(kind, pred == "v_prediction", N, g, lat0, mo, z, eta=eta)
  gl, gi = got_l.cpu().numpy(), got_i.cpu().numpy()
  worst = max(max(U.rel_l2(gl[i], want_l[i]), U.rel_l2(gi[i], want_i[i])) for i in range(N))
  return worst


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("kind,eta", SAMPLERS)
def test_sampler_kernels_vs_float64_restatement(cuda, kind, eta, pred):
  """Latents after every call and UNet input of every call against the float64 restatement, per-call rel-L2 <= BAR.
  Measured on the CPU (float32 numpy restatement against the float64 one, these cases): 8.93e-07; bar 8.93e-06.
  The kernels measure 1.0e-06 ... 1.5e-06; DPM-Solver++ with v-prediction 5.4e-06, at the last of 20 calls, whose second-order extrapolation to
  t = 0 weighs the two stored x0 with +2.98 and -2.11 (float32 numpy applied to the same folded rows gives the same figure)."""
  worst = {c: _check(kind, eta, pred, c[2], c[3], c[0], c[1], cuda) for c in kernel_cases()}
  print(f"[sampler kernels {kind} eta={eta} {pred}] worst per-call rel_l2={max(worst.values()):.3e} (bar {BAR:.3e})")
  for c, w in worst.items():
    assert w <= BAR, (kind, eta, pred, c, w)


@pytest.mark.parametrize("kind,eta", [("ddim", 0.0), ("dpmsolver++", 0.0), ("euler", 0.0)])
def test_noise_table_is_not_read_by_rows_without_noise(cuda, kind, eta):
  from gill_amd import ops
  B, n, N = 3, 144, 3
  lat0, mo, _, _ = _case(kind, eta, "epsilon", N, 7.5, B, n, cuda)
  poison = torch.full((N, B, n), float("nan"), device=cuda)
  a = ops.sd_sampler_run(kind, False, N, 7.5, lat0, mo, poison, eta=eta)
  b = ops.sd_sampler_run(kind, False, N, 7.5, lat0, mo, None, eta=eta)
  for x, y in zip(a, b):
    assert torch.isfinite(x).all() and torch.equal(x, y)


def test_missing_noise_table_is_an_error(cuda):
  from gill_amd import _native as N, ops
  lat0, mo, _, _ = _case("euler_ancestral", 0.0, "epsilon", 3, 1.0, 1, 64, cuda)
  with pytest.raises(N.GillNativeError, match="noise"):
    ops.sd_sampler_run("euler_ancestral", False, 3, 1.0, lat0, mo, None)


@pytest.mark.parametrize("kind,eta", [("ddim", 0.7), ("dpmsolver++", 0.0), ("euler_ancestral", 0.0)])
def test_sampler_kernels_bit_reproducible(cuda, kind, eta):
  from gill_amd import ops
  lat0, mo, z, _ = _case(kind, eta, "v_prediction", 20, 7.5, 2, 16384, cuda)
  a = ops.sd_sampler_run(kind, True, 20, 7.5, lat0, mo, z, eta=eta)
  b = ops.sd_sampler_run(kind, True, 20, 7.5, lat0, mo, z, eta=eta)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_pndm_through_the_operator_entry(cuda):
  """Kind 0 runs the PLMS kernel through the same entry: against the oracle's PNDMSchedulerRef in float64 (same bar: the multistep
  combination's weights sum to 160 / 24 in magnitude, times an eps coefficient below 1 — still a few fp32 roundings per call)."""
  from gill_amd import ops
  from oracle.scheduler_ref import PNDMSchedulerRef
  B, n, N = 3, 144, 6
  lat0, mo, _ = U.teacher_inputs(5, N + 1, B, 2 * B, n)
  got_l, got_i = ops.sd_sampler_run("pndm", False, N, 7.5, torch.from_numpy(lat0).to(cuda), torch.from_numpy(mo).to(cuda))
  ref = PNDMSchedulerRef()
  lat = torch.from_numpy(lat0).double()
  for i, t in enumerate(ref.set_timesteps(N)):
    assert U.rel_l2(got_i[i].cpu().numpy(), lat.numpy()) <= BAR
    e = torch.from_numpy(mo[i]).double()
    lat = ref.step(e[:B] + 7.5 * (e[B:] - e[:B]), t, lat)
    assert U.rel_l2(got_l[i].cpu().numpy(), lat.numpy()) <= BAR, i


# ------------------------------------------------------------------------------------------------ pipeline level
def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def _stats(name, got, ref):
  got, ref = got.float().cpu(), ref.float().cpu()
  mse = ((got - ref) ** 2).mean().item()
  rel = ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()
  cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
  print(f"[{name}] mse={mse:.3e} rel_l2={rel:.3e} cos={cos:.6f} max_abs={(got - ref).abs().max().item():.3e} ref_rms={ref.pow(2).mean().sqrt().item():.3f}")
  return mse, rel, cos


@pytest.fixture(scope="module")
def rig(cuda):
  from gill_amd.sd import GillSDPipeline
  cfg = synth.UNetConfig.tiny(16)
  sd = _bfw(synth.unet_state_dict(cfg, seed=3))
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=3).bfloat16().float()
  pipe = GillSDPipeline(sd, cfg, uncond, cuda, max_batch=8)
  cond = synth.normal("dn_cond", (2, 77, cfg.cross_attention_dim), 4).bfloat16().float()
  lat0 = synth.initial_latents(2, 4, 16, seed=1337)
  return cfg, sd, uncond, pipe, cond, lat0


def _oracle(cfg, sd, uncond, cond, lat0, kind, steps, g, eta=0.0, noise=None, pred="epsilon", heads=None):
  sched = U.make_ref(kind, pred, np.float64, eta)
  return U.denoise_ref(sd, cond, uncond, lat0, sched, steps, g, cfg.block_out_channels, heads or cfg.num_heads, cfg.norm_num_groups, noise)


@pytest.mark.parametrize("kind,g", [("ddim", 7.5), ("dpmsolver++", 7.5), ("euler", 7.5), ("dpmsolver++", 1.0)])
def test_denoise_tiny_vs_oracle(rig, kind, g):
  """10 calls of the tiny UNet (batch 2B under CFG) under DDIM / DPM-Solver++ / Euler against the fp32 oracle UNet driven by the float64
  restatement; the last case runs without CFG."""
  cfg, sd, uncond, pipe, cond, lat0 = rig
  ref = _oracle(cfg, sd, uncond, cond, lat0, kind, 10, g)
  got = pipe(prompt_embeds=cond, latents=lat0, guidance_scale=g, num_inference_steps=10, scheduler=kind).images
  _, rel, cos = _stats(f"denoise tiny {kind} 10 steps, guidance {g}", got, ref)
  assert got.shape == ref.shape and rel < 8e-2


@pytest.mark.parametrize("kind,eta", [("ddim", 0.5), ("euler_ancestral", 0.0)])
def test_stochastic_denoise_tiny_vs_oracle(rig, kind, eta):
  """6 calls with variance noise: the latents, then one draw per call, from a seeded CPU generator on both sides."""
  cfg, sd, uncond, pipe, cond, _ = rig
  g2 = torch.Generator().manual_seed(99)
  lat0 = torch.randn((2, 4, 16, 16), generator=g2)
  noise = torch.stack([torch.randn((2, 4, 16, 16), generator=g2) for _ in range(6)])
  ref = _oracle(cfg, sd, uncond, cond, lat0, kind, 6, 7.5, eta, noise)
  got = pipe(prompt_embeds=cond, generator=torch.Generator().manual_seed(99), guidance_scale=7.5, num_inference_steps=6, scheduler=kind,
             eta=eta).images
  _, rel, cos = _stats(f"denoise tiny {kind} eta={eta} 6 steps", got, ref)
  assert rel < 8e-2


def test_v_prediction_ddim_tiny_vs_oracle(cuda):
  """The SD-2.x geometry (a head count per level) with v-prediction under DDIM, the scheduler SD-2.1 ships."""
  from gill_amd.sd import GillSDPipeline
  cfg = synth.UNetConfig.tiny_sd2(16)
  sd = _bfw(synth.unet_state_dict(cfg, seed=4))
  uncond = synth.uncond_context(cfg.ctx_len, cfg.cross_attention_dim, seed=4).bfloat16().float()
  pipe = GillSDPipeline(sd, cfg, uncond, cuda, max_batch=8, scheduler="ddim")
  assert cfg.prediction_type == "v_prediction" and pipe.scheduler.kind == "ddim"
  cond = synth.normal("sd2_ctx", (2, 77, cfg.cross_attention_dim), 9).bfloat16().float()
  lat0 = synth.initial_latents(2, 4, 16, seed=1337)
  ref = _oracle(cfg, sd, uncond, cond, lat0, "ddim", 10, 7.5, pred="v_prediction", heads=cfg.heads_per_level)
  got = pipe(prompt_embeds=cond, latents=lat0, guidance_scale=7.5, num_inference_steps=10).images
  _, rel, cos = _stats("denoise tiny SD-2.x v-prediction ddim 10 steps", got, ref)
  assert rel < 8e-2


def test_one_handle_never_replays_another_samplers_graph(rig):
  cfg, sd, uncond, pipe, cond, lat0 = rig
  run = lambda k, **kw: pipe(prompt_embeds=cond, latents=lat0, guidance_scale=7.5, num_inference_steps=5, scheduler=k, **kw).images  # noqa: E731
  p1 = run("pndm")
  d = run("ddim")
  run("euler_ancestral", generator=torch.Generator().manual_seed(1))
  p2 = run("pndm")
  assert torch.equal(p1, p2)
  assert torch.isfinite(d).all() and ((d - p1).norm() / p1.norm()).item() > 1e-3
  assert pipe.scheduler.kind == "pndm"      # scheduler= is the call's, not the pipeline's


def test_eta_reaches_ddim_only(rig):
  cfg, sd, uncond, pipe, cond, lat0 = rig
  run = lambda **kw: pipe(prompt_embeds=cond, latents=lat0, guidance_scale=7.5, num_inference_steps=4, **kw).images  # noqa: E731
  assert torch.equal(run(eta=0.0), run(eta=0.3))               # the default PNDM ignores it
  pipe.set_scheduler("ddim")
  try:
    a, b = run(eta=0.0), run(eta=0.0)
    assert pipe.scheduler.kind == "ddim" and torch.equal(a, b)
    c = run(eta=0.3, generator=torch.Generator().manual_seed(2))
    assert ((c - a).norm() / a.norm()).item() > 1e-3
  finally:
    pipe.set_scheduler(None)
  assert pipe.scheduler.kind == "pndm"


def test_from_pretrained_reads_the_scheduler_class(cuda, tmp_path):
  from safetensors.torch import save_file
  from gill_amd.sd import GillSDPipeline
  ucfg = synth.UNetConfig(block_out_channels=(64, 128, 256, 256), num_heads=4, cross_attention_dim=768, sample_size=16)

  def make(name, cls):
    d = str(tmp_path / name)
    os.makedirs(os.path.join(d, "unet")), os.makedirs(os.path.join(d, "scheduler"))
    with open(os.path.join(d, "unet", "config.json"), "w") as f:
      json.dump(dict(in_channels=4, out_channels=4, block_out_channels=list(ucfg.block_out_channels), layers_per_block=2,
                     cross_attention_dim=768, attention_head_dim=4, norm_num_groups=32, sample_size=16), f)
    save_file({k: v.contiguous() for k, v in synth.unet_state_dict(ucfg, seed=71).items()},
              os.path.join(d, "unet", "diffusion_pytorch_model.safetensors"))
    with open(os.path.join(d, "scheduler", "scheduler_config.json"), "w") as f:
      json.dump(dict(_class_name=cls, prediction_type="epsilon", beta_schedule="scaled_linear", steps_offset=1, set_alpha_to_one=False), f)
    save_file({"uncond_embeds": synth.uncond_context(77, 768, seed=73).contiguous()}, os.path.join(d, "uncond_embeds.safetensors"))
    return d

  cond = synth.normal("fp_cond", (1, 77, 768), 5).bfloat16().float()
  run = lambda p: p(prompt_embeds=cond, generator=torch.Generator().manual_seed(7), guidance_scale=7.5, num_inference_steps=4).images  # noqa: E731
  ddim = GillSDPipeline.from_pretrained(make("ddim", "DDIMScheduler"), device=cuda, max_batch=2)
  assert ddim.scheduler.kind == "ddim"
  a = run(ddim)
  del ddim
  pndm = GillSDPipeline.from_pretrained(make("pndm", "PNDMScheduler"), device=cuda, max_batch=2)
  assert pndm.scheduler.kind == "pndm"
  p = run(pndm)
  b = run(pndm.set_scheduler("ddim"))
  assert torch.equal(a, b) and not torch.equal(a, p)
  over = GillSDPipeline.from_pretrained(make("over", "PNDMScheduler"), device=cuda, max_batch=2, scheduler="euler")
  assert over.scheduler.kind == "euler"
