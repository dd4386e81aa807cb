"""SHA-256 of one UNet output on seeded weights, for bit-identity A/B runs of two builds of libgill_amd (GILL_AMD_LIB), one fresh process per case:
  python tools/forward_digest.py <case>
    a  SD-1.5 at sample 64, batch 2 forward, two different timesteps        g / h / i  case a under GILL_UNET_LNPROJ=0 / GILL_UNET_XALG=0 /
    b  SD-1.5 at 64, a 2-step CFG loop with B = 1 (shared prefix, then the captured graph)        GILL_UNET_FFN_FUSED=0 (set here, before the library loads)
    c  SD-1.5 at sample 32, batch 2 forward
    d  the SD-2.1 geometry (heads 5 / 10 / 20 / 20, 1024-d context) at sample 32, batch 2
    e  UNetConfig.tiny(16), batch 3
    f  SD-1.5 with fp8_convs, batch 2
Prints `<case> <digest> construction took <bytes> of device memory` (the drop in free device memory across GillSDPipeline construction)."""
import hashlib
import os
import sys

case = sys.argv[1]
SWITCH = {"g": "GILL_UNET_LNPROJ", "h": "GILL_UNET_XALG", "i": "GILL_UNET_FFN_FUSED"}
if case in SWITCH:
  os.environ[SWITCH[case]] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gill_amd
gill_amd.configure_hip_runtime()
from gill_amd import synth
from gill_amd.sd import GillSDPipeline

U = synth.UNetConfig
cfg, B = {"a": (U.sd15(), 2), "b": (U.sd15(), 1), "c": (U(sample_size=32), 2),
          "d": (U(cross_attention_dim=1024, sample_size=32, heads_per_level=(5, 10, 20, 20), prediction_type="v_prediction"), 2),
          "e": (U.tiny(16), 3), "f": (U(fp8_convs=True), 2), "g": (U.sd15(), 2), "h": (U.sd15(), 2), "i": (U.sd15(), 2)}[case]
L, E = cfg.sample_size, cfg.cross_attention_dim
sd = {k: v.bfloat16() for k, v in synth.unet_state_dict(cfg, seed=95).items()}
torch.cuda.init()
free0 = torch.cuda.mem_get_info()[0]
pipe = GillSDPipeline(sd, cfg, synth.uncond_context(cfg.ctx_len, E, seed=95), "cuda:0", max_batch=4)
torch.cuda.synchronize()
took = free0 - torch.cuda.mem_get_info()[0]
ctx = synth.normal("fd_c", (B, cfg.ctx_len, E), 97)
if case == "b":
  y = pipe(prompt_embeds=ctx.cuda().bfloat16(), latents=synth.initial_latents(B, size=L), num_inference_steps=2, guidance_scale=7.5,
           output_type="latent").images
else:
  y = pipe.unet(synth.normal("fd_x", (B, 4, L, L), 96), torch.tensor([961.0, 41.0, 500.0][:B]), ctx)
y = y.float().cpu().contiguous()
assert bool(torch.isfinite(y).all())
print(case, hashlib.sha256(y.numpy().tobytes()).hexdigest(), "construction took", took, "of device memory", flush=True)
