"""SHA-256 of the outputs of every entry point that runs the shared transformer block (csrc/tfm.hip), on seeded synthetic weights, for
bit-identity A/B runs of two builds of libgill_amd (GILL_AMD_LIB), one fresh process per case:
  python tools/opt_digest.py <case>      one case, one line `<case> <digest>`
  python tools/opt_digest.py all | <case> <case> ...      every / the named cases, each in a child process of its own
Cases `<entry>-<geometry>[-<variant>]`, geometries "opt125" / "opt67" of tests/kv_cache_util.py:
  forward        gill_opt_forward at B = 2, T = 30
  cached         gill_opt_forward_cached as 17 + 13 tokens, then three single-token steps (B = 2)
  img / imgx     gill_opt_img_hidden_ex at B = 2 without / with extra rows; ids past the top of either table, and without extra rows a negative id
  loss / loss0   gill_opt_forward_loss (extra rows, labels) with every optional output / with none
  dec-*-b3, b9   gill_opt_prefill_ids + four gill_opt_decode_step at ragged lengths on a bf16 handle; row 0 of the last step holds a device
                 length beyond the cache (clamped; its flag is read back through the ragged decision)
  w8-*-b3, b16, b17   the same on a w8 handle (b17: past W8_MAX_ROWS, the bf16 kernels on the dequantised weights)
  w8cached       gill_opt_forward_cached on a w8 handle: a 30-token prefill (the bf16 kernels), then on the e4m3 bytes three single-token steps,
                 one 8-token block and two more single steps at B = 2, and on the same handle one single step at B = 1 and at B = 8 and an
                 8-token block at B = 3 (24 rows: the bf16 kernels again, on the cache the routed steps wrote)
  mapper, clipvision, cliptext   one forward each on the smallest configurations their GPU tests use
Every output a case produces goes into its digest; hidden states of the ragged cases only at the valid rows."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOS = ("opt125", "opt67")
CASES = [f"{e}-{g}" for g in GEOS for e in ("forward", "cached", "img", "imgx", "loss", "loss0")] + \
        [f"dec-{g}-{b}" for g in GEOS for b in ("b3", "b9")] + [f"w8-{g}-{b}" for g in GEOS for b in ("b3", "b16", "b17")] + \
        ["mapper", "clipvision", "cliptext"] + [f"w8cached-{g}" for g in GEOS]

todo = CASES if sys.argv[1:] == ["all"] else sys.argv[1:]
if not todo or any(c not in CASES for c in todo):
  sys.exit(__doc__)
if len(todo) > 1:
  for c in todo:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), c], timeout=300)
    if r.returncode != 0:      # nothing more on the device after a failed case
      sys.exit(f"case {c} exited with {r.returncode}")
  sys.exit(0)

case = sys.argv[1]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch   # noqa: E402
import gill_amd   # noqa: E402
gill_amd.configure_hip_runtime()
from gill_amd import _native as N, synth   # noqa: E402

torch.set_num_threads(synth.host_cores())
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
sha = hashlib.sha256()
lib, stream = N.lib(), N.current_stream()


def feed(*tensors):
  torch.cuda.synchronize()
  for t in tensors:
    t = t.detach().cpu().contiguous()
    assert t.dtype in (torch.int32, torch.int64) or bool(torch.isfinite(t.float()).all()), case
    sha.update(t.view(torch.uint8).numpy().tobytes())


def new(*shape, dt=torch.float32):
  return torch.zeros(shape, device=dev, dtype=dt)


def opt_handle(geo, mode, max_batch, max_seq):
  import kv_cache_util as U
  cfg, seed = U.GEOMETRIES[geo]["cfg"], U.GEOMETRIES[geo]["seed"]
  sd = U.peaked_opt_state_dict(cfg, seed)
  c = N.gill_opt_config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                        ffn_dim=cfg.ffn_dim, max_positions=cfg.max_positions, max_batch=max_batch, max_seq=max_seq)
  arr, keep = N.make_tensor_table(sd, dev)
  h = C.c_void_p()
  N.check(lib.gill_opt_create_ex(C.byref(h), C.byref(c), arr, len(keep), mode))
  del keep
  return h, cfg, sd


def ids_of(cfg, B, T, seed):
  return synth.synthetic_prompt_ids(16, T, seed=seed, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:B, :T].contiguous()


def run_forward(geo, cached):
  import kv_cache_util as U
  h, cfg, sd = opt_handle(geo, 0, 2, 64)
  B, T, D = 2, 30 + (3 if cached else 0), cfg.hidden_size
  x = U.token_embeds(sd, cfg, B, T, 5).to(dev, torch.bfloat16)
  if not cached:
    out = new(B, T, D)
    N.check(lib.gill_opt_forward(h, N.ptr(x), B, T, N.ptr(out), stream))
    return feed(out)
  past = 0
  for tn in (17, 13, 1, 1, 1):
    xs, out = x[:, past:past + tn].contiguous(), new(B, tn, D)
    N.check(lib.gill_opt_forward_cached(h, N.ptr(xs), B, tn, past, N.ptr(out), stream))
    feed(out)
    past += tn


def run_w8_cached(geo):
  import kv_cache_util as U
  h, cfg, sd = opt_handle(geo, 1, 8, 64)
  D = cfg.hidden_size
  x = U.token_embeds(sd, cfg, 8, 56, 6).to(dev, torch.bfloat16)
  past = 0
  for B, tn in ((2, 30), (2, 1), (2, 1), (2, 1), (2, 8), (2, 1), (2, 1), (1, 1), (8, 1), (3, 8)):
    assert lib.gill_opt_cached_uses_w8(h, B, tn, past) == int(past > 0 and B * tn <= 16)
    xs, out = x[:B, past:past + tn].contiguous(), new(B, tn, D)
    N.check(lib.gill_opt_forward_cached(h, N.ptr(xs), B, tn, past, N.ptr(out), stream))
    feed(out)
    past += tn


def hidden_inputs(cfg, with_extra):
  """ids (2, 24) holding an id past the top of the vocabulary and, with extra rows, visual rows and one past the top of that table;
  without them a negative id (row 0 of the vocabulary)."""
  B, T, D = 2, 24, cfg.hidden_size
  ids = ids_of(cfg, B, T, 9).clone()
  ids[0, 5] = cfg.vocab_size + 7
  extra = None
  if with_extra:
    extra = synth.normal("digest_extra", (3, D), 7, 0.5).to(dev, torch.bfloat16)
    ids[1, 2], ids[1, 3], ids[0, 9], ids[1, 11] = -2, -1, -3, -9
  else:
    ids[1, 4] = -5
  return B, T, ids.to(dev), extra, (C.c_int32 * B)(T - 1, 15)


def run_img(geo, with_extra):
  h, cfg, _ = opt_handle(geo, 0, 2, 32)
  B, T, ids, extra, last = hidden_inputs(cfg, with_extra)
  raw, emb = new(B, 8, cfg.hidden_size, dt=torch.bfloat16), new(B, 8, cfg.hidden_size, dt=torch.bfloat16)
  N.check(lib.gill_opt_img_hidden_ex(h, N.ptr(ids), last, B, T, 8, N.ptr(extra), 0 if extra is None else extra.shape[0], N.ptr(raw), N.ptr(emb),
                                     stream))
  feed(raw, emb)


def run_loss(geo, every):
  h, cfg, _ = opt_handle(geo, 0, 2, 32)
  B, T, ids, extra, last = hidden_inputs(cfg, True)
  D, V = cfg.hidden_size, cfg.vocab_size
  labels = ids.clamp(0, V - 1)
  labels[ids < 0] = -100
  labels[0, :3] = -100
  tl, tr, summ = new(B, T - 1), new(B, T - 1, dt=torch.int32), new(4)
  opt = [new(B, 8, D, dt=torch.bfloat16), new(B, 8, D, dt=torch.bfloat16), new(B, V), new(B, T, D)] if every else [None] * 4
  N.check(lib.gill_opt_forward_loss(h, N.ptr(ids), last if every else None, B, T, 8, N.ptr(extra), extra.shape[0], N.ptr(labels), N.ptr(opt[0]),
                                    N.ptr(opt[1]), N.ptr(tl), N.ptr(tr), N.ptr(summ), N.ptr(opt[2]), N.ptr(opt[3]), stream))
  feed(tl, tr, summ, *[t for t in opt if t is not None])


def run_decode(geo, mode, B):
  max_seq, steps = 48, 4
  h, cfg, sd = opt_handle(geo, mode, B, max_seq)
  lengths = [(30, 23, 9), (5, 31, 12, 26, 8, 19, 29, 15, 22, 17, 3, 28, 11, 24, 7, 20, 14)][B > 3][:B]
  Tmax, D = max(lengths), cfg.hidden_size
  # right-padded prompts (the pad positions hold other real tokens) and every row's own continuation
  seqs = synth.synthetic_prompt_ids(B, Tmax + steps, seed=13, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:, :Tmax + steps]
  prompt_ids = seqs[:, :Tmax].contiguous()
  step_ids = torch.stack([seqs[b, n:n + steps] for b, n in enumerate(lengths)])
  table = sd["model.decoder.embed_tokens.weight"]
  hid = new(B, Tmax, D)
  N.check(lib.gill_opt_prefill_ids(h, N.ptr(prompt_ids.to(dev)), B, Tmax, None, 0, N.ptr(hid), stream))
  feed(*[hid[b, :n] for b, n in enumerate(lengths)])
  for s in range(steps):
    lens = [n + s for n in lengths]
    if s == steps - 1:
      lens[0] = 4000      # beyond the cache: clamped and flagged; the host's bound stays inside
    x = table[step_ids[:, s]].to(dev, torch.bfloat16).contiguous()
    ld, out = torch.tensor(lens, dtype=torch.int32, device=dev), new(B, D)
    N.check(lib.gill_opt_decode_step(h, N.ptr(x), N.ptr(ld), B, Tmax + steps, N.ptr(out), stream))
    feed(out)
  # the flags the steps raised, as the ragged decision folds them into the rows' state
  rule = N.gill_decode_rule()
  rule.filter_value = float("-inf")
  rule.ret_scale = rule.gen_scale = 1.0
  logits, state = new(B, cfg.vocab_size), new(6 * B + 1, dt=torch.int32)
  toks, nxt = new(B, 4, dt=torch.int64), new(B, D, dt=torch.bfloat16)
  N.check(lib.gill_opt_pick_token_ragged(h, N.ptr(logits), B, C.byref(rule), 4, None, N.ptr(state), N.ptr(toks), 4, N.ptr(nxt), stream))
  feed(state, toks)
  assert state[5 * B:6 * B].cpu().tolist() == [2] + [0] * (B - 1), "the clamp of row 0 is not in the flags"


def run_mapper():
  from gill_amd.layers import TextFcLayer
  msd = {k: v.bfloat16().float() for k, v in synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=1).items()}
  layer = TextFcLayer(768, 768, num_input_tokens=8, num_output_tokens=77, mode="gill_mapper")
  layer.load_state_dict(msd, strict=True)
  x, e = synth.normal("digest_x", (2, 8, 768), 1).bfloat16().float(), synth.normal("digest_e", (1, 8, 768), 1).bfloat16().float()
  feed(layer.to(dev)(x.to(dev), e.to(dev)).float())


def run_clip_vision():
  cfg = synth.ClipConfig.tiny()
  sd = {k: v.bfloat16().float() for k, v in synth.clip_state_dict(cfg, seed=5).items()}
  c = N.gill_clip_config(image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers,
                         num_heads=cfg.num_heads, intermediate_size=cfg.intermediate_size, max_batch=4)
  arr, keep = N.make_tensor_table(sd, dev)
  h = C.c_void_p()
  N.check(lib.gill_clip_create(C.byref(h), C.byref(c), arr, len(keep)))
  px, pooled = synth.normal("digest_px", (3, 3, cfg.image_size, cfg.image_size), 3).to(dev), new(3, cfg.hidden_size)
  N.check(lib.gill_clip_forward(h, N.ptr(px), 3, N.ptr(pooled), stream))
  feed(pooled)


def run_clip_text():
  from gill_amd.clip_text import GillClipTextEncoder
  cfg = synth.ClipTextConfig.tiny()
  sd = {k: v.bfloat16().float() for k, v in synth.clip_text_state_dict(cfg, seed=11).items()}
  ids = synth.synthetic_prompt_ids(3, 33, seed=4, vocab_lo=1, vocab_hi=cfg.vocab_size - 1)[:3, :33]
  feed(*GillClipTextEncoder(sd, cfg, dev, max_batch=4)(ids, both=True))


parts = case.split("-")
if parts[0] in ("forward", "cached"):
  run_forward(parts[1], parts[0] == "cached")
elif parts[0] in ("img", "imgx"):
  run_img(parts[1], parts[0] == "imgx")
elif parts[0] in ("loss", "loss0"):
  run_loss(parts[1], parts[0] == "loss")
elif parts[0] == "w8cached":
  run_w8_cached(parts[1])
elif parts[0] in ("dec", "w8"):
  run_decode(parts[1], 1 if parts[0] == "w8" else 0, int(parts[2][1:]))
else:
  {"mapper": run_mapper, "clipvision": run_clip_vision, "cliptext": run_clip_text}[case]()
print(case, sha.hexdigest(), flush=True)
