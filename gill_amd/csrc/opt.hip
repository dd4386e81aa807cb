// Stage 1 — frozen OPT decoder (transformers OPTForCausalLM as called at gill/models.py:363-365 and :465).
//
// Pre-LN decoder layer (do_layer_norm_before=True: every OPT size but 350m):
//   h += out_proj(causal_attn(q,k,v = *_proj(LN(h))))         q scaled by head_dim^-0.5
//   h += fc2(relu(fc1(LN(h))))
// learned positions with the +2 offset, final LayerNorm; hidden_states[-1] is post-final-LN.
// The residual stream is fp32; GEMMs are bf16 MFMA with fp32 accumulation, split-K so that the
// skinny (M = B*T) weight-streaming GEMMs cover all 256 CUs; attention is the shared flash kernel.
// Every layer loop — forward, cached forward, the ragged decode step on bf16 weights or e4m3 bytes, the packed extend pass of a dialogue
// session and the candidate-scoring pass over the same cache — is TfmRun::layers of tfm.h; here: embeddings and positions, the KV cache, the
// hidden-rows pass of img_hidden / forward_loss, logits and the decode, extend and score-candidates entry points.
#include "tfm.h"
#include "philox.h"

struct gill_opt {
  gill_opt_config cfg;
  int weight_mode = 0;          // GILL_OPT_BF16 / GILL_OPT_W8 (gill_opt_create_ex)
  DevPool pool;
  bf16_t* embed = nullptr;      // [vocab][D]
  bf16_t* lm_head = nullptr;    // tied to embed unless lm_head.weight was supplied
  bf16_t* pos = nullptr;        // [max_positions+2][D]
  float *lnfg = nullptr, *lnfb = nullptr;
  std::vector<TfmLayer> layers;
  Tfm tfm;
  // workspace
  float* h = nullptr;       // [B*T][D]
  bf16_t* emb_tmp = nullptr;  // [B*T][D]
  float* gath = nullptr;      // [B*8][D]
  bf16_t* last_bf = nullptr;  // [8][D]
  int32_t* idx_dev = nullptr; // [B*8 + B*8]
  // KV cache of gill_opt_forward_cached (allocated at its first call): per layer K [B][H][Tcap][dp], Vt [B][H][dpv][Tcap]
  std::vector<TfmKv> cache;
  int kv_format = GILL_KV_BF16;   // gill_opt_set_kv_format: GILL_KV_E4M3 = per layer K8 / Vt8 bytes and Kexp / Vexp [B][H][Tcap] (attention_kv8_dev.h)
  int32_t* dec_flags = nullptr;   // [max_batch]: length clamps of gill_opt_decode_step's attention, folded into the rows' flags by the ragged decision
  int32_t* cached_lens = nullptr; // [max_batch]: past_len per row, filled on the stream by gill_opt_forward_cached where it runs on the e4m3 bytes
  // workspace of gill_opt_extend (allocated at its first call): the packed [B*T][3D] projection and the last new row of every sequence
  bf16_t* ext_qkv = nullptr;
  float* ext_last = nullptr;      // [max_batch][D]
  // workspace of the fork attention under gill_opt_score_candidates (attention_fork_ws_bytes; grown at a call that needs more)
  void* fork_ws = nullptr; size_t fork_ws_bytes = 0;
  // branch cache of gill_opt_decode_step_branch (gill_opt_branch_reserve): one slab, per layer Kb [br_rows][H][bpitch][dp] and
  // Vtb [br_rows][H][dpv][bpitch] (TfmKv::pad = bpitch), then br_flags [br_rows]: the clamps of the branch attention, folded into the
  // branches' flags by gill_opt_next_token_branch.  Not in the pool: a larger request frees and reallocates it
  std::vector<TfmKv> br_cache;
  void* br_slab = nullptr; size_t br_bytes = 0; int br_rows = 0;
  int32_t* br_flags = nullptr;
  ~gill_opt() { if (br_slab) (void)hipFree(br_slab); }
  // scoring workspace of gill_opt_forward_loss (allocated at its first call): the final LayerNorm of every row, the shifted targets, the
  // per-row results and the partials of lmloss.hip
  bf16_t* xn_bf = nullptr;      // [B*T][D]
  int64_t* loss_tgt = nullptr;  // [B*T]
  float *loss_lse = nullptr, *loss_tl = nullptr;   // [B*T]
  int* loss_rank = nullptr;     // [B*T]
  void* loss_ws = nullptr;
  float* ll_f32 = nullptr;      // [B][D]: the rows of last_logit_out after the final LayerNorm
  // layers over the fp32 stream h (B*T rows): ReLU, causal.  past < 0: plain forward over T tokens.  past >= 0: the T rows are
  // the tokens past .. past+T-1 of each sequence; their K/V are appended to the cache and they attend to it.  dec: the decode step, every
  // row's T tokens at its own device length (T == 1: the ragged step); w8: on the e4m3 bytes (the caller's gill_opt_*_uses_w8() says so).
  int run_layers(int B, int T, hipStream_t s, int past = -1, const TfmDecode* dec = nullptr, bool w8 = false) const {
    return TfmRun{tfm, s, w8}.layers(h, layers.data(), (int)layers.size(), B, T, ACT_RELU, true, past >= 0 ? cache.data() : nullptr,
                                     past >= 0 ? past : 0, dec);
  }
};

// h[row][:] = bf16->f32(emb[row][:]) + bf16->f32(pos[p][:]), p = pos_offset + row % T, or with lens (one token per row, the decode step)
// 2 + lens[row], the length read on the device and clamped into the table (the attention kernel of the same step raises the flag).
// 16-byte loads, 8 elements per thread (D % 64 == 0).
__global__ __launch_bounds__(256) void opt_add_pos_kernel(const bf16_t* __restrict__ emb, const bf16_t* __restrict__ pos,
                                                          const int32_t* __restrict__ lens, int max_positions, int pos_offset, int T, int D,
                                                          float* __restrict__ out) {
  const int row = blockIdx.x;
  int p = pos_offset + row % T;
  if (lens) {
    const int n = lens[row];
    p = 2 + (n < 0 ? 0 : (n > max_positions - 1 ? max_positions - 1 : n));
  }
  const bf16_t* e = emb + (size_t)row * D;
  const bf16_t* pe = pos + (size_t)p * D;
  float* o = out + (size_t)row * D;
  for (int c = threadIdx.x * 8; c < D; c += blockDim.x * 8) {
    const uint4 u = *reinterpret_cast<const uint4*>(e + c);
    const uint4 v = *reinterpret_cast<const uint4*>(pe + c);
    const uint32_t uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
    float r[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r[2 * i] = bf2f((bf16_t)(uu[i] & 0xffff)) + bf2f((bf16_t)(vv[i] & 0xffff));
      r[2 * i + 1] = bf2f((bf16_t)(uu[i] >> 16)) + bf2f((bf16_t)(vv[i] >> 16));
    }
    *reinterpret_cast<float4*>(o + c) = make_float4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<float4*>(o + c + 4) = make_float4(r[4], r[5], r[6], r[7]);
  }
}
static int opt_add_pos(const gill_opt* m, const void* emb_bf16, const int32_t* lens, int rows, int T, int pos_offset, hipStream_t s) {
  hipLaunchKernelGGL(opt_add_pos_kernel, dim3(rows), dim3(256), 0, s, (const bf16_t*)emb_bf16, m->pos, lens, m->cfg.max_positions, pos_offset, T,
                     m->cfg.hidden_size, m->h);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gill_opt_create(gill_opt** out, const gill_opt_config* cfg, const gill_tensor* weights, int n_weights) {
  return gill_opt_create_ex(out, cfg, weights, n_weights, GILL_OPT_BF16);
}

extern "C" int gill_opt_weight_mode(const gill_opt* m) { return m ? m->weight_mode : -1; }

// the decode step's branch, and the host-only query of it
extern "C" int gill_opt_decode_uses_w8(const gill_opt* m, int B) {
  return m && m->weight_mode == GILL_OPT_W8 && B >= 1 && B <= W8_MAX_ROWS ? 1 : 0;
}

// the cached forward's branch, and the host-only query of it
extern "C" int gill_opt_cached_uses_w8(const gill_opt* m, int B, int T_new, int past_len) {
  return m && m->weight_mode == GILL_OPT_W8 && past_len > 0 && B >= 1 && T_new >= 1 && (int64_t)B * T_new <= W8_MAX_ROWS ? 1 : 0;
}

extern "C" int gill_w8_max_rows(void) { return W8_MAX_ROWS; }

extern "C" int gill_opt_create_ex(gill_opt** out, const gill_opt_config* cfg, const gill_tensor* weights, int n_weights, int weight_mode) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  GILL_REQUIRE(weight_mode == GILL_OPT_BF16 || weight_mode == GILL_OPT_W8, "weight_mode is GILL_OPT_BF16 or GILL_OPT_W8");
  const int D = cfg->hidden_size, F = cfg->ffn_dim, H = cfg->num_heads;
  GILL_REQUIRE(D % 64 == 0 && F % 64 == 0 && H > 0 && D % H == 0, "OPT dims must be multiples of 64");
  const int hd = D / H;
  GILL_REQUIRE(attn_padded_dim(hd) == hd, "OPT head dim must be one of 48/64/80/128/160");
  GILL_REQUIRE(cfg->max_batch > 0 && cfg->max_seq > 0 && cfg->max_seq <= cfg->max_positions, "bad workspace sizing");
  gill_opt* m = new gill_opt();
  m->cfg = *cfg;
  m->weight_mode = weight_mode;
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  const std::string dec = "model.decoder.";
  if ((rc = load_bf16(wt, m->pool, dec + "embed_tokens.weight", (int64_t)cfg->vocab_size * D, &m->embed, s))) return fail(rc);
  if ((rc = load_bf16(wt, m->pool, dec + "embed_positions.weight", (int64_t)(cfg->max_positions + 2) * D, &m->pos, s)))
    return fail(rc);
  if (wt.find("lm_head.weight")) {
    if ((rc = load_bf16(wt, m->pool, "lm_head.weight", (int64_t)cfg->vocab_size * D, &m->lm_head, s))) return fail(rc);
  } else {
    m->lm_head = m->embed;
  }
  if ((rc = load_f32(wt, m->pool, dec + "final_layer_norm.weight", D, &m->lnfg, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, dec + "final_layer_norm.bias", D, &m->lnfb, s))) return fail(rc);
  m->layers.resize(cfg->num_layers);
  const TfmNames names = {{"self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj."}, "self_attn.out_proj.", "fc1.", "fc2.",
                          "self_attn_layer_norm.", "final_layer_norm."};
  // stream64: the skinny (M = B*T) GEMMs stream their weights; the blocked layout is what the STREAM64 kernel reads
  for (int i = 0; i < cfg->num_layers; ++i)
    if ((rc = tfm_load_layer(wt, m->pool, dec + "layers." + std::to_string(i) + ".", names, D, F, true, &m->layers[i], s))) return fail(rc);
  // w8: the four matrices of every layer also as e4m3 bytes + power-of-two row scales (the decode step's operands), the bf16 copies
  // replaced by the dequantised values (every other entry point: the same model on today's kernels)
  if (weight_mode == GILL_OPT_W8)
    for (int i = 0; i < cfg->num_layers; ++i)
      if ((rc = tfm_quantize_layer_w8(m->pool, &m->layers[i], s))) return fail(rc);
  const size_t R = (size_t)cfg->max_batch * cfg->max_seq;
  if ((rc = m->pool.alloc(&m->h, R * D))) return fail(rc);
  if ((rc = m->tfm.alloc(m->pool, cfg->max_batch, cfg->max_seq, D, F, H, hd, round_up(hd, 32)))) return fail(rc);
  // the reducer of out_proj / fc2 also runs the LayerNorm that follows (profiles/r05_opt_stream64.md: 11 -> 7 launches per layer)
  m->tfm.fuse_ln = true;
  if ((rc = m->pool.alloc(&m->emb_tmp, R * D))) return fail(rc);
  if ((rc = m->pool.alloc(&m->gath, (size_t)cfg->max_batch * 64 * D))) return fail(rc);
  if ((rc = m->pool.alloc(&m->last_bf, (size_t)8 * D))) return fail(rc);
  if ((rc = m->pool.alloc(&m->idx_dev, (size_t)cfg->max_batch * 64 * 2))) return fail(rc);
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("opt create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_opt_destroy(gill_opt* h) { delete h; }

extern "C" int gill_opt_embed(gill_opt* m, const int64_t* ids, int n, void* out_bf16, void* stream) {
  GILL_REQUIRE(m && ids && out_bf16 && n > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  // embedding rows are bf16 already: the lookup is a pure row copy (no allocation, no sync: both pointers are the caller's
  // device memory and the call is stream-ordered like every other entry point)
  GILL_TRY(embed_rows_bf16_launch(ids, m->embed, m->cfg.vocab_size, n, m->cfg.hidden_size, (bf16_t*)out_bf16, s));
  return 0;
}

extern "C" int gill_opt_forward(gill_opt* m, const void* inputs_embeds_bf16, int B, int T, float* hidden_out,
                                void* stream) {
  GILL_REQUIRE(m && inputs_embeds_bf16, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch && T >= 1 && T <= m->cfg.max_seq, "B/T exceed the handle's workspace");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size;
  GILL_TRY(opt_add_pos(m, inputs_embeds_bf16, nullptr, B * T, T, 2, s));
  GILL_TRY(m->run_layers(B, T, s));
  if (hidden_out) GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_out, B * T, D, 1e-5f, s));
  return 0;
}

// the KV cache of the cached entries, allocated at the first call that needs it
static int opt_ensure_cache(gill_opt* m) {
  if (!m->cache.empty()) return 0;
  // zero-filled: rows beyond the valid length are masked in attention, but must stay finite (0 * NaN would poison PV)
  const int tcap = round_up(m->cfg.max_seq, 32);
  const size_t kn = (size_t)m->cfg.max_batch * m->cfg.num_heads * tcap * m->tfm.dp;
  const size_t vn = (size_t)m->cfg.max_batch * m->cfg.num_heads * m->tfm.dpv * tcap;
  m->cache.assign(m->layers.size(), TfmKv{nullptr, nullptr, tcap});
  for (TfmKv& c : m->cache) {
    c.fmt = m->kv_format;
    if (m->kv_format == GILL_KV_E4M3) {     // zero bytes are zero codes, zero exponents a scale of 1
      GILL_TRY(m->pool.alloc(&c.k8, kn, true));
      GILL_TRY(m->pool.alloc(&c.vt8, vn, true));
      GILL_TRY(m->pool.alloc(&c.kexp, kn / m->tfm.dp, true));
      GILL_TRY(m->pool.alloc(&c.vexp, kn / m->tfm.dp, true));
    } else {
      GILL_TRY(m->pool.alloc(&c.k, kn, true));
      GILL_TRY(m->pool.alloc(&c.vt, vn, true));
    }
  }
  GILL_TRY(m->pool.alloc(&m->cached_lens, (size_t)m->cfg.max_batch, true));
  return m->pool.alloc(&m->dec_flags, (size_t)m->cfg.max_batch, true);
}

extern "C" int gill_opt_set_kv_format(gill_opt* m, int fmt) {
  GILL_REQUIRE(m, "null handle");
  GILL_REQUIRE(fmt == GILL_KV_BF16 || fmt == GILL_KV_E4M3, "kv format is GILL_KV_BF16 or GILL_KV_E4M3");
  GILL_REQUIRE(m->cache.empty() || fmt == m->kv_format, "the KV cache is allocated: its format can no longer change");
  if (fmt == GILL_KV_E4M3) {
    const int dp = m->tfm.dp;
    GILL_REQUIRE(dp == 64 || dp == 80 || dp == 128, "an e4m3 KV cache needs a head dim of 64, 80 or 128");
  }
  m->kv_format = fmt;
  return 0;
}

extern "C" int gill_opt_kv_format(const gill_opt* m) { return m ? m->kv_format : -1; }

extern "C" int64_t gill_opt_kv_bytes(const gill_opt* m) {
  if (!m || m->cache.empty()) return 0;
  const int64_t slots = (int64_t)m->layers.size() * m->cfg.max_batch * m->cfg.num_heads * m->cache[0].pad;
  return slots * (m->kv_format == GILL_KV_E4M3 ? m->tfm.dp + m->tfm.dpv + 2 : 2 * (m->tfm.dp + m->tfm.dpv));
}

// the entries whose flash kernel writes and reads a bf16 cache
#define OPT_REQUIRE_BF16_CACHE(m, what) \
  GILL_REQUIRE((m)->kv_format == GILL_KV_BF16, what ": the handle's KV cache format is e4m3 (GILL_KV_E4M3); prefill through gill_opt_extend at lengths 0")

__global__ void opt_fill_lens_kernel(int32_t* __restrict__ lens, int B, int v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) lens[i] = v;
}

extern "C" int gill_opt_forward_cached(gill_opt* m, const void* inputs_embeds_bf16, int B, int T_new, int past_len,
                                       float* hidden_out, void* stream) {
  GILL_REQUIRE(m && inputs_embeds_bf16 && hidden_out, "null argument");
  OPT_REQUIRE_BF16_CACHE(m, "gill_opt_forward_cached");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch && T_new >= 1 && past_len >= 0 && past_len + T_new <= m->cfg.max_seq,
               "B / past_len + T_new exceed the handle's workspace");
  GILL_REQUIRE(past_len + T_new + 2 <= m->cfg.max_positions + 2, "sequence longer than the position table");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size;
  GILL_TRY(opt_ensure_cache(m));
  GILL_TRY(opt_add_pos(m, inputs_embeds_bf16, nullptr, B * T_new, T_new, 2 + past_len, s));
  if (gill_opt_cached_uses_w8(m, B, T_new, past_len)) {
    // at most 16 rows on a w8 handle: the decode mode of the layer loop on the e4m3 bytes, every row at length past_len (checked above against
    // max_seq <= the cache pitch: no clamp can occur, so no flags)
    hipLaunchKernelGGL(opt_fill_lens_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, m->cached_lens, B, past_len);
    GILL_CHECK_HIP(hipGetLastError());
    const TfmDecode dec{m->cached_lens, nullptr};
    GILL_TRY(m->run_layers(B, T_new, s, 0, &dec, true));
  } else {
    GILL_TRY(m->run_layers(B, T_new, s, past_len));
  }
  GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_out, B * T_new, D, 1e-5f, s));
  return 0;
}

// The pass gill_opt_img_hidden_ex and gill_opt_forward_loss share: the gather indices (rows: the num_tokens rows ending at last_idx, slots
// [0, B * num_tokens) of idx_dev; last_logit: the rows last_idx - 1, slots [max_batch * 64, + B)) checked and uploaded, the bf16 embedding rows
// (-> emb_out), embeddings + learned positions -> the fp32 stream, the layers, and the final LayerNorm of the gathered rows -> raw_out.
static int opt_hidden_rows(gill_opt* m, const int64_t* ids, const int32_t* last_idx_host, int B, int T, int num_tokens, const void* extra_rows_bf16,
                           int n_extra, void* raw_out_bf16, void* emb_out_bf16, bool last_logit, hipStream_t s) {
  const int D = m->cfg.hidden_size, V = m->cfg.vocab_size, ll_base = m->cfg.max_batch * 64;
  const bf16_t* extra = (const bf16_t*)extra_rows_bf16;
  const bool rows = raw_out_bf16 || emb_out_bf16;
  if (rows || last_logit) {
    std::vector<int32_t> idx(last_logit ? (size_t)ll_base + B : (size_t)B * num_tokens, 0);
    for (int b = 0; b < B; ++b) {
      if (rows) {
        GILL_REQUIRE(last_idx_host[b] - num_tokens + 1 >= 0 && last_idx_host[b] < T, "last_idx out of range");
        for (int j = 0; j < num_tokens; ++j) idx[(size_t)b * num_tokens + j] = b * T + last_idx_host[b] - num_tokens + 1 + j;
      }
      if (last_logit) {
        GILL_REQUIRE(last_idx_host[b] - 1 >= 0 && last_idx_host[b] - 1 < T, "last_idx - 1 out of range");
        idx[(size_t)ll_base + b] = b * T + last_idx_host[b] - 1;
      }
    }
    GILL_CHECK_HIP(hipMemcpyAsync(m->idx_dev, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, s));
    GILL_CHECK_HIP(hipStreamSynchronize(s));  // idx is a stack-lifetime host buffer
  }
  // input_embs = input_embeddings(labels)  (models.py:180), bf16 rows
  GILL_TRY(embed_tokens_launch(ids, m->embed, V, extra, n_extra, nullptr, 2, B, T, D, m->h, s));
  GILL_TRY(cast_f32_to_bf16_launch(m->h, m->emb_tmp, (int64_t)B * T * D, s));
  if (emb_out_bf16) GILL_TRY(gather_rows_launch(m->emb_tmp, 0, m->idx_dev, B * num_tokens, D, emb_out_bf16, 0, s));
  // + learned positions -> fp32 stream
  GILL_TRY(embed_tokens_launch(ids, m->embed, V, extra, n_extra, m->pos, 2, B, T, D, m->h, s));
  GILL_TRY(m->run_layers(B, T, s));
  if (raw_out_bf16) {      // final LN only on the rows that are read (models.py:384)
    GILL_TRY(gather_rows_launch(m->h, 1, m->idx_dev, B * num_tokens, D, m->gath, 1, s));
    GILL_TRY(layernorm_launch(m->gath, 1, m->lnfg, m->lnfb, (bf16_t*)raw_out_bf16, B * num_tokens, D, 1e-5f, s));
  }
  return 0;
}

extern "C" int gill_opt_img_hidden_ex(gill_opt* m, const int64_t* ids, const int32_t* last_idx_host, int B, int T, int num_tokens,
                                      const void* extra_rows_bf16, int n_extra, void* raw_out_bf16, void* emb_out_bf16, void* stream) {
  GILL_REQUIRE(m && ids && last_idx_host && raw_out_bf16, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch && T >= 1 && T <= m->cfg.max_seq, "B/T exceed the handle's workspace");
  GILL_REQUIRE(num_tokens >= 1 && num_tokens <= 64, "num_tokens out of range");
  GILL_REQUIRE(n_extra >= 0 && (n_extra == 0 || extra_rows_bf16), "n_extra rows need a table");
  return opt_hidden_rows(m, ids, last_idx_host, B, T, num_tokens, extra_rows_bf16, n_extra, raw_out_bf16, emb_out_bf16, false, (hipStream_t)stream);
}

extern "C" int gill_opt_img_hidden(gill_opt* m, const int64_t* ids, const int32_t* last_idx_host, int B, int T,
                                   int num_tokens, void* raw_out_bf16, void* emb_out_bf16, void* stream) {
  return gill_opt_img_hidden_ex(m, ids, last_idx_host, B, T, num_tokens, nullptr, 0, raw_out_bf16, emb_out_bf16, stream);
}

extern "C" int gill_opt_last_logits(gill_opt* m, const float* hidden, int B, int T, float* logits_out, void* stream) {
  GILL_REQUIRE(m && hidden && logits_out, "null argument");
  GILL_REQUIRE(B >= 1 && T >= 1, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size, V = m->cfg.vocab_size;
  // the GEMV takes 8 rows per launch (last_bf holds 8); its rows are independent, so chunking leaves every row's bits as they are
  for (int b0 = 0; b0 < B; b0 += 8) {
    const int nb = B - b0 < 8 ? B - b0 : 8;
    for (int b = 0; b < nb; ++b)
      GILL_TRY(cast_f32_to_bf16_launch(hidden + ((size_t)(b0 + b) * T + (T - 1)) * D, m->last_bf + (size_t)b * D, D, s));
    GILL_TRY(skinny_gemm_launch(m->last_bf, m->lm_head, nb, V, D, logits_out + (size_t)b0 * V, s));
  }
  return 0;
}

// target[b][t] = labels[b][t + 1] for t < T - 1, -100 for the last position (HF shifts the labels; no labels: nothing is scored)
__global__ __launch_bounds__(256) void opt_shift_labels_kernel(const int64_t* __restrict__ labels, int n, int T, int64_t* __restrict__ target) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  target[i] = (labels && (i % T) < T - 1) ? labels[i + 1] : (int64_t)-100;
}

// (B, T) per-row results -> (B, T - 1) token_loss = lse - tgt (0 where ignored) and token_rank
__global__ __launch_bounds__(256) void opt_token_loss_kernel(const float* __restrict__ lse, const float* __restrict__ tgt, const int* __restrict__ rank,
                                                             int B, int T, float* __restrict__ token_loss, int32_t* __restrict__ token_rank) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * (T - 1)) return;
  const int b = i / (T - 1), t = i - b * (T - 1);
  const int r = b * T + t;
  token_loss[i] = lse[r] - tgt[r];
  token_rank[i] = rank[r];
}

// the scoring workspace of gill_opt_forward_loss and gill_opt_score_candidates, allocated at the first call of either
static int opt_ensure_loss_ws(gill_opt* m) {
  if (m->xn_bf) return 0;
  const int D = m->cfg.hidden_size, V = m->cfg.vocab_size;
  const size_t R = (size_t)m->cfg.max_batch * m->cfg.max_seq;
  GILL_TRY(m->pool.alloc(&m->xn_bf, R * D));
  GILL_TRY(m->pool.alloc(&m->loss_tgt, R));
  GILL_TRY(m->pool.alloc(&m->loss_lse, R));
  GILL_TRY(m->pool.alloc(&m->loss_tl, R));
  GILL_TRY(m->pool.alloc(&m->loss_rank, R));
  GILL_TRY(m->pool.alloc(&m->ll_f32, (size_t)m->cfg.max_batch * D));
  unsigned char* ws = nullptr;
  GILL_TRY(m->pool.alloc(&ws, lm_loss_workspace_bytes((int)R, V), false));
  m->loss_ws = ws;
  return 0;
}

extern "C" int gill_opt_forward_loss(gill_opt* m, const int64_t* ids, const int32_t* last_idx_host, int B, int T, int num_tokens,
                                     const void* extra_rows_bf16, int n_extra, const int64_t* labels, void* raw_out_bf16, void* emb_out_bf16,
                                     float* token_loss, int32_t* token_rank, float* summary, float* last_logit_out, float* hidden_out,
                                     void* stream) {
  GILL_REQUIRE(m && ids && token_loss && token_rank && summary, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch && T >= 2 && T <= m->cfg.max_seq, "B/T exceed the handle's workspace (T >= 2)");
  GILL_REQUIRE(n_extra >= 0 && (n_extra == 0 || extra_rows_bf16), "n_extra rows need a table");
  const bool rows = raw_out_bf16 || emb_out_bf16;
  GILL_REQUIRE(last_idx_host || !(rows || last_logit_out), "raw_out / emb_out / last_logit_out need last_idx");
  GILL_REQUIRE(!rows || (num_tokens >= 1 && num_tokens <= 64), "num_tokens out of range");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size, V = m->cfg.vocab_size;
  const int ll_base = m->cfg.max_batch * 64;      // idx_dev: the last-logit rows (opt_hidden_rows)
  GILL_TRY(opt_ensure_loss_ws(m));
  GILL_TRY(opt_hidden_rows(m, ids, last_idx_host, B, T, num_tokens, extra_rows_bf16, n_extra, raw_out_bf16, emb_out_bf16, last_logit_out != nullptr, s));
  // here the final LayerNorm runs on every row
  GILL_TRY(layernorm_launch(m->h, 1, m->lnfg, m->lnfb, m->xn_bf, B * T, D, 1e-5f, s));
  if (hidden_out) GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_out, B * T, D, 1e-5f, s));
  if (last_logit_out) {
    // gill_opt_last_logits on the rows last_idx - 1: fp32 LayerNorm rows -> bf16 -> the GEMV, 8 rows at a time
    GILL_TRY(gather_rows_launch(m->h, 1, m->idx_dev + ll_base, B, D, m->gath, 1, s));
    GILL_TRY(layernorm_f32out_launch(m->gath, 1, m->lnfg, m->lnfb, m->ll_f32, B, D, 1e-5f, s));
    GILL_TRY(gill_opt_last_logits(m, m->ll_f32, B, 1, last_logit_out, stream));
  }
  const int n = B * T;
  hipLaunchKernelGGL(opt_shift_labels_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, labels, n, T, m->loss_tgt);
  GILL_CHECK_HIP(hipGetLastError());
  GILL_TRY(lm_loss_launch(m->xn_bf, m->lm_head, m->loss_tgt, n, V, D, m->loss_lse, m->loss_tl, m->loss_rank, summary, m->loss_ws, s));
  hipLaunchKernelGGL(opt_token_loss_kernel, dim3(cdiv(B * (T - 1), 256)), dim3(256), 0, s, m->loss_lse, m->loss_tl, m->loss_rank, B, T, token_loss,
                     token_rank);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

// gill_decode_rule -> the kernel's form: ids normalised and range-checked like a torch index, the conditions of :478-489
// evaluated once (the scale tests in double precision, as Python compares the floats)
static int resolve_rule(const gill_opt* m, const gill_decode_rule* rule, DecodeRuleDev* r) {
  GILL_REQUIRE(rule, "null rule");
  GILL_REQUIRE(rule->n_ret >= 0 && rule->n_ret <= kDecodeMaxIds && rule->n_gen >= 0 && rule->n_gen <= kDecodeMaxIds,
               "rule: at most 16 retrieval / generation ids");
  const int V = m->cfg.vocab_size;
  *r = DecodeRuleDev{};
  r->vocab = V;
  r->n_ret = rule->n_ret;
  r->n_gen = rule->n_gen;
  for (int j = 0; j < rule->n_ret; ++j) {
    const int id = rule->ret_ids[j];
    GILL_REQUIRE(id >= -V && id < V, "rule: retrieval id out of the vocabulary");
    r->ret[j] = id < 0 ? id + V : id;
    r->ret_raw[j] = id;
  }
  for (int j = 0; j < rule->n_gen; ++j) {
    const int id = rule->gen_ids[j];
    GILL_REQUIRE(id >= -V && id < V, "rule: generation id out of the vocabulary");
    r->gen[j] = id < 0 ? id + V : id;
  }
  r->ret0_raw = rule->n_ret > 0 ? rule->ret_ids[0] : INT64_MIN;
  r->special = (rule->n_ret > 0 || rule->n_gen > 0) && rule->n_ret > 0 && rule->n_gen > 0 && rule->ret_ids[0] != -1 &&
               rule->gen_ids[0] != -1;
  r->suppress = rule->step < rule->min_word_tokens;
  r->do_ret_scale = rule->ret_scale > 1.0;
  r->do_gen_scale = rule->gen_scale > 1.0;
  r->ret_scale = (float)rule->ret_scale;
  r->gen_scale = (float)rule->gen_scale;
  r->filter_value = (float)rule->filter_value;
  r->ret_eq_gen = rule->ret_eq_gen != 0;
  return 0;
}

extern "C" int gill_opt_pick_token(gill_opt* m, float* logits, int B, const gill_decode_rule* rule, int64_t* tokens, int ld,
                                   int col, int32_t* n_out, void* next_embeds_bf16, void* stream) {
  GILL_REQUIRE(m && logits && tokens && n_out && next_embeds_bf16, "null argument");
  DecodeRuleDev r;
  GILL_TRY(resolve_rule(m, rule, &r));
  return decode_rule_pick_launch(logits, B, m->cfg.vocab_size, r, m->embed, m->cfg.hidden_size, tokens, ld, col, n_out,
                                 (bf16_t*)next_embeds_bf16, (hipStream_t)stream);
}

extern "C" int gill_opt_next_token(gill_opt* m, const float* hidden, int B, int T, const gill_decode_rule* rule, float* logits_out,
                                   int64_t* tokens, int ld, int col, int32_t* n_out, void* next_embeds_bf16, void* stream) {
  GILL_REQUIRE(m && rule && tokens && n_out && next_embeds_bf16, "null argument");
  DecodeRuleDev r;
  GILL_TRY(resolve_rule(m, rule, &r));   // argument errors before anything is enqueued
  GILL_TRY(gill_opt_last_logits(m, hidden, B, T, logits_out, stream));
  return decode_rule_pick_launch(logits_out, B, m->cfg.vocab_size, r, m->embed, m->cfg.hidden_size, tokens, ld, col, n_out,
                                 (bf16_t*)next_embeds_bf16, (hipStream_t)stream);
}

static int resolve_sampler(const gill_decode_sampler* sm, DecodeSampler* o) {
  GILL_REQUIRE(sm, "null sampler");
  *o = DecodeSampler{sm->seed, sm->draw, sm->row0, sm->temperature, sm->top_p};
  return 0;
}

extern "C" int gill_opt_draw_token(gill_opt* m, float* logits, int B, const gill_decode_rule* rule, const gill_decode_sampler* sampler,
                                   int64_t* tokens, int ld, int col, int32_t* n_out, void* next_embeds_bf16, void* stream) {
  GILL_REQUIRE(m && logits && tokens && n_out && next_embeds_bf16, "null argument");
  DecodeRuleDev r;
  DecodeSampler sm;
  GILL_TRY(resolve_rule(m, rule, &r));
  GILL_TRY(resolve_sampler(sampler, &sm));
  return decode_sample_launch(logits, B, m->cfg.vocab_size, r, sm, m->embed, m->cfg.hidden_size, tokens, ld, col, n_out,
                              (bf16_t*)next_embeds_bf16, (hipStream_t)stream);
}

extern "C" int gill_opt_sample_token(gill_opt* m, const float* hidden, int B, int T, const gill_decode_rule* rule,
                                     const gill_decode_sampler* sampler, float* logits_out, int64_t* tokens, int ld, int col,
                                     int32_t* n_out, void* next_embeds_bf16, void* stream) {
  GILL_REQUIRE(m && hidden && logits_out && tokens && n_out && next_embeds_bf16, "null argument");
  DecodeRuleDev r;
  DecodeSampler sm;
  GILL_TRY(resolve_rule(m, rule, &r));   // argument errors before anything is enqueued
  GILL_TRY(resolve_sampler(sampler, &sm));
  GILL_TRY(decode_sample_check(B, m->cfg.vocab_size, r, sm, m->cfg.hidden_size, ld, col));
  GILL_TRY(gill_opt_last_logits(m, hidden, B, T, logits_out, stream));
  return decode_sample_launch(logits_out, B, m->cfg.vocab_size, r, sm, m->embed, m->cfg.hidden_size, tokens, ld, col, n_out,
                              (bf16_t*)next_embeds_bf16, (hipStream_t)stream);
}

extern "C" int gill_decode_uniforms(uint64_t seed, int32_t row, int32_t draw, int32_t first, int32_t count, float* u_out) {
  GILL_REQUIRE(u_out && row >= 0 && draw >= 0 && first >= 0 && count >= 0, "decode uniforms: bad argument");
  GILL_REQUIRE((int64_t)first + count <= 65536, "decode uniforms: columns are below 65536");
  for (int32_t j = 0; j < count; ++j) u_out[j] = decode_uniform(seed, (uint32_t)row, (uint32_t)draw, (uint32_t)(first + j));
  return 0;
}

extern "C" int gill_opt_decode_logits(gill_opt* m, const float* hidden, int B, int T, const gill_decode_rule* rule, float* logits_out,
                                      void* stream) {
  GILL_REQUIRE(m && rule, "null argument");
  DecodeRuleDev r;
  GILL_TRY(resolve_rule(m, rule, &r));
  GILL_TRY(gill_opt_last_logits(m, hidden, B, T, logits_out, stream));
  return decode_rule_launch(logits_out, B, m->cfg.vocab_size, r, (hipStream_t)stream);
}

extern "C" int gill_opt_filter_logits(gill_opt* m, const float* in, float* out, int B, double temperature, double top_p,
                                      double filter_value, int reciprocal, void* stream) {
  GILL_REQUIRE(m, "null handle");
  return decode_filter_launch(in, out, B, m->cfg.vocab_size, temperature, reciprocal != 0, top_p, filter_value,
                              (hipStream_t)stream);
}

// ---- ragged batched decoding: every row at its own length ----

extern "C" int gill_opt_decode_step(gill_opt* m, const void* new_embeds_bf16, const int32_t* lens_dev, int B, int len_bound, float* hidden_out,
                                    void* stream) {
  GILL_REQUIRE(m && new_embeds_bf16 && lens_dev && hidden_out, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "B exceeds the handle's workspace");
  GILL_REQUIRE(len_bound >= 1 && len_bound <= m->cfg.max_seq, "len_bound exceeds the handle's max_seq");
  GILL_REQUIRE(len_bound <= m->cfg.max_positions, "sequence longer than the position table");
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(opt_ensure_cache(m));
  GILL_TRY(opt_add_pos(m, new_embeds_bf16, lens_dev, B, 1, 0, s));
  const TfmDecode dec{lens_dev, m->dec_flags};
  GILL_TRY(m->run_layers(B, 1, s, 0, &dec, gill_opt_decode_uses_w8(m, B) != 0));
  GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_out, B, m->cfg.hidden_size, 1e-5f, s));
  return 0;
}

extern "C" int gill_opt_prefill_ids(gill_opt* m, const int64_t* ids, int B, int Tmax, const void* extra_rows_bf16, int n_extra, float* hidden_out,
                                    void* stream) {
  GILL_REQUIRE(m && ids && hidden_out, "null argument");
  OPT_REQUIRE_BF16_CACHE(m, "gill_opt_prefill_ids");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch && Tmax >= 1 && Tmax <= m->cfg.max_seq, "B / Tmax exceed the handle's workspace");
  GILL_REQUIRE(Tmax <= m->cfg.max_positions, "sequence longer than the position table");
  GILL_REQUIRE(n_extra >= 0 && (n_extra == 0 || extra_rows_bf16), "n_extra rows need a table");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size;
  GILL_TRY(opt_ensure_cache(m));
  // rows of embed_tokens (id >= 0) or of extra_rows (id < 0) + positions 2 + t -> the fp32 stream, then the cached forward at past_len = 0
  GILL_TRY(embed_tokens_launch(ids, m->embed, m->cfg.vocab_size, (const bf16_t*)extra_rows_bf16, n_extra, m->pos, 2, B, Tmax, D, m->h, s));
  GILL_TRY(m->run_layers(B, Tmax, s, 0));
  GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_out, B * Tmax, D, 1e-5f, s));
  return 0;
}

// ---- dialogue sessions: packed new tokens at per-row cache lengths ----

// opt_add_pos_kernel / embed_tokens_kernel per token position: packed row r = cu_new[b] + i takes the embedding row of ids[r] (id < 0: row
// -(id + 1) of extra) or emb[r], plus position 2 + lens[b] + i, the length read on the device and kept inside the table (the attention kernel of
// the same pass raises the flag).  A row that no sequence owns (r >= cu_new[B]) is zero-filled: finite, and nothing reads it.
__global__ __launch_bounds__(256) void opt_extend_embed_kernel(const int64_t* __restrict__ ids, const bf16_t* __restrict__ emb,
                                                               const bf16_t* __restrict__ table, int vocab, const bf16_t* __restrict__ extra,
                                                               int n_extra, const bf16_t* __restrict__ pos, int max_positions,
                                                               const int32_t* __restrict__ cu_new, const int32_t* __restrict__ lens, int B, int D,
                                                               float* __restrict__ out) {
  const int row = blockIdx.x;
  int b = -1;
  for (int j = 0; j < B; ++j)       // (uniform: every thread walks the same few words)
    if (row >= cu_new[j] && row < cu_new[j + 1]) { b = j; break; }
  float* o = out + (size_t)row * D;
  if (b < 0) {
    for (int c = threadIdx.x * 2; c < D; c += blockDim.x * 2) *reinterpret_cast<float2*>(o + c) = make_float2(0.f, 0.f);
    return;
  }
  const int n = lens[b];
  int p = (n < 0 ? 0 : n) + (row - cu_new[b]);
  p = 2 + (p > max_positions - 1 ? max_positions - 1 : p);
  const bf16_t* e;
  if (ids) {
    int64_t id = ids[row];
    if (id < 0 && n_extra > 0) {
      int64_t x = -(id + 1);
      if (x >= n_extra) x = n_extra - 1;
      e = extra + (size_t)x * D;
    } else {
      if (id < 0) id = 0;
      if (id >= vocab) id = vocab - 1;
      e = table + (size_t)id * D;
    }
  } else {
    e = emb + (size_t)row * D;
  }
  const bf16_t* pe = pos + (size_t)p * D;
  for (int c = threadIdx.x * 2; c < D; c += blockDim.x * 2) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(e + c);
    const uint32_t v = *reinterpret_cast<const uint32_t*>(pe + c);
    *reinterpret_cast<float2*>(o + c) = make_float2(bf2f((bf16_t)(u & 0xffff)) + bf2f((bf16_t)(v & 0xffff)), bf2f((bf16_t)(u >> 16)) + bf2f((bf16_t)(v >> 16)));
  }
}

// idx[b] = the packed row of sequence b's last new token (0 for a sequence without new tokens: gathered, never copied out)
__global__ void opt_extend_last_idx_kernel(const int32_t* __restrict__ cu_new, int B, int total_new, int32_t* __restrict__ idx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int last = cu_new[b + 1] - 1;
  idx[b] = (last >= cu_new[b] && last >= 0 && last < total_new) ? last : 0;
}
// dst[b][:] = src[b][:] for the sequences that brought new tokens
__global__ __launch_bounds__(256) void opt_extend_copy_last_kernel(const float* __restrict__ src, const int32_t* __restrict__ cu_new, int total_new,
                                                                   int D, float* __restrict__ dst) {
  const int b = blockIdx.x;
  const int last = cu_new[b + 1] - 1;
  if (!(last >= cu_new[b] && last >= 0 && last < total_new)) return;
  for (int c = threadIdx.x; c < D; c += blockDim.x) dst[(size_t)b * D + c] = src[(size_t)b * D + c];
}

extern "C" int gill_opt_extend(gill_opt* m, const int64_t* ids, const void* embeds_bf16, const void* extra_rows_bf16, int n_extra,
                               const int32_t* cu_new, const int32_t* lens_dev, int B, int total_new, int max_new, int len_bound, float* hidden_last,
                               float* hidden_all, void* stream) {
  GILL_REQUIRE(m && (ids || embeds_bf16) && cu_new && lens_dev && hidden_last, "null argument");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "B exceeds the handle's workspace");
  GILL_REQUIRE(max_new >= 1 && total_new >= max_new && (int64_t)total_new <= (int64_t)B * max_new &&
               (int64_t)total_new <= (int64_t)m->cfg.max_batch * m->cfg.max_seq, "extend: max_new <= total_new <= B * max_new, within the workspace");
  GILL_REQUIRE(len_bound >= max_new && len_bound <= m->cfg.max_seq, "len_bound exceeds the handle's max_seq");
  GILL_REQUIRE(len_bound <= m->cfg.max_positions, "sequence longer than the position table");
  GILL_REQUIRE(n_extra >= 0 && (n_extra == 0 || extra_rows_bf16), "n_extra rows need a table");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size;
  GILL_TRY(opt_ensure_cache(m));
  if (!m->ext_qkv) {
    GILL_TRY(m->pool.alloc(&m->ext_qkv, (size_t)m->cfg.max_batch * m->cfg.max_seq * 3 * D, false));
    GILL_TRY(m->pool.alloc(&m->ext_last, (size_t)m->cfg.max_batch * D, false));
  }
  hipLaunchKernelGGL(opt_extend_embed_kernel, dim3(total_new), dim3(256), 0, s, ids, (const bf16_t*)embeds_bf16, m->embed, m->cfg.vocab_size,
                     (const bf16_t*)extra_rows_bf16, n_extra, m->pos, m->cfg.max_positions, cu_new, lens_dev, B, D, m->h);
  GILL_CHECK_HIP(hipGetLastError());
  // the one layer loop over the packed rows, on the bf16 matrices (a w8 handle: the dequantised ones, as the prefill)
  TfmDecode dec{lens_dev, m->dec_flags};
  dec.cu_new = cu_new; dec.nseq = B; dec.max_new = max_new; dec.qkv = m->ext_qkv;
  GILL_TRY(m->run_layers(1, total_new, s, 0, &dec, false));
  if (hidden_all) GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_all, total_new, D, 1e-5f, s));
  hipLaunchKernelGGL(opt_extend_last_idx_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, cu_new, B, total_new, m->idx_dev);
  GILL_CHECK_HIP(hipGetLastError());
  GILL_TRY(gather_rows_launch(m->h, 1, m->idx_dev, B, D, m->gath, 1, s));
  GILL_TRY(layernorm_f32out_launch(m->gath, 1, m->lnfg, m->lnfb, m->ext_last, B, D, 1e-5f, s));
  hipLaunchKernelGGL(opt_extend_copy_last_kernel, dim3(B), dim3(256), 0, s, m->ext_last, cu_new, total_new, D, hidden_last);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- candidate ranking: packed continuations scored against the rows' cached prefixes, nothing appended ----

// One thread per candidate, its tokens in packed order: token_logprob = tgt - lse of a scored row (0 where the target is -100), token_rank, and
// the candidate's sum, count and mean (NaN over zero targets, HF's mean).  The candidate's range and parent are checked as the attention
// kernel checks them: one it treats as empty scores nothing.  A fixed summation order: the same inputs give the same bits.
__global__ __launch_bounds__(64) void opt_score_reduce_kernel(const float* __restrict__ lse, const float* __restrict__ tl, const int* __restrict__ rank,
                                                              const int64_t* __restrict__ target, const int32_t* __restrict__ cu_new,
                                                              const int32_t* __restrict__ parent, int C, int rows, int total_new, int max_new,
                                                              float* __restrict__ token_logprob, int32_t* __restrict__ token_rank,
                                                              float* __restrict__ score_sum, int32_t* __restrict__ n_scored,
                                                              float* __restrict__ score_mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int64_t lo = cu_new[c], hi = cu_new[c + 1];
  int64_t cnt = hi - lo;
  const int par = parent[c];
  if (cnt < 0 || cnt > max_new || lo < 0 || hi > total_new || par < 0 || par >= rows) cnt = 0;
  float sum = 0.f;
  int n = 0;
  for (int64_t i = 0; i < cnt; ++i) {
    const int64_t r = lo + i;
    const bool scored = target[r] != -100;
    const float lp = scored ? tl[r] - lse[r] : 0.f;
    token_logprob[r] = lp;
    if (token_rank) token_rank[r] = rank[r];
    if (scored) { sum += lp; ++n; }
  }
  score_sum[c] = sum;
  n_scored[c] = n;
  score_mean[c] = n > 0 ? sum / (float)n : __builtin_nanf("");
}

extern "C" int gill_opt_score_candidates(gill_opt* m, const int64_t* ids, const void* embeds_bf16, const void* extra_rows_bf16, int n_extra,
                                         const int32_t* cu_new, const int32_t* parent, const int32_t* plen, const int64_t* target, int C,
                                         int total_new, int max_new, int len_bound, float* token_logprob, int32_t* token_rank, float* score_sum,
                                         int32_t* n_scored, float* score_mean, float* hidden_all, int32_t* flags, void* stream) {
  GILL_REQUIRE(m && (ids || embeds_bf16) && cu_new && parent && plen && target && token_logprob && score_sum && n_scored && score_mean,
               "null argument");
  GILL_REQUIRE(m->kv_format == GILL_KV_BF16,
               "gill_opt_score_candidates: the handle's KV cache format is e4m3 (GILL_KV_E4M3); candidate scoring reads a bf16 cache");
  GILL_REQUIRE(!m->cache.empty(), "gill_opt_score_candidates: the handle has no KV cache yet (a cached entry such as gill_opt_extend fills it)");
  const int64_t R = (int64_t)m->cfg.max_batch * m->cfg.max_seq;
  GILL_REQUIRE(C >= 1 && C <= 65535, "score candidates: 1 <= C <= 65535");
  GILL_REQUIRE(max_new >= 1 && total_new >= 1 && (int64_t)total_new <= R, "score candidates: total_new within the workspace (max_batch * max_seq), max_new >= 1");
  GILL_REQUIRE(len_bound >= 1 && len_bound <= m->cfg.max_positions, "score candidates: sequence longer than the position table");
  GILL_REQUIRE(n_extra >= 0 && (n_extra == 0 || extra_rows_bf16), "n_extra rows need a table");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->cfg.hidden_size, V = m->cfg.vocab_size;
  if (!m->ext_qkv) {
    GILL_TRY(m->pool.alloc(&m->ext_qkv, (size_t)m->cfg.max_batch * m->cfg.max_seq * 3 * D, false));
    GILL_TRY(m->pool.alloc(&m->ext_last, (size_t)m->cfg.max_batch * D, false));
  }
  GILL_TRY(opt_ensure_loss_ws(m));
  const size_t fork_need = attention_fork_ws_bytes(C, m->cfg.num_heads, m->tfm.dp, max_new);
  if (fork_need > m->fork_ws_bytes) {
    unsigned char* ws = nullptr;
    GILL_TRY(m->pool.alloc(&ws, fork_need, false));
    m->fork_ws = ws; m->fork_ws_bytes = fork_need;
  }
  // rows no candidate owns: log-probability 0, rank -1
  GILL_CHECK_HIP(hipMemsetAsync(token_logprob, 0, sizeof(float) * (size_t)total_new, s));
  if (token_rank) GILL_CHECK_HIP(hipMemsetAsync(token_rank, 0xFF, sizeof(int32_t) * (size_t)total_new, s));
  // packed row cu_new[c] + i: its embedding (or visual) row + position 2 + plen[c] + i
  hipLaunchKernelGGL(opt_extend_embed_kernel, dim3(total_new), dim3(256), 0, s, ids, (const bf16_t*)embeds_bf16, m->embed, V,
                     (const bf16_t*)extra_rows_bf16, n_extra, m->pos, m->cfg.max_positions, cu_new, plen, C, D, m->h);
  GILL_CHECK_HIP(hipGetLastError());
  // the one layer loop over the packed rows in fork mode, on the bf16 matrices (a w8 handle: the dequantised ones, the extend pass's rule)
  TfmDecode dec{nullptr, flags};
  dec.cu_new = cu_new; dec.nseq = C; dec.max_new = max_new; dec.qkv = m->ext_qkv;
  dec.fork_parent = parent; dec.fork_plen = plen; dec.fork_rows = m->cfg.max_batch; dec.fork_ws = m->fork_ws; dec.fork_ws_bytes = m->fork_ws_bytes;
  GILL_TRY(m->run_layers(1, total_new, s, 0, &dec, false));
  GILL_TRY(layernorm_launch(m->h, 1, m->lnfg, m->lnfb, m->xn_bf, total_new, D, 1e-5f, s));
  if (hidden_all) GILL_TRY(layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_all, total_new, D, 1e-5f, s));
  GILL_TRY(lm_loss_launch(m->xn_bf, m->lm_head, target, total_new, V, D, m->loss_lse, m->loss_tl, m->loss_rank, nullptr, m->loss_ws, s));
  hipLaunchKernelGGL(opt_score_reduce_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, m->loss_lse, m->loss_tl, m->loss_rank, target, cu_new, parent, C,
                     m->cfg.max_batch, total_new, max_new, token_logprob, token_rank, score_sum, n_scored, score_mean);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

// the arguments both ragged decisions share, checked before anything is enqueued
static int ragged_args(const gill_opt* m, int B, const gill_decode_rule* rule, const gill_decode_sampler* sampler, int max_steps, DecodeRuleDev* r,
                       DecodeSampler* sm) {
  GILL_REQUIRE(B >= 1 && max_steps >= 0, "ragged decode: bad shape");
  GILL_TRY(resolve_rule(m, rule, r));
  if (sampler) {
    GILL_TRY(resolve_sampler(sampler, sm));
    sm->draw = 0; sm->row0 = 0;     // the row's own step and row_id take their place
  }
  return 0;
}

extern "C" int gill_opt_pick_token_ragged(gill_opt* m, float* logits, int B, const gill_decode_rule* rule, int max_steps,
                                          const gill_decode_sampler* sampler, int32_t* state, int64_t* tokens, int ld, void* next_embeds_bf16,
                                          void* stream) {
  GILL_REQUIRE(m && logits && state && tokens && next_embeds_bf16, "null argument");
  DecodeRuleDev r;
  DecodeSampler sm;
  GILL_TRY(ragged_args(m, B, rule, sampler, max_steps, &r, &sm));
  return decode_ragged_launch(logits, B, m->cfg.vocab_size, r, rule->min_word_tokens, max_steps, sampler ? &sm : nullptr, state, m->dec_flags,
                              m->embed, m->cfg.hidden_size, tokens, ld, (bf16_t*)next_embeds_bf16, (hipStream_t)stream);
}

// the ragged decision over B rows; clamp_flags: the [>= B] words the rows' attention step raised (the handle's dec_flags, or br_flags for branches)
static int opt_next_token_ragged(gill_opt* m, const float* hidden, int B, const gill_decode_rule* rule, int max_steps,
                                 const gill_decode_sampler* sampler, float* logits_out, int32_t* state, int64_t* tokens, int ld,
                                 void* next_embeds_bf16, int32_t* clamp_flags, void* stream) {
  GILL_REQUIRE(m && hidden && logits_out && state && tokens && next_embeds_bf16, "null argument");
  DecodeRuleDev r;
  DecodeSampler sm;
  GILL_TRY(ragged_args(m, B, rule, sampler, max_steps, &r, &sm));      // argument errors before anything is enqueued
  if (sampler) GILL_TRY(decode_sample_check(B, m->cfg.vocab_size, r, sm, m->cfg.hidden_size, kDecodeMaxIds + 1, 0));
  GILL_REQUIRE(ld >= 1 && m->cfg.hidden_size % 2 == 0, "ragged decode: bad shape");
  GILL_TRY(gill_opt_last_logits(m, hidden, B, 1, logits_out, stream));
  return decode_ragged_launch(logits_out, B, m->cfg.vocab_size, r, rule->min_word_tokens, max_steps, sampler ? &sm : nullptr, state, clamp_flags,
                              m->embed, m->cfg.hidden_size, tokens, ld, (bf16_t*)next_embeds_bf16, (hipStream_t)stream);
}

extern "C" int gill_opt_next_token_ragged(gill_opt* m, const float* hidden, int B, const gill_decode_rule* rule, int max_steps,
                                          const gill_decode_sampler* sampler, float* logits_out, int32_t* state, int64_t* tokens, int ld,
                                          void* next_embeds_bf16, void* stream) {
  GILL_REQUIRE(m, "null argument");
  return opt_next_token_ragged(m, hidden, B, rule, max_steps, sampler, logits_out, state, tokens, ld, next_embeds_bf16, m->dec_flags, stream);
}

// ---- branch decode: S sampled continuations of cached dialogues, one token each per step (csrc/attention_branch.hip) ----

#define OPT_REQUIRE_BRANCH_BF16(m, what) \
  GILL_REQUIRE((m)->kv_format == GILL_KV_BF16, what ": the handle's KV cache format is e4m3 (GILL_KV_E4M3); a branch cache is bf16 beside a bf16 cache")

extern "C" int gill_opt_branch_reserve(gill_opt* m, int max_branches, int branch_capacity) {
  GILL_REQUIRE(m, "null handle");
  OPT_REQUIRE_BRANCH_BF16(m, "gill_opt_branch_reserve");
  const int D = m->cfg.hidden_size, H = m->cfg.num_heads, dp = m->tfm.dp, dpv = m->tfm.dpv;
  GILL_REQUIRE(dp == 64 || dp == 80 || dp == 128, "gill_opt_branch_reserve: branch attention needs a head dim of 64, 80 or 128");
  GILL_REQUIRE(max_branches >= 1 && branch_capacity >= 1 && branch_capacity <= 1024, "gill_opt_branch_reserve: max_branches >= 1, 1 <= branch_capacity <= 1024");
  // every buffer a step over max_branches rows writes: the stream, nbuf, ff and o hold max_batch * max_seq rows; the projection lands in
  // Tfm::q, which takes 3 * S * D elements (Tfm::alloc: the larger of the flash operand and 48 D)
  const int64_t R = (int64_t)m->cfg.max_batch * m->cfg.max_seq;
  const int64_t qn = (int64_t)m->cfg.max_batch * H * round_up(m->cfg.max_seq, 32) * dp, qdec = (int64_t)48 * D;
  GILL_REQUIRE(max_branches <= R, "gill_opt_branch_reserve: max_branches exceeds the workspace rows (max_batch * max_seq)");
  GILL_REQUIRE((int64_t)3 * max_branches * D <= (qn > qdec ? qn : qdec), "gill_opt_branch_reserve: the projection of max_branches rows (3 * S * D) exceeds the workspace");
  const int bpitch = round_up(branch_capacity, 32);
  if (m->br_slab && m->br_rows >= max_branches && m->br_cache[0].pad >= bpitch) return 0;
  if (m->br_slab) {
    GILL_CHECK_HIP(hipDeviceSynchronize());
    GILL_CHECK_HIP(hipFree(m->br_slab));
    m->br_slab = nullptr; m->br_bytes = 0; m->br_rows = 0; m->br_flags = nullptr; m->br_cache.clear();
  }
  const size_t kn = (size_t)max_branches * H * bpitch * dp, vn = (size_t)max_branches * H * dpv * bpitch;     // elements; both byte sizes % 256 == 0
  const size_t nl = m->layers.size();
  const size_t bytes = nl * (kn + vn) * sizeof(bf16_t) + (((size_t)max_branches * sizeof(int32_t) + 255) & ~(size_t)255);
  void* p = nullptr;
  GILL_CHECK_HIP(hipMalloc(&p, bytes));
  if (hipMemset(p, 0, bytes) != hipSuccess) {
    (void)hipFree(p);
    GILL_REQUIRE(false, "gill_opt_branch_reserve: hipMemset failed");
  }
  m->br_slab = p; m->br_bytes = bytes; m->br_rows = max_branches;
  bf16_t* base = (bf16_t*)p;
  m->br_cache.assign(nl, TfmKv{nullptr, nullptr, bpitch});
  for (size_t i = 0; i < nl; ++i) {
    m->br_cache[i].k = base + i * (kn + vn);
    m->br_cache[i].vt = base + i * (kn + vn) + kn;
    m->br_cache[i].fmt = GILL_KV_BF16;
  }
  m->br_flags = (int32_t*)(base + nl * (kn + vn));
  return 0;
}

extern "C" int64_t gill_opt_branch_bytes(const gill_opt* m) { return m ? (int64_t)m->br_bytes : 0; }

extern "C" int gill_opt_decode_step_branch(gill_opt* m, const void* new_embeds_bf16, const int32_t* lens_dev, const int32_t* gstart,
                                           const int32_t* gparent, const int32_t* gplen, int S, int G, int len_bound, float* hidden_out,
                                           void* stream) {
  GILL_REQUIRE(m && new_embeds_bf16 && lens_dev && gstart && gparent && gplen && hidden_out, "null argument");
  OPT_REQUIRE_BRANCH_BF16(m, "gill_opt_decode_step_branch");
  GILL_REQUIRE(!m->cache.empty(), "gill_opt_decode_step_branch: the handle has no KV cache yet (a cached entry such as gill_opt_extend fills it)");
  GILL_REQUIRE(m->br_slab, "gill_opt_decode_step_branch: no branch cache (gill_opt_branch_reserve)");
  GILL_REQUIRE(S >= 1 && S <= m->br_rows, "gill_opt_decode_step_branch: S exceeds the reserved branches");
  GILL_REQUIRE(G >= 1 && G <= S, "gill_opt_decode_step_branch: 1 <= G <= S");
  GILL_REQUIRE(len_bound >= 1 && len_bound <= m->cfg.max_positions, "sequence longer than the position table");
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(opt_add_pos(m, new_embeds_bf16, lens_dev, S, 1, 0, s));
  TfmDecode dec{lens_dev, m->br_flags};
  dec.br = m->br_cache.data(); dec.br_main = m->cache.data();
  dec.br_gstart = gstart; dec.br_gparent = gparent; dec.br_gplen = gplen;
  dec.br_groups = G; dec.br_rows = m->br_rows; dec.br_main_rows = m->cfg.max_batch;
  GILL_TRY(m->run_layers(S, 1, s, 0, &dec, gill_opt_decode_uses_w8(m, S) != 0));
  return layernorm_f32out_launch(m->h, 1, m->lnfg, m->lnfb, hidden_out, S, m->cfg.hidden_size, 1e-5f, s);
}

extern "C" int gill_opt_next_token_branch(gill_opt* m, const float* hidden, int S, const gill_decode_rule* rule, int max_steps,
                                          const gill_decode_sampler* sampler, float* logits_out, int32_t* state, int64_t* tokens, int ld,
                                          void* next_embeds_bf16, void* stream) {
  GILL_REQUIRE(m, "null argument");
  GILL_REQUIRE(m->br_slab && S >= 1 && S <= m->br_rows, "gill_opt_next_token_branch: S exceeds the reserved branches (gill_opt_branch_reserve)");
  return opt_next_token_ragged(m, hidden, S, rule, max_steps, sampler, logits_out, state, tokens, ld, next_embeds_bf16, m->br_flags, stream);
}

extern "C" int gill_opt_branch_adopt(gill_opt* m, int sidx, int r, int plen, int count, void* stream) {
  GILL_REQUIRE(m, "null handle");
  OPT_REQUIRE_BRANCH_BF16(m, "gill_opt_branch_adopt");
  GILL_REQUIRE(!m->cache.empty() && m->br_slab, "gill_opt_branch_adopt: the handle needs its KV cache and a branch cache (gill_opt_branch_reserve)");
  KvBranchAdoptArgs a;
  a.Sb = m->br_rows; a.Bc = m->cfg.max_batch; a.H = m->cfg.num_heads; a.dp = m->tfm.dp; a.dpv = m->tfm.dpv;
  a.s = sidx; a.r = r; a.plen = plen; a.count = count;
  for (size_t i = 0; i < m->layers.size(); ++i) {      // the first layer's argument check speaks for all: nothing is launched before it
    a.Kb = m->br_cache[i].k; a.Vtb = m->br_cache[i].vt; a.K = m->cache[i].k; a.Vt = m->cache[i].vt;
    a.pitch = m->cache[i].pad; a.bpitch = m->br_cache[i].pad;
    GILL_TRY(kv_branch_adopt_launch(a, (hipStream_t)stream));
  }
  return 0;
}
