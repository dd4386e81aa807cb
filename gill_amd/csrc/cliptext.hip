// CLIP text tower (transformers CLIPTextModel as the Stable Diffusion pipeline calls it: gill/custom_sd.py:305-309 and :353-357
// read `text_encoder(input_ids)[0]`, last_hidden_state after final_layer_norm) on gfx950, through the same GEMM / attention /
// LayerNorm kernels as the vision tower (clip.hip) and the OPT engine.
//   ids (B,T) int32 -> token_embedding[ids] + position_embedding[0..T) -> L x { LN1, QKV (bias), causal softmax(QK^T/sqrt(d)) V,
//   out_proj, +res, LN2, fc1, quick_gelu | gelu, fc2, +res } -> final_layer_norm -> (B,T,D) bf16 and / or fp32.
// fp32 residual stream, bf16 GEMM operands, fp32 accumulation (as clip.hip / opt.hip).  No attention mask: the reference passes
// none (neither SD-1.5's nor SD-2.1's text_encoder config sets use_attention_mask), so padding positions attend causally like
// any other.  Two kernels live here, the two ends of the tower; everything between them is the shared block of tfm.h.
// Launches per forward: 1 + 7 L + 1 without split-K (86 at L = 12, 163 at L = 23); a GEMM that gemm_pick_splitk() splits
// (few rows) adds its reducer.
#include "tfm.h"

namespace {
constexpr int kFinalLnMaxOctets = 4;    // final LayerNorm keeps a row in registers: D <= 8 * 64 * 4 = 2048
}  // namespace

struct gill_clip_text {
  gill_clip_text_config cfg;
  DevPool pool;
  float* tok = nullptr;       // [vocab][D] fp32: the rows enter the fp32 stream unrounded
  float* pos = nullptr;       // [max_positions][D]
  float *fing = nullptr, *finb = nullptr;
  std::vector<TfmLayer> layers;
  Tfm tfm;
  float* h = nullptr;         // [B*T][D] the fp32 stream
};

// h[b*T + t][:] = token_embedding[ids[b*T + t]][:] + position_embedding[t][:]       (CLIPTextEmbeddings.forward)
// One wave per row, 16-byte loads and stores; the id is wave-uniform, read once from device memory.  Memory-bound: 2 reads + 1
// write of D floats per row.  The caller validates the ids; the clamp keeps a bad one inside the table instead of faulting.
__global__ __launch_bounds__(256) void clip_text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                              const float* __restrict__ pos, int rows, int T, int D, int vocab,
                                                              float* __restrict__ h) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* e = reinterpret_cast<const float4*>(tok + (size_t)id * D);
  const float4* p = reinterpret_cast<const float4*>(pos + (size_t)(row % T) * D);
  float4* o = reinterpret_cast<float4*>(h + (size_t)row * D);
  for (int c = lane; c < D / 4; c += 64) {
    const float4 a = e[c], b = p[c];
    o[c] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
}

// final_layer_norm over the fp32 stream: y = (x - mean) * rstd * g + b, written as bf16 (the context gill_sd_denoise consumes)
// and / or fp32 (what return_prompts_only hands back) in one pass.  One wave per row; lane l owns the octets l, l + 64, ... of the
// row, which is read once and stays in registers; exact two-pass mean / variance on the registers.  The bf16 value is the
// rounding of the fp32 value that is stored, so the two outputs can never disagree.
template <int MAXV>
__global__ __launch_bounds__(256) void clip_text_final_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, bf16_t* __restrict__ y16,
                                                                 float* __restrict__ y32, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = D >> 3;
  const float* xr = x + (size_t)row * D;
  float v[MAXV][8];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int o = lane + k * 64;
    if (o < nv) {
      const float4 a = *reinterpret_cast<const float4*>(xr + o * 8), b = *reinterpret_cast<const float4*>(xr + o * 8 + 4);
      v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; v[k][3] = a.w; v[k][4] = b.x; v[k][5] = b.y; v[k][6] = b.z; v[k][7] = b.w;
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[k][i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[k][i] = 0.f;
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k)
    if (lane + k * 64 < nv) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float dlt = v[k][i] - mean; ss += dlt * dlt; }
    }
  const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int o = lane + k * 64;
    if (o < nv) {
      const float4 g0 = *reinterpret_cast<const float4*>(gamma + o * 8), g1 = *reinterpret_cast<const float4*>(gamma + o * 8 + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(beta + o * 8), b1 = *reinterpret_cast<const float4*>(beta + o * 8 + 4);
      const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float r[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = (v[k][i] - mean) * rstd * g[i] + bb[i];
      if (y32) {
        float* yr = y32 + (size_t)row * D + o * 8;
        *reinterpret_cast<float4*>(yr) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(yr + 4) = make_float4(r[4], r[5], r[6], r[7]);
      }
      if (y16) {
        uint4 u;
        u.x = pack_bf2(r[0], r[1]); u.y = pack_bf2(r[2], r[3]); u.z = pack_bf2(r[4], r[5]); u.w = pack_bf2(r[6], r[7]);
        *reinterpret_cast<uint4*>(y16 + (size_t)row * D + o * 8) = u;
      }
    }
  }
}

extern "C" int gill_clip_text_create(gill_clip_text** out, const gill_clip_text_config* cfg, const gill_tensor* weights, int n_weights) {
  GILL_REQUIRE(out && cfg && weights, "null argument");
  const int D = cfg->hidden_size, F = cfg->intermediate_size, H = cfg->num_heads, V = cfg->vocab_size, P = cfg->max_positions;
  GILL_REQUIRE(D > 0 && F > 0 && D % 64 == 0 && F % 64 == 0 && H > 0 && D % H == 0, "CLIP text dims must be multiples of 64");
  GILL_REQUIRE(D <= 8 * 64 * kFinalLnMaxOctets, "CLIP text hidden size above 2048");
  GILL_REQUIRE(V >= 1 && P >= 1 && cfg->max_batch >= 1 && cfg->num_layers >= 1, "bad CLIP text geometry");
  GILL_REQUIRE(cfg->hidden_act == GILL_CLIP_TEXT_ACT_QUICK_GELU || cfg->hidden_act == GILL_CLIP_TEXT_ACT_GELU,
               "CLIP text hidden_act must be quick_gelu (0) or gelu (1)");
  const int hd = D / H;
  GILL_REQUIRE(attn_padded_dim(hd) == hd, "CLIP text head dim must be one of 48/64/80/128/160");
  gill_clip_text* m = new gill_clip_text();
  m->cfg = *cfg;
  WeightTable wt(weights, n_weights);
  hipStream_t s = nullptr;
  int rc = 0;
  auto fail = [&](int r) { delete m; return r; };
  const std::string tm = "text_model.";
  if ((rc = load_f32(wt, m->pool, tm + "embeddings.token_embedding.weight", (int64_t)V * D, &m->tok, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, tm + "embeddings.position_embedding.weight", (int64_t)P * D, &m->pos, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, tm + "final_layer_norm.weight", D, &m->fing, s))) return fail(rc);
  if ((rc = load_f32(wt, m->pool, tm + "final_layer_norm.bias", D, &m->finb, s))) return fail(rc);
  m->layers.resize(cfg->num_layers);
  const TfmNames names = {{"self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj."}, "self_attn.out_proj.", "mlp.fc1.", "mlp.fc2.",
                          "layer_norm1.", "layer_norm2."};
  // row-major weights, not the STREAM64 layout: kept as found
  for (int i = 0; i < cfg->num_layers; ++i)
    if ((rc = tfm_load_layer(wt, m->pool, tm + "encoder.layers." + std::to_string(i) + ".", names, D, F, false, &m->layers[i], s)))
      return fail(rc);
  if ((rc = m->pool.alloc(&m->h, (size_t)cfg->max_batch * P * D))) return fail(rc);
  // fuse_ln stays off (a stand-alone LayerNorm at every seam): kept as found.  The split-K partials are capped at 16 Mi floats:
  // gemm_pick_splitk() splits only under-filled grids (< 384 tiles of 128 x 128, at most 16 ways aiming at 512 workgroups), so
  // splitk * M * N stays near 512 * 128 * 128 floats whatever max_batch is; that only this engine caps is kept as found
  if ((rc = m->tfm.alloc(m->pool, cfg->max_batch, P, D, F, H, hd, round_up(hd, 32), (size_t)16 << 20))) return fail(rc);
  if (hipDeviceSynchronize() != hipSuccess) { gill_set_error("clip text create: device sync failed"); return fail(-1); }
  *out = m;
  return 0;
}

extern "C" void gill_clip_text_destroy(gill_clip_text* h) { delete h; }

extern "C" int gill_clip_text_forward(gill_clip_text* m, const int32_t* ids, int B, int T, void* out_bf16, float* out_f32,
                                      void* stream) {
  GILL_REQUIRE(m && ids, "null argument");
  GILL_REQUIRE(out_bf16 || out_f32, "no output buffer");
  GILL_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "batch exceeds the CLIP text handle's max_batch");
  GILL_REQUIRE(T >= 1 && T <= m->cfg.max_positions, "sequence length exceeds the CLIP text handle's max_positions");
  hipStream_t s = (hipStream_t)stream;
  const gill_clip_text_config& c = m->cfg;
  const int D = c.hidden_size, R = B * T;
  const int act = c.hidden_act == GILL_CLIP_TEXT_ACT_GELU ? ACT_GELU : ACT_QUICK_GELU;
  hipLaunchKernelGGL(clip_text_embed_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, ids, m->tok, m->pos, R, T, D, c.vocab_size, m->h);
  GILL_CHECK_HIP(hipGetLastError());
  GILL_TRY((TfmRun{m->tfm, s}.layers(m->h, m->layers.data(), (int)m->layers.size(), B, T, act, true)));
  hipLaunchKernelGGL((clip_text_final_ln_kernel<kFinalLnMaxOctets>), dim3(cdiv(R, 4)), dim3(256), 0, s, m->h, m->fing, m->finb,
                     (bf16_t*)out_bf16, out_f32, R, D, 1e-5f);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
